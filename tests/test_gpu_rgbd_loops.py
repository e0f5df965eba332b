"""script.train with RGB-D batches (`args.use_depth`, batch[2] the depth batch) on training.GraphedTrainStep: three seeded batches of
2x3x32x48 and one short batch, one epoch, against the restated reference body (script._FORCE_RESTATED) on the same batches.  The
restated run also switches the one-launch fusion gate off (layers._FUSED_FUSION_GATE), so the two sides share neither the step nor the
gate node: a fault in either does not cancel.

Bounds, those of the loop's test without depth (tests/test_gpu_train_loop.py): loss average within 2e-5 |ref| + 1e-5; areas within an
L1 distance per histogram of 2 x (pixels whose top-2 margin of the restated run's main head is below 1e-3); parameters by
synth.assert_weights_close_after_adam.  BatchNorm is frozen in this loop, and the seed is the one tests/test_gpu_rgbd_grad_parity.py
chose for its conditioning.

The supervised loops (train_seg_ue, train_seg) keep the restated body for RGB-D batches; tests/test_train_seg*_host.py pin that."""
import argparse

import numpy as np
import pytest
import torch

from tests.synth import assert_weights_close_after_adam, grad_sample_index, synth_input, synth_labels, synth_state_dict
from tests.train_loop_cases import CLASS_WEIGHTS, IGNORE_IDX, NEAR_MARGIN

pytestmark = pytest.mark.gpu
DEV = 'cuda'
HW = (32, 48)
BATCHES = (2, 2, 2, 1)
FULL = 3
SEED = 2
NUM_CLASSES = 5
LR, WD, TOT_ITER = 5e-4, 5e-4, 6.0
LOSS_RTOL, LOSS_ATOL = 2e-5, 1e-5          # tests/test_gpu_train_loop.py


def _batches(depth_scale=1.0):
    return [(synth_input((b, 3) + HW, SEED + i).to(DEV), synth_labels((b,) + HW, NUM_CLASSES, SEED + i).to(DEV),
             (depth_scale * synth_input((b, 1) + HW, SEED + 100 + i)).to(DEV)) for i, b in enumerate(BATCHES)]


class Loader(object):
    def __init__(self, batches, spy):
        self.batches, self.spy = batches, spy

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        for i, b in enumerate(self.batches):
            self.spy['inside'] = i >= 1
            yield b
        self.spy['inside'] = False


class Writer(object):
    def __init__(self):
        self.records = []

    def add_scalar(self, tag, value, idx):
        self.records.append([tag, float(value), int(idx)])


def _model():
    from mspl_amd import models
    a = argparse.Namespace(s=2.0, channels=3, num_classes=1000)
    m = models.ESPDNetwithUncertaintyEstimation(a, classes=NUM_CLASSES, dataset='greenhouse', trainable_fusion=True, fix_pyr_plane_proj=True)
    m.load_state_dict(synth_state_dict(m.state_dict(), SEED))
    return m.to(DEV).eval()


def _sample(m):
    return torch.cat([t.detach().reshape(-1)[grad_sample_index(t.numel()).to(DEV)] for t in m.parameters()]).cpu().numpy()


def _run(restated=False, depth_scale=1.0, use_depth=True, lanes=None, model=None, expect_raise=None):
    """One epoch of script.train on the seeded batches -> dict(loss_avg, areas, params, spy, model, optimizer, near)."""
    from mspl_amd import layers, losses, script, training
    spy = {'inside': False, 'inside_calls': [], 'graph_built': 0, 'graph_calls': 0, 'eager_steps': 0, 'eager_depth': [], 'reads': [],
           'visual': [], 'near': []}
    mp = pytest.MonkeyPatch()
    try:
        def counted(owner, attr):
            orig = getattr(owner, attr)

            def wrapper(*a, **k):
                if spy['inside']:
                    spy['inside_calls'].append(attr)
                return orig(*a, **k)
            mp.setattr(owner, attr, wrapper)
        if not restated:
            counted(torch.cuda, 'synchronize')
            counted(torch.Tensor, 'item')
            counted(torch.Tensor, 'cpu')
        g_init, g_call, t_step = training.GraphedTrainStep.__init__, training.GraphedTrainStep.__call__, training.train_step
        m_read, m_add = training.TrainMeters.read, training.TrainMeters.add

        def init(self, *a, **k):
            spy['graph_built'] += 1
            spy['building'] = True
            try:
                g_init(self, *a, **k)
            finally:
                spy['building'] = False

        def call(self, *a, **k):
            spy['graph_calls'] += 1
            return g_call(self, *a, **k)

        def step(*a, **k):
            if not spy.get('building'):
                spy['eager_steps'] += 1
                spy['eager_depth'].append(k.get('depth') is not None)
            return t_step(*a, **k)

        def read(self):
            r = m_read(self)
            spy['reads'].append(r)
            return r

        def add(self, pred, *a, **k):              # (the restated body hands its main head to the meters: the near-ties of the run)
            top = pred.detach().topk(2, dim=1).values
            spy['near'].append(((top[:, 0] - top[:, 1]) < NEAR_MARGIN).sum())
            return m_add(self, pred, *a, **k)
        mp.setattr(training.GraphedTrainStep, '__init__', init)
        mp.setattr(training.GraphedTrainStep, '__call__', call)
        mp.setattr(training, 'train_step', step)
        mp.setattr(training.TrainMeters, 'read', read)
        if restated:
            mp.setattr(training.TrainMeters, 'add', add)
            mp.setattr(layers, '_FUSED_FUSION_GATE', False)
        mp.setattr(script, '_FORCE_RESTATED', bool(restated))

        m = _model() if model is None else model
        loader = Loader(_batches(depth_scale), spy)
        crit = losses.UncertaintyWeightedSegmentationLoss(NUM_CLASSES, class_weights=torch.tensor(CLASS_WEIGHTS), ignore_idx=IGNORE_IDX,
                                                          device=DEV)
        opt = torch.optim.Adam(m.parameters(), lr=LR, weight_decay=WD)
        ns = {'in_training_visualization_img': lambda model, **kw: spy['visual'].append(sorted(kw))}
        assert 'train' in script.patch_script(ns, train=True)
        args = argparse.Namespace(model='espdnetue', use_depth=use_depth, use_uncertainty=True, use_traversable=False, learning_rate=LR,
                                  power=0.9)
        if lanes is not None:
            args.train_lanes = lanes
        writer = Writer()
        run = lambda: ns['train'](loader, m, crit, DEV, None, opt, TOT_ITER, 0, 0, args, None, None, None, 7, None, writer, None)  # noqa: E731
        if expect_raise is not None:
            with pytest.raises(RuntimeError, match=expect_raise):
                run()
            return {'spy': spy, 'model': m}
        run()
        near = int(torch.stack(spy['near']).sum()) if spy['near'] else None
        return {'loss_avg': writer.records[0][1], 'areas': spy['reads'][0]['areas'], 'params': _sample(m), 'spy': spy, 'model': m,
                'optimizer': opt, 'near': near}
    finally:
        mp.undo()


_RUNS = {}


def _cached(**kw):
    key = tuple(sorted(kw.items()))
    if key not in _RUNS:
        _RUNS[key] = _run(**kw)
    return _RUNS[key]


def test_rgbd_loop_runs_on_one_graphed_step_without_host_sync():
    got = _cached()
    spy = got['spy']
    assert spy['graph_built'] == 1
    assert spy['graph_calls'] == FULL and spy['eager_steps'] == len(BATCHES) - FULL
    assert spy['eager_depth'] == [True] * (len(BATCHES) - FULL)          # the short batch's eager step got its depth batch
    assert spy['inside_calls'] == []
    assert len(spy['reads']) == 1 and spy['reads'][0]['steps'] == len(BATCHES)
    assert len(got['optimizer'].state) == 0                               # the caller's optimizer never stepped
    step = got['model'].__dict__['_mspl_train_loop']['step']
    assert step.depth is not None and tuple(step.depth.shape) == (2, 1) + HW
    assert step.lanes == 2                                                # the default of args.train_lanes, with depth
    assert spy['visual'] == [['class_encoding', 'data', 'depths', 'device', 'epoch', 'images', 'labels', 'writer']]


def test_rgbd_loop_against_the_restated_body():
    fast, slow = _cached(), _cached(restated=True)
    assert slow['spy']['graph_built'] == 0 and len(slow['optimizer'].state) > 0
    ref = slow['loss_avg']
    dev, bound = abs(fast['loss_avg'] - ref), LOSS_RTOL * abs(ref) + LOSS_ATOL
    print('loss average %.9g against %.9g (deviation %.2e, allowed %.2e)' % (fast['loss_avg'], ref, dev, bound))
    assert dev <= bound
    cap = 2 * slow['near']
    l1 = np.abs(fast['areas'] - slow['areas']).sum(1)
    print('    areas L1 per histogram', l1.tolist(), 'allowed', cap)
    assert (l1 <= cap).all()
    assert_weights_close_after_adam(fast['params'], slow['params'], LR, len(BATCHES))


def test_another_depth_batch_gives_another_result():
    """Depth scaled by -4: the float64 oracle's loss of the first batch moves by 1.2e-2 relative (by 1.3e-4 for another seeded depth)."""
    a = _cached()
    b = _run(depth_scale=-4.0, lanes=1)
    assert b['spy']['graph_built'] == 1
    assert abs(a['loss_avg'] - b['loss_avg']) > 100 * (LOSS_RTOL * abs(a['loss_avg']) + LOSS_ATOL)


def test_depth_with_nid_takes_the_restated_body():
    from mspl_amd import losses, script
    m = _model()
    crit = losses.UncertaintyWeightedSegmentationLoss(NUM_CLASSES, class_weights=torch.tensor(CLASS_WEIGHTS), ignore_idx=IGNORE_IDX, device=DEV)
    opt = torch.optim.Adam(m.parameters(), lr=LR, weight_decay=WD)
    nid = losses.NIDLoss(label_bin=NUM_CLASSES)
    args = argparse.Namespace(model='espdnetue', use_depth=True, use_uncertainty=True)
    assert script._fast_path(m, crit, opt, args, None)
    assert not script._fast_path(m, crit, opt, args, nid)
    args.use_depth = False
    assert script._fast_path(m, crit, opt, args, nid)


def test_a_step_captured_with_depth_refuses_a_loop_without_and_the_reverse():
    from mspl_amd import training
    _run(use_depth=False, model=_cached()['model'], expect_raise='depth')
    # the reverse, on the step itself: captured without depth, called with one
    m = _model()
    x, y, xd = _batches()[0]
    gs = training.GraphedTrainStep(m, x, y, torch.ones(NUM_CLASSES), ignore_idx=IGNORE_IDX, lanes=1)
    with pytest.raises(RuntimeError, match='depth'):
        gs(x, y, xd)
    gs(x, y)


def test_supervised_step_refuses_a_depth_mismatch():
    from mspl_amd import losses, supervised
    m = _model().train()
    x, y, xd = _batches()[0]
    crit = losses.SegmentationLoss(n_classes=NUM_CLASSES, device=DEV, ignore_idx=IGNORE_IDX, class_weights=torch.tensor(CLASS_WEIGHTS))
    gs = supervised.GraphedSupervisedStep(m, x, y, crit, depth=xd)
    with pytest.raises(RuntimeError, match='depth'):
        gs(x, y)
    gs(x, y, xd)
