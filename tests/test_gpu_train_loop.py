"""mspl_amd.script.train -- the drop-in for the reference's self-training loop (uest_seg_multi_os.py:958-1089) -- against the golden
written by the reference's own train() (tests/golden/make_train_loop_golden.py)."""
import argparse
import json
import os

import numpy as np
import pytest
import torch

from tests.conftest import GOLDEN
from tests.optim_shadow import StepAudit
from tests.synth import assert_weights_close_after_adam, grad_sample_index, synth_state_dict
from tests.train_loop_cases import (CLASS_WEIGHTS, IGNORE_IDX, LR, TOT_ITER, TRAIN_LOOP_CASES, WEIGHT_DECAY, WRITER_IDX0, loop_args,
                                    loop_batches)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
KEYS = json.load(open(os.path.join(GOLDEN, 'state_dict_keys.json')))
META = json.load(open(os.path.join(GOLDEN, 'train_loop.json')))


class Writer(object):
    def __init__(self):
        self.records = []

    def add_scalar(self, tag, value, idx):
        self.records.append([tag, float(value), int(idx)])


class Loader(object):
    """The seeded batches, device-resident; tells the spies when the loop is inside steps 2..K."""

    def __init__(self, batches, spy):
        self.batches, self.spy = batches, spy

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        for i, b in enumerate(self.batches):
            self.spy['inside'] = i >= 1
            yield b
        self.spy['inside'] = False


def _sample(model):
    flat = torch.cat([p.detach().reshape(-1)[grad_sample_index(p.numel()).to(DEV)] for p in model.parameters()])
    return flat.cpu().numpy()


def _run(name, epochs=None, restated=False):
    """The generator's schedule through script.train (bound the way install_dropin(script=..., train_loops=True) binds it).  Returns
    what the loop wrote and returned, the meters read per epoch, a parameter sample per epoch and what the spies counted."""
    from mspl_amd import losses, models, script, training
    case = TRAIN_LOOP_CASES[name]
    spy = {'inside': False, 'inside_calls': [], 'graph_built': 0, 'graph_calls': 0, 'eager_steps': 0, 'reads': [], 'visual': []}
    mp = pytest.MonkeyPatch()
    audit = StepAudit()          # every FlatAdam step of the run: device clones only while the spies count, host work after the loop
    try:
        def counted(owner, attr):
            orig = getattr(owner, attr)

            def wrapper(*a, **k):
                if spy['inside']:
                    spy['inside_calls'].append(attr)
                return orig(*a, **k)
            mp.setattr(owner, attr, wrapper)
        counted(torch.cuda, 'synchronize')
        counted(torch.Tensor, 'item')
        counted(torch.Tensor, 'cpu')
        g_init, g_call, t_step, m_read = (training.GraphedTrainStep.__init__, training.GraphedTrainStep.__call__, training.train_step,
                                          training.TrainMeters.read)

        def init(self, *a, **k):
            spy['graph_built'] += 1
            spy['building'] = True
            audit.tag = 'capture'          # the two steps the constructor takes on the batch that only shapes the capture
            try:
                g_init(self, *a, **k)
            finally:
                spy['building'] = False
                audit.tag = None

        def call(self, *a, **k):
            spy['graph_calls'] += 1
            return g_call(self, *a, **k)

        def step(*a, **k):
            if not spy.get('building'):
                spy['eager_steps'] += 1
            return t_step(*a, **k)

        def read(self):
            r = m_read(self)
            spy['reads'].append(r)
            return r
        mp.setattr(training.GraphedTrainStep, '__init__', init)
        mp.setattr(training.GraphedTrainStep, '__call__', call)
        mp.setattr(training, 'train_step', step)
        mp.setattr(training.TrainMeters, 'read', read)
        mp.setattr(script, '_FORCE_RESTATED', bool(restated))

        m = models.ESPDNetwithUncertaintyEstimation(argparse.Namespace(s=2.0, channels=3, num_classes=1000), classes=5,
                                                    dataset='greenhouse', fix_pyr_plane_proj=True)
        m.load_state_dict(synth_state_dict(KEYS['espdnetue_s2.0_c5'], case['sd_seed']))
        m = m.to(DEV).eval()
        cw = torch.tensor(CLASS_WEIGHTS)
        if case['use_uncertainty']:
            crit = losses.UncertaintyWeightedSegmentationLoss(5, class_weights=cw, ignore_idx=IGNORE_IDX, device=DEV)
        else:
            crit = losses.SegmentationLoss(n_classes=5, device=DEV, ignore_idx=IGNORE_IDX, class_weights=cw)
        loader = Loader([(x.to(DEV), y.to(DEV)) for x, y in loop_batches(case)], spy)
        ns = {'in_training_visualization_img': lambda model, **kw: spy['visual'].append(sorted(kw))}
        assert 'train' in script.patch_script(ns, train=True)
        args, writer, idx = loop_args(case), Writer(), WRITER_IDX0
        out = {'returned': [], 'params': [], 'optimizers': []}
        epoch = 0
        with audit:
            audit.watch(m)
            for n_epochs in case['phases']:
                opt = torch.optim.Adam(m.parameters(), lr=LR, weight_decay=WEIGHT_DECAY)
                out['optimizers'].append(opt)
                for _ in range(n_epochs):
                    if epochs is not None and epoch >= epochs:
                        break
                    idx = ns['train'](loader, m, crit, DEV, None, opt, TOT_ITER, 0, epoch, args, None, None, None, idx, None, writer, None)
                    out['returned'].append(int(idx))
                    out['params'].append(_sample(m))
                    epoch += 1
        out.update(records=writer.records, spy=spy, epochs=epoch, audit=_audit_summary(audit, m, name))
        return out
    finally:
        mp.undo()


def _audit_summary(audit, model, label):
    """Host side of the audit, after the loop: every recorded Adam step of every epoch and phase checked per tensor against float64
    (frozen BatchNorm buffers and the 230 gradient-less tensors bit-identical), then what the tests assert about the sequence --
    the device clones are dropped, the cached run keeps numbers only."""
    if not audit.records:
        return {'steps': [], 'fresh_moments_zero': [], 'first_step_from_entry_weights': None}
    audit.check(model, label='train loop ' + label)
    loop = [r for r in audit.records if r.tag is None]
    entry = audit._entry[id(model)]
    names = dict((id(p), n) for n, p in model.named_parameters())
    opt = loop[0].opt
    same = all(torch.equal(loop[0].pre[0][o:o + p.numel()].view(torch.int32), entry[names[id(p)]].reshape(-1).view(torch.int32))
               for o, p in zip(opt.bucket.offsets, opt.params))
    out = {'steps': [(r.tag, r.step, r.lrs[0]) for r in audit.records],
           'fresh_moments_zero': [not bool(r.pre[2].any()) and not bool(r.pre[3].any()) for r in audit.records if r.step == 1],
           'first_step_from_entry_weights': same, 'worst': dict(audit.worst)}
    audit.records = []
    return out


_RUNS = {}


def _cached(name):
    if name not in _RUNS:
        _RUNS[name] = _run(name)
    return _RUNS[name]


LOSS_RTOL, LOSS_ATOL = 2e-5, 1e-5          # the one-step bound of test_train_step_vs_reference_golden


def _check_against(case, golden_prefix, g, got, first_epochs=None, want_records=None, want_params=None):
    """Loss average and areas of `got` against the golden (or, with want_params, against another run of this project)."""
    for e in range(got['epochs'] if first_epochs is None else first_epochs):
        rec, r = got['records'][8 * e:8 * e + 8], got['spy']['reads'][e]
        ref = want_records[8 * e:8 * e + 8]
        dev = abs(rec[0][1] - ref[0][1])
        print('%s epoch %d: loss average %.9g against %.9g (relative deviation %.2e)' % (golden_prefix, e, rec[0][1], ref[0][1], dev / abs(ref[0][1])))
        assert dev <= LOSS_RTOL * abs(ref[0][1]) + LOSS_ATOL
        cap = 2 * int(g[golden_prefix + '.near'][e].sum())
        want_areas = g[golden_prefix + '.areas'][e].sum(0) if want_params is None else want_params['areas'][e]
        l1 = np.abs(r['areas'] - want_areas).sum(1)
        print('    areas L1 per histogram', l1.tolist(), 'allowed', cap)
        assert (l1 <= cap).all()


@pytest.mark.parametrize('name', sorted(TRAIN_LOOP_CASES))
def test_train_loop_against_the_reference_loop(name, golden):
    """What the loop writes and returns, the meters per epoch and a sample of EVERY parameter after each optimizer's last step.

    Loss average: within the one-step bound of test_train_step_vs_reference_golden (rtol 2e-5, atol 1e-5).  Areas: per epoch and
    histogram an L1 distance of at most 2 * (the pixels whose top-2 margin of the reference's main head is below 1e-3), a number the
    fixture caps at 2 % of the pixels.  Parameters: assert_weights_close_after_adam over the steps applied so far -- a doubled first
    step or a lost partial batch moves far more than one per cent of the elements.  Moments or a step count kept across a fresh
    optimizer do NOT (Adam's next step is +-lr either way): those are caught by the step audit installed in `_run`
    (tests/optim_shadow.py), which checks every Adam step of the loop per tensor against float64 at the step's own inputs and
    whose recorded sequence is asserted below -- counts restarting at 1 on zero moments with each fresh optimizer, the poly
    learning rate of every iteration, and a first step that starts from the entry weights (the capture batch leaves no trace)."""
    case, g, meta, got = TRAIN_LOOP_CASES[name], golden('train_loop'), META[name], _cached(name)
    steps, epochs = len(case['batches']), sum(case['phases'])
    ref = meta['records']
    assert got['epochs'] == epochs and got['returned'] == meta['returned']
    assert [r[0] for r in got['records']] == [r[0] for r in ref] and [r[2] for r in got['records']] == [r[2] for r in ref]
    for e in range(epochs):
        rec, r = got['records'][8 * e:8 * e + 8], got['spy']['reads'][e]
        assert abs(rec[7][1] - ref[8 * e + 7][1]) <= 1e-12                    # learning rate after the last step
        assert rec[1][1] == 0.0 and r['steps'] == steps
        # the written IoU scalars are the reference's formulas on the adapter's own areas
        a = r['areas']
        iou = a[0] / (a[1] + a[2] - a[0] + steps * 1e-6 + 1e-10)
        want = [iou.mean() * 100 if case['use_traversable'] else iou[[1, 2, 3]].mean() * 100] + list(iou)
        np.testing.assert_allclose([x[1] for x in rec[2:7]], want, rtol=1e-6)
    _check_against(case, name, g, got, want_records=ref)
    done, e = 0, 0
    for p, n_epochs in enumerate(case['phases']):
        e += n_epochs
        done += n_epochs * steps
        assert_weights_close_after_adam(got['params'][e - 1], g[name + '.params_%d' % p], LR, done)
    assert got['spy']['visual'] == [['class_encoding', 'data', 'device', 'epoch', 'images', 'labels', 'writer']] * epochs
    assert len(got['spy']['reads']) == epochs
    audited = got['audit']
    if case['use_uncertainty']:          # the graphed path: FlatAdam steps (the restated body steps the caller's torch.optim.Adam)
        from mspl_amd.training import lr_poly
        lrs = [lr_poly(LR, i, TOT_ITER, case['power']) for i in range(steps)]
        want = [('capture', 1, lrs[0]), ('capture', 2, lrs[0])]
        for n_epochs in case['phases']:
            want += [(None, e_ * steps + i + 1, lrs[i]) for e_ in range(n_epochs) for i in range(steps)]
        assert audited['steps'] == want
        assert audited['fresh_moments_zero'] == [True] * (1 + len(case['phases']))
        assert audited['first_step_from_entry_weights'] is True
    else:
        assert audited['steps'] == []


@pytest.mark.parametrize('name', ['loop_32x48', 'loop_64x96_tail'])
def test_fast_path_runs_on_one_graphed_step_without_host_sync(name):
    """The shipped settings run on training.GraphedTrainStep: built once per model and reused in the second epoch and with the fresh
    optimizer; the partial batch takes training.train_step; nothing inside steps 2..K calls torch.cuda.synchronize, Tensor.item or
    Tensor.cpu, and the meters are read once per epoch.  The caller's Adam never stepped."""
    case, got = TRAIN_LOOP_CASES[name], _cached(name)
    spy, epochs = got['spy'], sum(case['phases'])
    full = sum(1 for b in case['batches'] if b == case['batches'][0])
    assert spy['graph_built'] == 1
    assert spy['graph_calls'] == full * epochs and spy['eager_steps'] == (len(case['batches']) - full) * epochs
    assert spy['inside_calls'] == []
    assert len(spy['reads']) == epochs
    assert all(len(o.state) == 0 for o in got['optimizers'])


def test_restated_body_is_taken_when_the_settings_ask_for_it():
    got = _cached('loop_ce_32x48')
    assert got['spy']['graph_built'] == 0 and got['spy']['graph_calls'] == 0
    assert all(len(o.state) > 0 for o in got['optimizers'])                   # the caller's own optimizer stepped


def test_fast_path_against_restated_body(golden):
    """loop_32x48's first epoch through the graphed step and through the restated reference body (forced by the internal switch):
    the same loss-average, areas and parameter bounds as against the golden."""
    name = 'loop_32x48'
    case, g = TRAIN_LOOP_CASES[name], golden('train_loop')
    fast, slow = _cached(name), _run(name, epochs=1, restated=True)
    assert slow['spy']['graph_built'] == 0 and len(slow['optimizers'][0].state) > 0
    _check_against(case, name, g, fast, first_epochs=1, want_records=slow['records'],
                   want_params={'areas': [r['areas'] for r in slow['spy']['reads']]})
    assert_weights_close_after_adam(fast['params'][0], slow['params'][0], LR, len(case['batches']))


def test_deeplabv3_is_refused():
    from mspl_amd import script
    args = argparse.Namespace(model='deeplabv3', use_depth=False, use_uncertainty=True, use_traversable=False, learning_rate=LR, power=0.0)
    m = torch.nn.Conv2d(3, 5, 1).to(DEV).eval()
    with pytest.raises(RuntimeError, match='deeplabv3'):
        script.train([], m, None, DEV, None, torch.optim.Adam(m.parameters()), TOT_ITER, 0, 0, args, None, None, None, 0, None, Writer(), None)
