"""CPU-side checks of the drop-in single-head loops train_seg() / val_seg(): their signatures against the text recorded from the
reference, the opt-in binding, the decisions of the fast-path predicate on host-side stand-ins, the scalar miou with its IndexError,
and val_seg's host logic through an EvalSums stand-in.  No kernel is launched."""
import argparse
import inspect
import json
import os
import sys

import numpy as np
import pytest
import torch

from mspl_amd import evaluation, script
from tests.conftest import GOLDEN
from tests.single_head_loop_cases import NID_GAP_CAP, SINGLE_HEAD_LOOP_CASES

META = json.load(open(os.path.join(GOLDEN, 'train_seg_loop.json')))


@pytest.mark.parametrize('name', ['train_seg', 'val_seg'])
def test_the_loops_have_the_reference_signatures(name):
    fn = script.train_seg if name == 'train_seg' else evaluation.val_seg
    rec = META['signatures'][name]
    sig = inspect.signature(fn)
    n = len(rec['names'])
    # the reference's parameters, in its order, with its defaults; val_seg's own extras (sharding, lanes) come after them, keyword-able
    assert list(sig.parameters)[:n] == rec['names']
    defaults = {k: p.default for k, p in list(sig.parameters.items())[:n] if p.default is not inspect.Parameter.empty}
    assert defaults == rec['defaults']
    head = inspect.Signature(list(sig.parameters.values())[:n])
    assert str(head) == rec['text']
    if name == 'train_seg':
        assert len(sig.parameters) == n
        # the order of the last two arguments is NOT train_seg_ue's
        assert rec['names'][-2:] == ['greenhouse_use_trav', 'weight']
        assert list(inspect.signature(script.train_seg_ue).parameters)[-2:] == ['weight', 'greenhouse_use_trav']
    else:
        assert all(p.default is not inspect.Parameter.empty for p in list(sig.parameters.values())[n:])


def _purge():
    for n in [k for k in sys.modules if k.split('.')[0] in ('nn_layers', 'model', 'loss_fns', 'data_loader', 'utilities', 'transforms',
                                                             '_mspl_reference')]:
        del sys.modules[n]


def test_binding_is_opt_in():
    import mspl_amd
    _purge()
    try:
        mspl_amd.install_dropin()
        alias = sys.modules['utilities.train_eval_seg'].__dict__
        assert alias['val_seg_ue'] is evaluation.val_seg_ue
        assert not any(k in alias for k in ('train_seg', 'val_seg', 'train_seg_ue'))
        _purge()
        mspl_amd.install_dropin(train_loops=True)
        from utilities.train_eval_seg import train_seg, train_seg_ue, val_seg, val_seg_ue
        assert train_seg is script.train_seg and val_seg is evaluation.val_seg
        assert train_seg_ue is script.train_seg_ue and val_seg_ue is evaluation.val_seg_ue
    finally:
        _purge()


@pytest.fixture(scope='module')
def standins():
    from mspl_amd import losses, models
    a = argparse.Namespace(s=0.5, channels=3, num_classes=1000)
    v2 = models.ESPNetv2Segmentation(a, classes=5, dataset='greenhouse')
    esp = models.ESPDNetSegmentation(argparse.Namespace(s=2.0, channels=3, num_classes=1000), classes=5, dataset='greenhouse')
    ue = models.ESPDNetwithUncertaintyEstimation(argparse.Namespace(s=2.0, channels=3, num_classes=1000), classes=5, dataset='greenhouse',
                                                 fix_pyr_plane_proj=True)
    crit = losses.SegmentationLoss(n_classes=5, device='cpu', ignore_idx=4, class_weights=torch.ones(5))
    ps = [torch.nn.Parameter(torch.zeros(3)) for _ in range(4)]

    def sgd(groups=2, **kw):
        return torch.optim.SGD([{'params': [p]} for p in ps[:groups]], 0.01, momentum=kw.pop('momentum', 0.9), **kw)
    return v2, esp, ue, crit, sgd, ps


def test_fast_path_predicate(standins, monkeypatch):
    from mspl_amd import losses
    v2, esp, ue, crit, sgd, ps = standins
    fast = script._single_head_fast_path
    for m in (v2, esp):
        for dev in ('cuda', 'cuda:0', torch.device('cuda')):
            assert fast(m, crit, sgd(2), None, dev) and fast(m, crit, sgd(3), None, dev)
        assert fast(m, crit, sgd(2, momentum=0.0, weight_decay=4e-5), None, 'cuda')
        assert not fast(m, crit, sgd(2), None, 'cpu')
        assert not fast(m, crit, sgd(2), losses.NIDLoss(), 'cuda')                       # an additional criterion
        assert not fast(m, crit, sgd(2), None, 'cuda', use_depth=True)                   # an RGB-D batch
        assert not fast(m, crit, sgd(1), None, 'cuda') and not fast(m, crit, sgd(4), None, 'cuda')
        assert not fast(m, crit, sgd(2, nesterov=True), None, 'cuda')
        assert not fast(m, crit, sgd(2, dampening=0.1), None, 'cuda')
        assert not fast(m, crit, sgd(2, maximize=True), None, 'cuda')
        assert not fast(m, crit, torch.optim.Adam([{'params': [ps[0]]}, {'params': [ps[1]]}]), None, 'cuda')
        assert not fast(m, losses.UncertaintyWeightedSegmentationLoss(5, device='cpu'), sgd(2), None, 'cuda')
    # the two-head model belongs to train_seg_ue, and the other way round
    assert not fast(ue, crit, sgd(2), None, 'cuda')
    assert not script._supervised_fast_path(v2, crit, sgd(2), None, 'cuda') and not script._supervised_fast_path(esp, crit, sgd(2), None, 'cuda')
    assert script._supervised_fast_path(ue, crit, sgd(2), None, 'cuda')

    class MyLoss(losses.SegmentationLoss):
        pass
    assert not fast(v2, MyLoss(n_classes=5, device='cpu'), sgd(2), None, 'cuda')
    assert not fast(torch.nn.Conv2d(3, 5, 1), crit, sgd(2), None, 'cuda')
    monkeypatch.setattr(script, '_FORCE_RESTATED', True)
    assert not fast(v2, crit, sgd(2), None, 'cuda')


class _Sums(evaluation.EvalSums):
    """EvalPass's call signature over precomputed per-batch sums: (areas (3,K), loss, images)."""

    def __init__(self, K, batches):
        self.K, self.batches_in, self.seen = K, batches, []

    def __call__(self, images, labels, depth=None):
        self.seen.append((images, labels, depth))

    def sums(self):
        K = self.K
        a = sum(b[0] for b in self.batches_in[:len(self.seen)])
        loss = sum(b[1] * b[2] for b in self.batches_in[:len(self.seen)])
        n = sum(b[2] for b in self.batches_in[:len(self.seen)])
        return torch.tensor(list(a.reshape(-1)) + [loss, n, float(len(self.seen))], dtype=torch.float64)


def _areas(K, seed):
    rng = np.random.RandomState(seed)
    inter = rng.randint(10, 100, K)
    return np.stack([inter, inter + rng.randint(0, 50, K), inter + rng.randint(0, 50, K)]).astype(np.float64)


def test_val_seg_returns_the_scalar_miou_through_a_standin():
    K = 4
    batches = [(_areas(K, 1), 0.75, 4), (_areas(K, 2), 1.25, 2)]
    loader = [('x0', 'y0', 'd0'), ('x1', 'y1', 'd1')]
    a = batches[0][0] + batches[1][0]
    iou = a[0] / (a[1] + a[2] - a[0] + 2 * 1e-6 + 1e-10)
    crit = argparse.Namespace(loss_type='ce', class_wts=None, ignore_idx=4)
    ep = _Sums(K, batches)
    miou, loss = evaluation.val_seg(None, loader, criterion=crit, num_classes=K + 1, _eval_pass=ep)
    assert np.ndim(miou) == 0 and abs(miou - iou[[1, 2, 3]].mean() * 100) <= 1e-9
    assert abs(loss - (0.75 * 4 + 1.25 * 2) / 6) <= 1e-12
    assert [s[2] for s in ep.seen] == [None, None]                                  # no depth batch unless use_depth
    ep = _Sums(K, batches)
    miou_t, loss0 = evaluation.val_seg(None, loader, criterion=None, num_classes=K + 1, use_depth=True, greenhouse_use_trav=True, _eval_pass=ep)
    assert abs(miou_t - iou.mean() * 100) <= 1e-9 and loss0 == 0
    assert [s[2] for s in ep.seen] == ['d0', 'd1']
    # fewer than four MIOU classes without greenhouse_use_trav: the reference's IndexError (iou[[1, 2, 3]])
    small = [(_areas(3, 3), 1.0, 4)]
    with pytest.raises(IndexError):
        evaluation.val_seg(None, loader[:1], criterion=crit, num_classes=4, _eval_pass=_Sums(3, small))
    m3, _ = evaluation.val_seg(None, loader[:1], criterion=crit, num_classes=4, greenhouse_use_trav=True, _eval_pass=_Sums(3, small))
    assert np.isfinite(m3)
    with pytest.raises(NotImplementedError):
        evaluation.val_seg(None, loader, criterion=argparse.Namespace(loss_type='bce'), num_classes=5, _eval_pass=_Sums(K, batches))


def test_miou_percent_is_the_loops_summary():
    iou = np.array([0.5, 0.25, 0.75, 1.0])
    assert evaluation.miou_percent(iou) == pytest.approx((0.25 + 0.75 + 1.0) / 3 * 100)
    assert evaluation.miou_percent(iou, True) == pytest.approx(iou.mean() * 100)
    with pytest.raises(IndexError):
        evaluation.miou_percent(iou[:3])


def test_fixture_satisfies_its_conditions():
    from tests.supervised_loop_cases import NEAR_CAP, NUM_CLASSES, group_of
    g = dict(np.load(os.path.join(GOLDEN, 'train_seg_loop.npz'), allow_pickle=False))
    assert sorted(META['cases']) == sorted(SINGLE_HEAD_LOOP_CASES)
    K = NUM_CLASSES - 1
    for name, case in SINGLE_HEAD_LOOP_CASES.items():
        names = META['cases'][name]['names']
        groups = [group_of(n) for n in names]
        assert groups.count(0) > 100 and groups.count(1) > 50
        epochs, steps = sum(case['phases']), len(case['batches'])
        pixels = sum(case['batches']) * case['hw'][0] * case['hw'][1]
        assert g[name + '.areas'].shape == (epochs, steps, 3, K) and g[name + '.loss'].shape == (epochs, steps)
        near = g[name + '.near']
        assert near.shape == (epochs, steps) and near.sum(axis=1).max() <= NEAR_CAP * pixels
        assert (g[name + '.area_gap'] <= 2 * near.sum(axis=1)[:, None]).all()
        w = np.asarray(case['batches'], dtype=np.float64)
        for e in range(epochs):
            # the returned values are the reference's formulas on the stored areas and losses (float32 sums there, integers here)
            a = g[name + '.areas'][e].sum(0).astype(np.float64)
            iou = a[0] / (a[1] + a[2] - a[0] + steps * 1e-6 + 1e-10)
            np.testing.assert_allclose(g[name + '.miou'][e], iou[[1, 2, 3]].mean() * 100, rtol=1e-5)
            np.testing.assert_allclose(g[name + '.loss_avg'][e], (g[name + '.loss'][e] * w).sum() / w.sum(), rtol=1e-12)
        va = g[name + '.val_areas'].astype(np.float64)
        viou = va[0] / (va[1] + va[2] - va[0] + 2 * 1e-6 + 1e-10)
        np.testing.assert_allclose(g[name + '.val'][0], viou[[1, 2, 3]].mean() * 100, rtol=1e-5)
        assert len(g[name + '.params_off']) == len(names) + 1
        if case['nid'] is not None:
            assert g[name + '.params_gap_0'].max() <= NID_GAP_CAP          # the conditioning rule of the NID case
