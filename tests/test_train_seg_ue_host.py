"""CPU-side checks of the drop-in train_seg_ue() loop: its signature against the one recorded from the reference, its opt-in binding,
the decisions of the fast-path predicate on host-side stand-ins, and the committed fixture's own conditions.  No kernel is launched."""
import argparse
import inspect
import json
import os
import sys

import numpy as np
import pytest
import torch

from mspl_amd import script
from tests.conftest import GOLDEN
from tests.supervised_loop_cases import NEAR_CAP, NUM_CLASSES, PARAM_FLOOR, SUPERVISED_LOOP_CASES, group_of

META = json.load(open(os.path.join(GOLDEN, 'train_seg_ue_loop.json')))


def test_train_seg_ue_has_the_reference_signature():
    sig = inspect.signature(script.train_seg_ue)
    assert list(sig.parameters) == META['signature']['names']
    defaults = {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
    assert defaults == META['signature']['defaults']
    assert all(p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for p in sig.parameters.values())


def _purge():
    for n in [k for k in sys.modules if k.split('.')[0] in ('nn_layers', 'model', 'loss_fns', 'data_loader', 'utilities', 'transforms',
                                                             '_mspl_reference')]:
        del sys.modules[n]


def test_binding_is_opt_in():
    import mspl_amd
    from mspl_amd import evaluation
    _purge()
    try:
        mspl_amd.install_dropin()
        alias = sys.modules['utilities.train_eval_seg']
        assert alias.__dict__['val_seg_ue'] is evaluation.val_seg_ue and 'train_seg_ue' not in alias.__dict__
        _purge()
        ns = {}
        mspl_amd.install_dropin(train_loops=True)          # independent of `script=`
        from utilities.train_eval_seg import train_seg_ue, val_seg_ue
        assert train_seg_ue is script.train_seg_ue and val_seg_ue is evaluation.val_seg_ue and ns == {}
        _purge()
        ns = {}
        mspl_amd.install_dropin(script=ns)                  # the script-level functions alone do not bind it
        assert 'train_seg_ue' not in sys.modules['utilities.train_eval_seg'].__dict__ and 'generate_pseudo_label' in ns
    finally:
        _purge()


@pytest.fixture(scope='module')
def standins():
    from mspl_amd import losses, models
    m = models.ESPDNetwithUncertaintyEstimation(argparse.Namespace(s=2.0, channels=3, num_classes=1000), classes=5, dataset='greenhouse',
                                                fix_pyr_plane_proj=True)
    crit = losses.SegmentationLoss(n_classes=5, device='cpu', ignore_idx=4, class_weights=torch.ones(5))
    ps = [torch.nn.Parameter(torch.zeros(3)) for _ in range(4)]

    def sgd(groups=2, **kw):
        return torch.optim.SGD([{'params': [p]} for p in ps[:groups]], 0.01, momentum=kw.pop('momentum', 0.9), **kw)
    return m, crit, sgd, ps


def test_fast_path_predicate(standins, monkeypatch):
    from mspl_amd import losses
    m, crit, sgd, ps = standins
    fast = script._supervised_fast_path
    for dev in ('cuda', 'cuda:0', torch.device('cuda')):
        assert fast(m, crit, sgd(2), None, dev) and fast(m, crit, sgd(3), None, dev)
    assert fast(m, crit, sgd(2, momentum=0.0, weight_decay=4e-5), None, 'cuda')
    assert not fast(m, crit, sgd(2), None, 'cpu')
    assert not fast(m, crit, sgd(2), losses.NIDLoss(), 'cuda')                       # an additional criterion
    assert not fast(m, crit, sgd(2), None, 'cuda', use_depth=True)
    assert not fast(m, crit, sgd(1), None, 'cuda') and not fast(m, crit, sgd(4), None, 'cuda')
    assert not fast(m, crit, sgd(2, nesterov=True), None, 'cuda')
    assert not fast(m, crit, sgd(2, dampening=0.1), None, 'cuda')
    assert not fast(m, crit, sgd(2, maximize=True), None, 'cuda')
    assert not fast(m, crit, torch.optim.Adam([{'params': [ps[0]]}, {'params': [ps[1]]}]), None, 'cuda')

    class MySGD(torch.optim.SGD):
        pass
    assert not fast(m, crit, MySGD([{'params': [ps[0]]}, {'params': [ps[1]]}], 0.01, momentum=0.9), None, 'cuda')
    assert not fast(m, losses.UncertaintyWeightedSegmentationLoss(5, device='cpu'), sgd(2), None, 'cuda')

    class MyLoss(losses.SegmentationLoss):
        pass
    assert not fast(m, MyLoss(n_classes=5, device='cpu'), sgd(2), None, 'cuda')
    assert not fast(torch.nn.Conv2d(3, 5, 1), crit, sgd(2), None, 'cuda')
    monkeypatch.setattr(script, '_FORCE_RESTATED', True)
    assert not fast(m, crit, sgd(2), None, 'cuda')


def test_fixture_satisfies_its_conditions():
    g = dict(np.load(os.path.join(GOLDEN, 'train_seg_ue_loop.npz'), allow_pickle=False))
    assert sorted(META['cases']) == sorted(SUPERVISED_LOOP_CASES)
    K = NUM_CLASSES - 1
    groups = [group_of(n) for n in META['names']]
    assert groups.count(0) > 100 and groups.count(1) > 50
    for name, case in SUPERVISED_LOOP_CASES.items():
        epochs, steps = sum(case['phases']), len(case['batches'])
        pixels = sum(case['batches']) * case['hw'][0] * case['hw'][1]
        assert len(case['lrs']) == epochs
        assert g[name + '.areas'].shape == (epochs, steps, 3, K) and g[name + '.loss'].shape == (epochs, steps)
        near = g[name + '.near']
        assert near.shape == (epochs, steps) and near.sum(axis=1).max() <= NEAR_CAP * pixels
        assert (g[name + '.area_gap'] <= 2 * near.sum(axis=1)[:, None]).all()
        w = np.asarray(case['batches'], dtype=np.float64)
        for e in range(epochs):
            # the returned values are the reference's formulas on the stored areas and losses (float32 sums there, integers here)
            a = g[name + '.areas'][e].sum(0).astype(np.float64)
            np.testing.assert_allclose(g[name + '.iou'][e], a[0] / (a[1] + a[2] - a[0] + steps * 1e-6 + 1e-10), rtol=1e-5)
            np.testing.assert_allclose(g[name + '.loss_avg'][e], (g[name + '.loss'][e] * w).sum() / w.sum(), rtol=1e-12)
        assert len(g[name + '.params_off']) == len(META['names']) + 1
        for p in range(len(case['phases'])):
            assert g[name + '.params_%d' % p].shape == (g[name + '.params_off'][-1],)
            assert g[name + '.params_gap_%d' % p].shape == (len(META['names']),)
            assert g[name + '.buffers_%d' % p].shape == (g[name + '.buffers_off'][-1],)
        if case['nid'] is not None:
            assert g[name + '.params_gap_0'].max() <= PARAM_FLOOR          # the conditioning rule of the NID case


def test_flat_sgd_partition_and_reattach():
    """FlatSGD.same_partition / reattach / reset on CPU tensors (no kernel runs)."""
    from mspl_amd.supervised import FlatSGD
    ps = [torch.nn.Parameter(torch.randn(n)) for n in (3, 5, 2, 7)]
    for p in ps[:3]:
        p.grad = torch.ones_like(p)                       # the fourth has no gradient: left out, as torch.optim skips it
    groups = [{'params': ps[:2], 'lr': 0.1}, {'params': ps[2:], 'lr': 1.0}]
    opt = FlatSGD(groups, lr=0.1, momentum=0.9, weight_decay=4e-5)
    assert [len(g['params']) for g in opt.param_groups] == [2, 1]
    assert opt.same_partition(groups) and opt.same_partition([{'params': ps[:2]}, {'params': ps[2:]}])
    assert not opt.same_partition([{'params': ps[2:]}, {'params': ps[:2]}])
    assert not opt.same_partition([{'params': ps}]) and not opt.same_partition([{'params': ps[:1]}, {'params': ps[1:]}])
    ps[0].grad = None
    ps[1].grad = torch.zeros(5)
    opt.reattach()
    b = opt.bucket
    assert all(p.grad.data_ptr() == b.flat.data_ptr() + 4 * off for p, off in zip(b.params, b.offsets))
    opt.buf.fill_(1.0)
    opt.step_count = 3
    opt.reset([{'lr': 0.5, 'momentum': 0.8, 'weight_decay': 0.0, 'params': []}, {'lr': 5.0, 'params': []}])
    assert not opt.buf.any() and opt.step_count == 0
    assert [(g['lr'], g['momentum'], g['weight_decay']) for g in opt.param_groups] == [(0.5, 0.8, 0.0), (5.0, 0.9, 4e-5)]
    with pytest.raises(ValueError):
        opt.reset([{'lr': 1.0}])
    ps[1].data = torch.zeros(5)
    with pytest.raises(RuntimeError, match='flat parameter buffer'):
        opt.reattach()
