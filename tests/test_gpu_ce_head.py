"""mspl_ce_head_meters_fwd_bwd (mspl_amd/csrc/ce_head.hip) and autograd.ce_head_meters: the cross-entropy sums, the MIOU areas and the
logit gradient of train_seg (utilities/train_eval_seg.py:44-58) from the decoder's low-resolution head, in one launch.

Reference: float64 on the CPU -- F.interpolate(mode='bilinear', align_corners=True) of the head in double, F.cross_entropy(weight,
ignore_index); the gradient with respect to the LOW-RESOLUTION head from autograd in double (the kernel's label-resolution gradient
goes through mspl_bilinear_bwd and the 1 / sums[1] factor first, as the node does).  Areas: tests.train_loop_cases.reference_areas
on the float64 argmax, whose intersection and union are also held against oracle.labels.miou_areas.

Bounds (tests/test_gpu_supervised_grad_parity.py): loss 5e-6 relative, gradient 2e-4 relative norm / 2.5e-4 of the largest element,
sums[1] 1e-12 relative (a double sum of float32 weights).  Areas: the kernel interpolates in float32, so a pixel whose float64
top-two margin is below 1e-4 may turn; each such pixel moves at most two counts of a histogram, hence L1 <= 2 x their number, and
the CPU asserts that they are at most 0.2 % of a case's pixels (seeds C * 100 + H: at most 0.048 % over the cases of this file).

Trained-logit magnitudes (tests/confident_cases.py, `(randn + onehot) * magnitude`): loss and gradient within MARGIN = 4 units, a unit
being the float32 restatement's own error on the case (the same torch-CPU computation in float32 against float64) floored at 2**-22
-- the rule of tests/test_gpu_confident_logits.py.  Each test prints what it measured."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import labels as olab
from tests import confident_cases as cc
from tests.train_loop_cases import reference_areas

pytestmark = pytest.mark.gpu
DEV = 'cuda'
LOSS_TAU, GRAD_TAU_REL, GRAD_TAU_EL = cc.LOSS_TAU, cc.GRAD_TAU_REL, cc.GRAD_TAU_EL
DEN_RTOL = 1e-12
NEAR_MARGIN, NEAR_CAP = 1e-4, 0.002
FLOOR = 2.0 ** -22
# (head, labels): two column tiles with a ragged 16-column one, several bands, the image stride | not an exact x2, a last band shorter
# than the band height | rows kept
SHAPES = [((20, 136), (40, 272)), ((9, 17), (20, 40)), ((12, 130), (12, 260))]
CLASSES = (1, 3, 5, 7, 13, 20)
KINDS = ('weighted', 'outside', 'void_image')


def _lib():
    from mspl_amd._native import check, lib
    from mspl_amd.ops import _p, _stream
    return check, lib, _p, _stream


def _reference(head, target, cw, ignore, size, K, dtype=torch.float64):
    """{'loss', 'num', 'den', 'ghead', 'areas' (3,K), 'near'} of the case in `dtype` on the CPU."""
    C = head.shape[1]
    h = head.detach().to(dtype).clone().requires_grad_()
    up = F.interpolate(h, size=size, mode='bilinear', align_corners=True)
    tt = torch.where((target < 0) | (target >= C), torch.full_like(target, ignore), target)
    w = torch.ones(C, dtype=dtype) if cw is None else cw.to(dtype)
    num = F.cross_entropy(up, tt, weight=w, ignore_index=ignore, reduction='sum')
    den = w[tt[tt != ignore]].sum()
    loss = num / den
    loss.backward()
    up = up.detach()
    if C > 1:
        top = torch.sort(up, dim=1, descending=True)[0]
        near = int(((top[:, 0] - top[:, 1]) < NEAR_MARGIN).sum())
    else:
        near = 0
    areas = reference_areas(up.argmax(1).numpy(), target.numpy(), K)
    return {'loss': float(loss.detach()), 'num': float(num.detach()), 'den': float(den), 'ghead': h.grad, 'areas': areas, 'near': near,
            'up': up}


@functools.lru_cache(maxsize=None)
def _case(C, shape_idx, kind='plain'):
    """Inputs and the float64 reference of one case; computed once, shared, never modified.
    plain: labels of every class and 10 % of 255 = ignore_index, no class weights, K = C - 1 (1 at C = 1)
    weighted: ignore_index = C - 1, class weights linspace(0.5, 2, C)
    outside: 15 % of the labels in C..254 -- invalid for the loss, counted by the uint8 rule for the areas (K = C + 2 bins)
    void_image: image 0 ignored entirely"""
    hs, size = SHAPES[shape_idx]
    N = 2
    g = torch.Generator().manual_seed(C * 100 + size[0])
    head = torch.randn((N, C) + hs, generator=g) * 3
    target = torch.randint(0, C, (N,) + size, generator=g)
    target[torch.rand((N,) + size, generator=g) < 0.1] = 255
    ignore, cw, K = 255, None, max(C - 1, 1)
    if kind == 'weighted':
        ignore, cw = C - 1, torch.linspace(0.5, 2, C)
    elif kind == 'outside':
        out = torch.rand((N,) + size, generator=g) < 0.15
        target[out] = torch.randint(C, 255, (N,) + size, generator=g)[out]
        K = C + 2
    elif kind == 'void_image':
        target[0] = 255
    ref = _reference(head, target, cw, ignore, size, K)
    # the reference against the oracle's own MIOU (intersection and union of the same argmax; torch.histc widens a one-bin range)
    if K > 1:
        inter, union = olab.miou_areas(ref['up'], target, K)
        a = ref['areas']
        assert np.array_equal(inter.astype(np.int64), a[0]) and np.allclose(union, a[1] + a[2] - a[0] + 1e-6, rtol=0, atol=1e-3)
    # a condition on the case, not a measurement
    assert ref['near'] <= NEAR_CAP * target.numel(), 'case C=%d %s: %d near-margin pixels' % (C, size, ref['near'])
    return {'head': head, 'target': target, 'cw': cw, 'ignore': ignore, 'size': size, 'K': K, 'ref': ref, 'N': N, 'C': C}


def _launch(head, target, cw, ignore, size, K, grad=True, areas=True):
    """(sums float64[2], areas int64[3K] or None, gfull or None, ghead or None) through the C ABI, the way the node composes it."""
    check, lib, _p, _stream = _lib()
    N, C, Hm, Wm = head.shape
    H, W = size
    hd, td = head.to(DEV), target.to(DEV)
    cwd = None if cw is None else cw.to(DEV)
    assert lib.mspl_ce_head_supported(C) == 1 and lib.mspl_ce_head_fits(N, C, Hm, Wm, H, W) == 1
    sums = torch.zeros(2, dtype=torch.float64, device=DEV)
    ar = torch.zeros(3 * K, dtype=torch.int64, device=DEV) if areas else None
    gfull = torch.full((N, C, H, W), float('nan'), device=DEV) if grad else None         # (the launch overwrites every element)
    check(lib.mspl_ce_head_meters_fwd_bwd(_p(hd), _p(td), _p(cwd), int(ignore), N, C, Hm, Wm, H, W, K, _p(sums), _p(ar), _p(gfull),
                                          _stream()))
    ghead = None
    if grad:
        ghead = torch.empty_like(hd)
        check(lib.mspl_bilinear_bwd(_p(gfull), N, C, Hm, Wm, H, W, _p(ghead), _stream()))
        ghead = ghead * (1.0 / sums[1]).float()
    return sums, ar, gfull, ghead


def _check(tag, c, sums, areas, ghead):
    ref = c['ref']
    s = sums.cpu().numpy()
    loss = s[0] / s[1]
    lerr = cc.loss_error(loss, ref['loss'])
    derr = abs(s[1] - ref['den']) / ref['den']
    print('%s: loss %.12g against %.12g (%.2e); den %.15g against %.15g' % (tag, loss, ref['loss'], lerr, s[1], ref['den']))
    assert lerr <= LOSS_TAU and derr <= DEN_RTOL
    if ghead is not None:
        assert torch.isfinite(ghead).all()
        e = cc.grad_errors(ghead, ref['ghead'])
        print('%s: head gradient rel %.2e element %.2e' % (tag, e[0], e[1]))
        assert e[0] <= GRAD_TAU_REL and e[1] <= GRAD_TAU_EL
    if areas is not None:
        got = areas.cpu().numpy().reshape(3, c['K'])
        l1 = np.abs(got - ref['areas']).sum(1)
        print('%s: %d near-margin pixels of %d, area L1 differences %s' % (tag, ref['near'], c['target'].numel(), l1.tolist()))
        assert int(l1.max()) <= 2 * ref['near']


@pytest.mark.parametrize('shape_idx', range(len(SHAPES)))
@pytest.mark.parametrize('C', CLASSES)
def test_sums_areas_and_gradient(C, shape_idx):
    c = _case(C, shape_idx)
    sums, areas, gfull, ghead = _launch(c['head'], c['target'], c['cw'], c['ignore'], c['size'], c['K'])
    assert torch.isfinite(gfull).all()
    # invalid pixels get zeros, in every class plane
    invalid = ((c['target'] == c['ignore']) | (c['target'] >= C)).to(DEV)
    assert float(gfull.abs().amax(1)[invalid].max()) == 0.0
    _check('C=%d %s->%s' % (C, SHAPES[shape_idx][0], c['size']), c, sums, areas, ghead)
    # forward only: the same sums and areas, nothing else written
    s2, a2, _, _ = _launch(c['head'], c['target'], c['cw'], c['ignore'], c['size'], c['K'], grad=False)
    assert torch.equal(a2, areas)
    assert torch.allclose(s2, sums, rtol=1e-12, atol=0)
    # without histograms
    s3 = _launch(c['head'], c['target'], c['cw'], c['ignore'], c['size'], c['K'], grad=False, areas=False)[0]
    assert torch.allclose(s3, sums, rtol=1e-12, atol=0)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('C', (3, 5, 13, 20))
def test_label_rules(C, kind):
    c = _case(C, 0, kind)
    sums, areas, gfull, ghead = _launch(c['head'], c['target'], c['cw'], c['ignore'], c['size'], c['K'])
    _check('C=%d %s' % (C, kind), c, sums, areas, ghead)
    invalid = ((c['target'] == c['ignore']) | (c['target'] >= C)).to(DEV)
    assert float(gfull.abs().amax(1)[invalid].max()) == 0.0
    if kind == 'void_image':
        assert float(gfull[0].abs().max()) == 0.0 and float(ghead[0].abs().max()) == 0.0
        assert float(c['ref']['ghead'][0].abs().max()) == 0.0
    if kind == 'outside':
        assert int(c['ref']['areas'][2, C:].sum()) > 0          # labels C and C + 1 are counted in the mask histogram


@pytest.mark.parametrize('C', (5, 20))
@pytest.mark.parametrize('kind', ('plain', 'weighted'))
def test_node_meets_the_reference(C, kind):
    """autograd.ce_head_meters: loss, gradient of the head, meters; forward only under no_grad."""
    from mspl_amd import autograd as ag
    from mspl_amd.supervised import SupervisedMeters
    c = _case(C, 1, kind)
    ref = c['ref']
    meters = SupervisedMeters(c['K'], DEV)
    head = c['head'].to(DEV).requires_grad_()
    cw = None if c['cw'] is None else c['cw'].to(DEV)
    assert ag.ce_head_fits(head, c['target'])
    loss = ag.ce_head_meters(head, c['target'].to(DEV), cw, c['ignore'], meters)
    loss.backward()
    loss = loss.detach()
    lerr = cc.loss_error(float(loss), ref['loss'])
    e = cc.grad_errors(head.grad, ref['ghead'])
    print('node C=%d %s: loss %.9g against %.9g (%.2e); gradient rel %.2e element %.2e' % (C, kind, float(loss), ref['loss'], lerr, e[0], e[1]))
    assert lerr <= LOSS_TAU and e[0] <= GRAD_TAU_REL and e[1] <= GRAD_TAU_EL
    assert float(meters.sums.abs().max()) == 0.0                                   # cleared for the next step
    assert abs(float(meters.meter[0]) - float(loss) * c['N']) <= 1e-12 * abs(float(loss) * c['N'])
    l1 = np.abs(meters.areas.cpu().numpy().reshape(3, c['K']) - ref['areas']).sum(1)
    assert int(l1.max()) <= 2 * ref['near']
    with torch.no_grad():
        loss2 = ag.ce_head_meters(head, c['target'].to(DEV), cw, c['ignore'], None)
    assert abs(float(loss2) - float(loss)) <= 2.0 ** -22 * abs(float(loss))


def test_unsupported_class_count_takes_the_fallback():
    """21 classes (pascal): `supported` says 0, the launch refuses before anything runs, the node's fallback meets the same reference."""
    from mspl_amd import autograd as ag
    from mspl_amd.supervised import SupervisedMeters
    check, lib, _p, _stream = _lib()
    C, (hs, size), N = 21, SHAPES[1], 2
    g = torch.Generator().manual_seed(C * 100 + size[0])
    head = torch.randn((N, C) + hs, generator=g) * 3
    target = torch.randint(0, C, (N,) + size, generator=g)
    target[torch.rand((N,) + size, generator=g) < 0.1] = 255
    K = C - 1
    ref = _reference(head, target, None, 255, size, K)
    assert ref['near'] <= NEAR_CAP * target.numel()
    assert lib.mspl_ce_head_supported(C) == 0 and lib.mspl_ce_head_fits(N, C, hs[0], hs[1], size[0], size[1]) == 0
    assert lib.mspl_ce_head_fits(N, 5, size[0], size[1], hs[0], hs[1]) == 0          # a head larger than the label map
    hd = head.to(DEV).requires_grad_()
    td = target.to(DEV)
    sums = torch.zeros(2, dtype=torch.float64, device=DEV)
    rc = lib.mspl_ce_head_meters_fwd_bwd(_p(hd), _p(td), None, 255, N, C, hs[0], hs[1], size[0], size[1], K, _p(sums), None, None, _stream())
    assert rc != 0 and float(sums.abs().max()) == 0.0
    with pytest.raises(RuntimeError):
        ag.ce_head_meters(hd, td, None, 255, None, fused=True)
    meters = SupervisedMeters(K, DEV)
    loss = ag.ce_head_meters(hd, td, None, 255, meters)
    loss.backward()
    loss = loss.detach()
    lerr = cc.loss_error(float(loss), ref['loss'])
    e = cc.grad_errors(hd.grad, ref['ghead'])
    print('fallback C=21: loss %.9g against %.9g (%.2e); gradient rel %.2e element %.2e' % (float(loss), ref['loss'], lerr, e[0], e[1]))
    assert lerr <= LOSS_TAU and e[0] <= GRAD_TAU_REL and e[1] <= GRAD_TAU_EL
    l1 = np.abs(meters.areas.cpu().numpy().reshape(3, K) - ref['areas']).sum(1)
    assert int(l1.max()) <= 2 * ref['near']


def test_node_in_a_graph_replayed_three_times():
    """(The captured leaf is a tensor of its own, first used inside the capture: autograd runs a leaf's AccumulateGrad on the stream
    that was current when the leaf was first used, and a leaf first used eagerly would pull the default stream into the capture.)"""
    from mspl_amd import autograd as ag
    from mspl_amd.supervised import SupervisedMeters
    c = _case(5, 0, 'weighted')
    meters = SupervisedMeters(c['K'], DEV)
    td, cw = c['target'].to(DEV), c['cw'].to(DEV)
    with torch.no_grad():                                               # eager once: what one application adds
        one_loss = ag.ce_head_meters(c['head'].to(DEV), td, cw, c['ignore'], meters).clone()
    one_areas = meters.areas.clone()
    meters.reset()
    head = c['head'].to(DEV).requires_grad_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gl = ag.ce_head_meters(head, td, cw, c['ignore'], meters)
        gl.backward()
    meters.reset()
    losses = []
    for _ in range(3):
        graph.replay()
        losses.append(gl.detach().clone())
    torch.cuda.synchronize()
    assert torch.equal(losses[0], losses[1]) and torch.equal(losses[1], losses[2])
    assert abs(float(losses[0]) - float(one_loss)) <= 2.0 ** -22 * abs(float(one_loss))
    assert torch.equal(meters.areas, 3 * one_areas)
    want = 3 * float(losses[0]) * c['N']
    assert abs(float(meters.meter[0]) - want) <= 1e-12 * want
    e = cc.grad_errors(head.grad, c['ref']['ghead'])
    assert e[0] <= GRAD_TAU_REL and e[1] <= GRAD_TAU_EL


@functools.lru_cache(maxsize=None)
def _confident_case(C, mag):
    hs, size = SHAPES[0]
    head, _, target = cc.confident_logits(2, C, hs, mag, 'agree', 7, target_size=size, ignore=255)
    cw = cc.class_weights(C)
    K = C - 1
    r64 = _reference(head, target, cw, 255, size, K)
    r32 = _reference(head, target, cw, 255, size, K, torch.float32)
    return head, target, cw, size, K, r64, r32


@pytest.mark.parametrize('mag', cc.TRAIN_MAGNITUDES)
@pytest.mark.parametrize('C', (5, 20))
def test_trained_logit_magnitudes(C, mag):
    head, target, cw, size, K, r64, r32 = _confident_case(C, mag)
    sums, areas, gfull, ghead = _launch(head, target, cw, 255, size, K)
    s = sums.cpu().numpy()
    loss = s[0] / s[1]
    lunit = max(cc.loss_error(r32['loss'], r64['loss']), FLOOR)
    e32 = cc.grad_errors(r32['ghead'], r64['ghead'])
    e = cc.grad_errors(ghead, r64['ghead'])
    lerr = cc.loss_error(loss, r64['loss'])
    units = (lerr / lunit, e[0] / max(e32[0], FLOOR), e[1] / max(e32[1], FLOOR))
    print('C=%d magnitude %d: loss %.9g against %.9g, %.2f units of max(err32 = %.2e, 2**-22); gradient rel %.2e = %.2f units of '
          'max(%.2e, 2**-22), element %.2e = %.2f units of max(%.2e, 2**-22)'
          % (C, mag, loss, r64['loss'], units[0], cc.loss_error(r32['loss'], r64['loss']), e[0], units[1], e32[0], e[1], units[2], e32[1]))
    assert torch.isfinite(ghead).all()
    assert max(units) <= cc.MARGIN
    assert abs(s[1] - r64['den']) <= DEN_RTOL * r64['den']
