"""Every kernel that takes a softmax, a log-sum-exp or a KL divergence, at the logit magnitudes of a trained network (|logit| up to
~160, heads that agree, KL of 1e-2 or less -- tests/confident_cases.py), against float64.

The unit of a KL or probability bound is the float32 oracle's own error on the case (the CPU, ATen), floored at 2**-22 / 2**-23:
    |kernel - float64| <= MARGIN * max(err32, floor),  MARGIN = 4.
Why 4: the kernels sum the classes in another order than ATen; v_exp_f32 / v_log_f32 take one to two ulp where libm takes under
one; three rounded terms add up; and the centred formula restated in numpy float32 stays under 1.5 units on every case
(tests/test_confident_cases.py).  The formula labels.hip used before (T1/S1 - lse(main) + lse(aux) on raw logits) misses this by
8x to 40x on the `agree` and `same` cases from magnitude 8 on.  Loss and gradient bounds are the project's own
(tests/test_gpu_supervised_grad_parity.py).  Each test prints what it measured."""
import numpy as np
import pytest
import torch

from tests import confident_cases as cc
from tests.train_loop_cases import reference_areas

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SUMS_RTOL = 1e-6                            # tests/test_gpu_ce_meters.py


def _lib():
    from mspl_amd._native import check, lib
    from mspl_amd.ops import _p, _stream
    return check, lib, _p, _stream


# ------------------------------------------------------------------ label epilogue
def _check_kld(tag, got, ref, heads):
    unit = cc.kld_unit(ref)
    got = got.cpu().double()
    ratio = float((got - ref['kld64']).abs().max()) / unit
    print('%s: KL map %.2f units of max(err32 = %.2e, 2**-22); min %.3e' % (tag, ratio, ref['err32'], float(got.min())))
    assert torch.isfinite(got).all()
    assert ratio <= cc.MARGIN
    if heads == 'same':
        assert float(got.abs().max()) <= cc.MARGIN * cc.KLD_FLOOR


def _check_labels(tag, got, pred, aux, size, ref):
    got = got.cpu()
    if tuple(pred.shape[-2:]) == tuple(aux.shape[-2:]) == tuple(size):       # no interpolation: the float32 sum decides, exactly
        assert torch.equal(got, (pred + 0.5 * aux).argmax(1).to(torch.uint8))
    else:
        assert ref['excluded'] <= cc.TIE_CAP * got.numel()
        bad = (got != ref['labels64']) & ref['sure']
        print('%s: %d near-ties left out, %d other labels differ' % (tag, ref['excluded'], int(bad.sum())))
        assert int(bad.sum()) == 0


def _form(name):
    return name.split('_')[0]


@pytest.mark.parametrize('case', [c for c in cc.LABEL_CASES if _form(c[0]) in ('lds', 'wide', 'odd', 'id')], ids=cc.label_case_id)
def test_label_epilogue_lds_form_and_histogram_form(case):
    """The LDS-staged kernel in each instantiation; the histogram form of the same launch equals it bit for bit."""
    from mspl_amd import ops
    name, mag, heads = case
    pred, aux, size, ref = cc.label_case(case)
    C = pred.shape[1]
    pd, ad = pred.to(DEV), aux.to(DEV)
    assert ops.label_epilogue_hist_fits(pd, ad, size)
    r = ops.label_epilogue(pd, ad, size, want_kld=True)
    tag = cc.label_case_id(case)
    _check_kld(tag, r['kld'], ref, heads)
    _check_labels(tag, r['labels'], pred, aux, size, ref)
    hist = torch.zeros(C, dtype=torch.int64, device=DEV)
    h = ops.label_epilogue_hist(pd, ad, size, hist, C, want_kld=True)
    assert torch.equal(h['labels'], r['labels']) and torch.equal(h['kld'], r['kld'])
    assert hist.cpu().tolist() == np.bincount(r['labels'].cpu().numpy().ravel(), minlength=C).tolist()


@pytest.mark.parametrize('case', [c for c in cc.LABEL_CASES if _form(c[0]) == 'reg'], ids=cc.label_case_id)
def test_label_epilogue_register_form(case):
    from mspl_amd import ops
    name, mag, heads = case
    pred, aux, size, ref = cc.label_case(case)
    pd, ad = pred.to(DEV), aux.to(DEV)
    assert pred.shape[1] <= 24 and not ops.label_epilogue_hist_fits(pd, ad, size)
    r = ops.label_epilogue(pd, ad, size, want_kld=True)
    tag = cc.label_case_id(case)
    _check_kld(tag, r['kld'], ref, heads)
    _check_labels(tag, r['labels'], pred, aux, size, ref)


@pytest.mark.parametrize('case', [c for c in cc.LABEL_CASES if _form(c[0]) == 'gen'], ids=cc.label_case_id)
def test_label_epilogue_general_form(case):
    """More than 24 classes, or the probabilities / up-sampled logits asked for (get_output's drop-in form)."""
    from mspl_amd import ops
    name, mag, heads = case
    pred, aux, size, ref = cc.label_case(case)
    pd, ad = pred.to(DEV), aux.to(DEV)
    tag = cc.label_case_id(case)
    if pred.shape[1] > 24:
        r = ops.label_epilogue(pd, ad, size, want_kld=True)
        _check_kld(tag, r['kld'], ref, heads)
        _check_labels(tag, r['labels'], pred, aux, size, ref)
        return
    r = ops.label_epilogue(pd, ad, size, want_kld=True, want_prob=True)
    _check_kld(tag + ' (prob)', r['kld'], ref, heads)
    _check_labels(tag, r['labels'], pred, aux, size, ref)
    punit = max(ref['perr32'], cc.PROB_FLOOR)
    pratio = float((r['prob'].cpu().double() - ref['prob64']).abs().max()) / punit
    print('%s: probabilities %.2f units of max(err32 = %.2e, 2**-23)' % (tag, pratio, ref['perr32']))
    assert pratio <= cc.MARGIN
    r2 = ops.label_epilogue(pd, ad, size, want_kld=True, want_logits=True)
    assert torch.equal(r2['kld'], r['kld']) and torch.equal(r2['labels'], r['labels'])


# ------------------------------------------------------------------ the fused uest loss (K11) and its head-resolution forms
def _check_loss(tag, loss, gp, ga, r64):
    l64, gp64, ga64 = r64
    lerr = cc.loss_error(float(loss), l64)
    ep, ea = cc.grad_errors(gp, gp64), cc.grad_errors(ga, ga64)
    print('%s: loss %.9g against %.9g (%.2e); gpred rel %.2e element %.2e; gaux rel %.2e element %.2e'
          % (tag, float(loss), l64, lerr, ep[0], ep[1], ea[0], ea[1]))
    assert torch.isfinite(gp).all() and torch.isfinite(ga).all()
    assert lerr <= cc.LOSS_TAU
    assert max(ep[0], ea[0]) <= cc.GRAD_TAU_REL and max(ep[1], ea[1]) <= cc.GRAD_TAU_EL


@pytest.mark.parametrize('scaled', [False, True], ids=['plain', 'scaled'])
@pytest.mark.parametrize('case', cc.grid(cc.FULL_SHAPES), ids=cc.grid_id)
def test_uw_loss(case, scaled):
    check, lib, _p, _stream = _lib()
    out_scale = 0.25 if scaled else 1.0
    r = cc.loss_case(case, out_scale)
    pred, aux, tgt, cw = [r[k].to(DEV) for k in ('pred', 'aux', 'target', 'cw')]
    N, C, H, W = pred.shape
    loss = torch.zeros(1, device=DEV)
    gp, ga = torch.empty_like(pred), torch.empty_like(aux)
    if scaled:
        check(lib.mspl_uw_loss_scaled_fwd_bwd(_p(pred), _p(aux), _p(tgt), _p(cw), N, C, H * W, 20.0, out_scale, _p(loss), _p(gp), _p(ga), None,
                                              _stream()))
    else:
        check(lib.mspl_uw_loss_fwd_bwd(_p(pred), _p(aux), _p(tgt), _p(cw), N, C, H * W, 20.0, _p(loss), _p(gp), _p(ga), None, _stream()))
    _check_loss(cc.grid_id(case) + (' x0.25' if scaled else ''), loss[0], gp, ga, r['ref64'])


def _heads_call(r, meters=None):
    check, lib, _p, _stream = _lib()
    main, aux, tgt, cw = [r[k].to(DEV) for k in ('pred', 'aux', 'target', 'cw')]
    N, C, Hm, Wm = main.shape
    Ha, Wa = aux.shape[2:]
    H, W = r['size']
    loss = torch.zeros(1, device=DEV)
    g = torch.empty((2, N, C, H, W), device=DEV)
    if meters is None:
        check(lib.mspl_uw_loss_heads_fwd_bwd(_p(main), _p(aux), _p(tgt), _p(cw), N, C, Hm, Wm, Ha, Wa, H, W, 20.0, 1.0, _p(loss), _p(g[0]), _p(g[1]),
                                             _stream()))
    else:
        K, areas, meter = meters
        check(lib.mspl_uw_loss_heads_meters_fwd_bwd(_p(main), _p(aux), _p(tgt), _p(cw), N, C, Hm, Wm, Ha, Wa, H, W, 20.0, 1.0, _p(loss), _p(g[0]),
                                                    _p(g[1]), K, float(N), _p(areas), _p(meter), _stream()))
    return loss[0], g[0], g[1]


@pytest.mark.parametrize('case', cc.grid(cc.HEADS_SHAPES), ids=cc.grid_id)
def test_uw_loss_at_head_resolution(case):
    from mspl_amd import autograd as ag
    r = cc.loss_case(case)
    assert ag.uw_loss_heads_supported(r['C'])
    loss, gp, ga = _heads_call(r)
    _check_loss(cc.grid_id(case), loss, gp, ga, r['ref64'])


@pytest.mark.parametrize('case', cc.grid([s for s in cc.HEADS_SHAPES if s[2] == 5]), ids=cc.grid_id)
def test_uw_loss_at_head_resolution_with_meters(case):
    r = cc.loss_case(case)
    K = r['C'] - 1
    areas = torch.zeros(3 * K, dtype=torch.int64, device=DEV)
    meter = torch.zeros(2, dtype=torch.float64, device=DEV)
    loss, gp, ga = _heads_call(r, (K, areas, meter))
    _check_loss(cc.grid_id(case) + ' (meters)', loss, gp, ga, r['ref64'])
    up64 = cc.upsample(r['pred'].double(), r['size'])               # the meters take the first maximum of the MAIN head alone
    top = torch.sort(up64, dim=1, descending=True)[0]
    near = int(((top[:, 0] - top[:, 1]) <= cc.TIE_GAP_REL * case[1]).sum())
    want = reference_areas(up64.argmax(1).numpy(), r['target'].numpy(), K)
    diff = int(np.abs(areas.cpu().numpy().reshape(3, K) - want).max())
    print('%s: %d near-ties of the main head, largest area difference %d' % (cc.grid_id(case), near, diff))
    assert near <= cc.TIE_CAP * top[:, 0].numel() and diff <= near          # exact but for a label a near-tie may turn
    assert abs(float(meter[0]) - float(loss) * r['N']) <= 1e-6 * abs(float(loss) * r['N'])


# ------------------------------------------------------------------ PixelwiseKLD
@pytest.mark.parametrize('case', cc.grid(cc.KLD_SHAPES, heads=cc.HEADS), ids=cc.grid_id)
def test_pixelwise_kld_forward_and_backward(case):
    check, lib, _p, _stream = _lib()
    (name, N, C, size), mag, heads = case
    r = cc.kld_case(case)
    a, b = r['d1'].to(DEV), r['d2'].to(DEV)
    H, W = size
    out = torch.empty((N, H, W), device=DEV)
    check(lib.mspl_pixelwise_kld_fwd(_p(a), _p(b), N, C, H * W, _p(out), _stream()))
    _check_kld(cc.grid_id(case), out, r['ref'], heads)
    g1_64, g2_64 = r['g64']
    g1, g2 = torch.empty_like(a), torch.empty_like(b)
    check(lib.mspl_pixelwise_kld_bwd(_p(a), _p(b), _p(r['gk'].to(DEV)), N, C, H * W, _p(g1), _p(g2), _stream()))
    assert torch.isfinite(g1).all() and torch.isfinite(g2).all()
    if heads == 'same':
        # the float64 gradients are the rounding of aux = pred + 3 here (1e-6 and below; the float32 oracle is off by 30 % to 200 % of
        # them), so the relative bounds do not apply: absolute, in units of the float32 oracle's own error (cc.kld_case)
        d = max(float((g1.cpu().double() - g1_64).abs().max()), float((g2.cpu().double() - g2_64).abs().max()))
        print('%s: gradients within %.2f units of %.2e (float32 oracle)' % (cc.grid_id(case), d / r['grad_unit'], r['grad_unit']))
        assert d <= cc.MARGIN * r['grad_unit']
        return
    e1, e2 = cc.grad_errors(g1, g1_64), cc.grad_errors(g2, g2_64)
    print('%s: gd1 rel %.2e element %.2e; gd2 rel %.2e element %.2e' % (cc.grid_id(case), e1[0], e1[1], e2[0], e2[1]))
    assert max(e1[0], e2[0]) <= cc.GRAD_TAU_REL and max(e1[1], e2[1]) <= cc.GRAD_TAU_EL


# ------------------------------------------------------------------ weighted cross entropy
@pytest.mark.parametrize('mode', ['all', 'weights'])
@pytest.mark.parametrize('with_u', [True, False], ids=['u', 'nou'])
@pytest.mark.parametrize('case', cc.grid(cc.CE_SHAPES), ids=cc.grid_id)
def test_weighted_ce_forward_and_backward(case, with_u, mode):
    check, lib, _p, _stream = _lib()
    (name, N, C, size), mag, heads = case
    r = cc.wce_case(case, with_u, mode)
    x, tgt, u, cw = r['x'], r['target'], r['u'], r['cw']
    num64, den64, gp64, gu64 = r['ref64']
    xd, td, cwd = x.to(DEV), tgt.to(DEV), cw.to(DEV)
    ud = None if u is None else u.to(DEV)
    H, W = size
    sums = torch.zeros(2, device=DEV)
    check(lib.mspl_weighted_ce_fwd(_p(xd), _p(td), _p(ud), _p(cwd), 255, N, C, H * W, _p(sums), _stream()))
    s = sums.cpu().double().numpy()
    tag = '%s %s %s' % (cc.grid_id(case), 'u' if with_u else 'no u', mode)
    print('%s: sums[0] %.9g against %.9g (%.2e), sums[1] %.9g against %.9g' % (tag, s[0], num64, abs(s[0] - num64) / abs(num64), s[1], den64))
    assert abs(s[0] - num64) <= cc.LOSS_TAU * abs(num64)
    assert abs(s[1] - den64) <= 2.0 ** -23 * den64 * 4            # a float32 sum of a few thousand weights in a tree of partial sums
    g = torch.ones(1, device=DEV)
    gp = torch.empty_like(xd)
    gu = torch.empty((N, H, W), device=DEV) if with_u else None
    den = sums[1:] if mode == 'weights' else None
    check(lib.mspl_weighted_ce_bwd(_p(xd), _p(td), _p(ud), _p(cwd), 255, N, C, H * W, _p(g), _p(den), _p(gp), _p(gu), _stream()))
    ep = cc.grad_errors(gp, gp64)
    eu = cc.grad_errors(gu, gu64) if with_u else (0.0, 0.0)
    print('%s: gpred rel %.2e element %.2e; gu rel %.2e element %.2e' % (tag, ep[0], ep[1], eu[0], eu[1]))
    assert max(ep[0], eu[0]) <= cc.GRAD_TAU_REL and max(ep[1], eu[1]) <= cc.GRAD_TAU_EL


# ------------------------------------------------------------------ the cross-entropy meters and the evaluation epilogue
@pytest.mark.parametrize('case', cc.grid(cc.CE_SHAPES), ids=cc.grid_id)
def test_ce_meters(case):
    check, lib, _p, _stream = _lib()
    (name, N, C, size), mag, heads = case
    pred, aux, tgt = cc.confident_logits(N, C, size, mag, heads, 4, ignore=255)
    x = (pred + 0.5 * aux).reshape(N, C, -1).contiguous()
    t = tgt.reshape(N, -1).contiguous()
    cw = cc.class_weights(C)
    K = C - 1
    num, den = cc.ce_sums_reference(x, t, cw, 255)
    sums = torch.zeros(2, dtype=torch.float64, device=DEV)
    areas = torch.zeros(3 * K, dtype=torch.int64, device=DEV)
    xd, td, cwd = x.to(DEV), t.to(DEV), cw.to(DEV)
    check(lib.mspl_ce_meters_fwd(_p(xd), _p(td), _p(cwd), 255, N, C, x.shape[2], K, _p(sums), _p(areas), _stream()))
    s = sums.cpu().numpy()
    print('%s: num %.12g against %.12g (%.2e), den %.12g against %.12g' % (cc.grid_id(case), s[0], num, abs(s[0] - num) / abs(num), s[1], den))
    assert abs(s[0] - num) <= SUMS_RTOL * abs(num) and abs(s[1] - den) <= SUMS_RTOL * abs(den)
    assert np.array_equal(areas.cpu().numpy().reshape(3, K), reference_areas(torch.max(x, 1)[1].numpy(), t.numpy(), K))


@pytest.mark.parametrize('case', cc.grid(cc.EVAL_SHAPES), ids=cc.grid_id)
def test_eval_epilogue(case):
    from mspl_amd import evaluation as ev
    (name, N, C, ms, as_, size), mag, heads = case
    pred, aux, tgt = cc.confident_logits(N, C, ms, mag, heads, 5, aux_size=as_, target_size=size, ignore=255)
    cw = cc.class_weights(C)
    K = C - 1
    o64 = cc.upsample(pred.double(), size) + 0.5 * cc.upsample(aux.double(), size)
    num, den = cc.ce_sums_reference(o64, tgt, cw, 255)
    top = torch.sort(o64, dim=1, descending=True)[0]
    sure = (top[:, 0] - top[:, 1]) > cc.TIE_GAP_REL * mag
    excluded = int((~sure).sum())
    assert excluded <= cc.TIE_CAP * sure.numel()
    sums = torch.zeros(2, dtype=torch.float64, device=DEV)
    areas = torch.zeros((3, K), dtype=torch.int64, device=DEV)
    labels = torch.empty((N,) + tuple(size), dtype=torch.uint8, device=DEV)
    ev.eval_epilogue(pred.to(DEV), aux.to(DEV), tgt.to(DEV), cw.to(DEV), size, 0.5, 255, K, sums, areas, labels)
    s = sums.cpu().numpy()
    print('%s: num %.12g against %.12g (%.2e), den %.12g against %.12g; %d near-ties left out'
          % (cc.grid_id(case), s[0], num, abs(s[0] - num) / abs(num), s[1], den, excluded))
    assert abs(s[0] - num) <= SUMS_RTOL * abs(num) and abs(s[1] - den) <= SUMS_RTOL * abs(den)
    lab64 = o64.argmax(1).to(torch.uint8)
    assert int(((labels.cpu() != lab64) & sure).sum()) == 0
    want = reference_areas(lab64.numpy(), tgt.numpy(), K)
    assert int(np.abs(areas.cpu().numpy() - want).max()) <= excluded


# ------------------------------------------------------------------ NIDLoss
def test_nid_loss_on_confident_label_logits():
    """The soft-arg-max (beta = 500) of logits of magnitude 20: exp(500 * gap) is far outside float32 without its maximum taken out."""
    from mspl_amd import losses
    N, C, K, size = 2, 5, 16, (18, 44)
    lab, _, _ = cc.confident_logits(N, C, size, 20, 'agree', 6)
    cam = torch.rand((N, 3) + size, generator=torch.Generator().manual_seed(12)) * 1.6 - 0.3
    l64 = lab.double().requires_grad_()
    ref = cc.olab.nid_loss(cam.double(), l64, image_bin=K, label_bin=C)
    ref.backward()
    ld = lab.to(DEV).requires_grad_()
    loss = losses.NIDLoss(image_bin=K, label_bin=C)(cam.to(DEV), ld)
    loss.backward()
    g = ld.grad.cpu()
    zero64 = l64.grad == 0
    print('NIDLoss: %.9g against %.9g; float64 gradient exactly zero on %d of %d elements, the kernel non-zero on %d of those'
          % (float(loss.detach()), float(ref.detach()), int(zero64.sum()), zero64.numel(), int((g[zero64] != 0).sum())))
    torch.testing.assert_close(loss.detach().cpu().double(), ref.detach(), rtol=1e-4, atol=2e-4)
    assert torch.isfinite(g).all()
    assert int(zero64.sum()) > 0 and bool((g[zero64] == 0).all())
