"""mspl_nid_heads_fwd / mspl_nid_finalize / mspl_nid_heads_bwd (mspl_amd/csrc/nid_heads.hip): NIDLoss on the up-sampled main head,
from the low-resolution head.

1. Against the reference in float64 (tests/golden/nid_heads.npz, the reference's NIDLoss on F.interpolate(main_lo)): histogram
   within GAP_FACTOR x gap_hist, loss2 within rtol 1e-4 / atol 2e-4 (the bound of test_nid_loss_vs_reference_golden) or GAP_FACTOR x
   gap_loss if larger, gradient w.r.t. main_lo within max(GAP_FACTOR x gap_grad, 2e-4 max |ref|).  The gaps are the largest
   distance of the reference's own float32 runs (tests/nid_heads_cases.py FLOAT32_RUNS) from its float64 run, recorded by the
   generator; never ours.  Measured: the worst case (x2) uses 0.43 of its gradient bound and 0.45 of its histogram bound.
2. Against the three-step form on the device (mspl_bilinear_fwd -> mspl_nid_hist_fwd / mspl_nid_hist_bwd with the same gjoint / gpl
   -> mspl_bilinear_bwd).  Per-pixel values are the same floats by construction, only summation order differs: histograms within
   the bound of 1 of each other; head gradients |fused - three_step| <= 2 n 2^-24 mspl_bilinear_bwd(|g_full|) element-wise, n the
   plan's largest number of label pixels one head pixel feeds.  Immune to the 5e5 amplification of NIDLoss's slopes.
3. mspl_nid_finalize on the fixtures' histograms against float64 autograd of the reference's nid() and normalisations: loss2 rtol
   1e-6, gjoint / gpl 1e-5 of their largest entry.
4. Determinism and contract: the forward is bit-identical over two runs, gmain_lo is accumulated into, an unsupported plan returns
   MSPL_ERR_UNSUPPORTED and leaves the outputs untouched, and the 20-class K = 32 head does what the plan says.
Each test prints what it measured."""
import functools

import numpy as np
import pytest
import torch

from tests import nid_heads_cases as nc

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CASES = sorted(nc.NID_HEADS_CASES)


def _lib():
    from mspl_amd._native import CONSTANTS, check, lib
    from mspl_amd.ops import _p, _stream
    return CONSTANTS, check, lib, _p, _stream


def _sizes(case):
    B, C, K, (Hm, Wm), (H, W) = case[:5]
    Cl = min(C, K)
    return B, C, K, Hm, Wm, H, W, Cl, K * Cl + K + Cl


def _fused_forward(cam, main, case):
    """(out, ws) of mspl_nid_heads_fwd."""
    _, check, lib, _p, _stream = _lib()
    B, C, K, Hm, Wm, H, W, Cl, E = _sizes(case)
    ws = torch.full((lib.mspl_nid_heads_workspace_floats(C, H, W, K),), float('nan'), device=DEV)
    out = torch.full((E,), float('nan'), device=DEV)
    check(lib.mspl_nid_heads_fwd(_p(cam), _p(main), B, C, Hm, Wm, H, W, K, nc.BW_CAMERA, nc.BW_LABEL, _p(ws), _p(out), _stream()))
    return out, ws


def _finalize(out, case, label_bin=None):
    _, check, lib, _p, _stream = _lib()
    B, C, K, Hm, Wm, H, W, Cl, E = _sizes(case)
    loss2 = torch.full((1,), float('nan'), device=DEV)
    gj = torch.full((K * Cl,), float('nan'), device=DEV)
    gpl = torch.full((Cl,), float('nan'), device=DEV)
    check(lib.mspl_nid_finalize(_p(out), K, C, C if label_bin is None else label_bin, float(B * H * W), _p(loss2), _p(gj), _p(gpl), _stream()))
    return loss2, gj, gpl


@functools.lru_cache(maxsize=None)
def _run(name):
    """Everything the tests of one case share, computed once: inputs on the device, the fused chain and the three-step chain."""
    _, check, lib, _p, _stream = _lib()
    case = nc.NID_HEADS_CASES[name] if name in nc.NID_HEADS_CASES else nc.WIDE_CASE[1]
    B, C, K, Hm, Wm, H, W, Cl, E = _sizes(case)
    cam, main = (t.to(DEV).contiguous() for t in nc.case_inputs(case))
    out, ws = _fused_forward(cam, main, case)
    loss2, gj, gpl = _finalize(out, case)
    gmain = torch.zeros_like(main)
    check(lib.mspl_nid_heads_bwd(_p(main), B, C, Hm, Wm, H, W, K, nc.BW_LABEL, _p(ws), _p(gj), _p(gpl), None, _p(gmain), _stream()))
    # the three-step form with the same gjoint / gpl
    full = torch.empty((B, C, H, W), device=DEV)
    check(lib.mspl_bilinear_fwd(_p(main), B, C, Hm, Wm, H, W, 1, None, _p(full), _stream()))
    ws3 = torch.empty(lib.mspl_nid_workspace_floats(C, H, W, K), device=DEV)
    out3 = torch.empty(E, device=DEV)
    check(lib.mspl_nid_hist_fwd(_p(cam), _p(full), B, C, H, W, K, nc.BW_CAMERA, nc.BW_LABEL, _p(ws3), _p(out3), _stream()))
    gfull = torch.zeros((B, C, H, W), device=DEV)
    check(lib.mspl_nid_hist_bwd(_p(cam), _p(full), B, C, H, W, K, nc.BW_CAMERA, nc.BW_LABEL, _p(gj), _p(gpl), _p(gfull), _stream()))
    g3 = torch.empty_like(main)
    check(lib.mspl_bilinear_bwd(_p(gfull), B, C, Hm, Wm, H, W, _p(g3), _stream()))
    g3abs = torch.empty_like(main)
    check(lib.mspl_bilinear_bwd(_p(gfull.abs().contiguous()), B, C, Hm, Wm, H, W, _p(g3abs), _stream()))
    torch.cuda.synchronize()
    host = dict(loss2=loss2, gj=gj, gpl=gpl, gmain=gmain, out3=out3, g3=g3, g3abs=g3abs)          # float64 numpy copies
    r = dict((k, v.cpu().double().numpy()) for k, v in host.items())
    r.update(case=case, cam=cam, main=main, out=out, ws=ws)                                     # device tensors, left unchanged
    return r


def _hist_bound(fixture, name):
    return nc.GAP_FACTOR * float(fixture[name + '.gap_hist'])


@pytest.fixture(scope='module')
def fixture(golden):
    return golden('nid_heads')


@pytest.mark.parametrize('name', CASES)
def test_against_the_reference_in_float64(name, fixture):
    r = _run(name)
    out = r['out'].detach().cpu().double().numpy()
    dh = float(np.abs(out - fixture[name + '.hist']).max())
    ref_l = float(fixture[name + '.loss2'])
    dl = abs(float(r['loss2'][0]) - ref_l)
    bl = max(1e-4 * abs(ref_l) + 2e-4, nc.GAP_FACTOR * float(fixture[name + '.gap_loss']))
    ref_g = fixture[name + '.grad']
    dg = float(np.abs(r['gmain'] - ref_g).max())
    bg = max(nc.GAP_FACTOR * float(fixture[name + '.gap_grad']), 2e-4 * float(np.abs(ref_g).max()))
    print('%s: hist %.3e (bound %.3e)  loss2 %.3e (bound %.3e)  grad %.3e (bound %.3e, max |ref| %.3e)'
          % (name, dh, _hist_bound(fixture, name), dl, bl, dg, bg, np.abs(ref_g).max()))
    assert dh <= _hist_bound(fixture, name)
    assert dl <= bl
    assert dg <= bg


@pytest.mark.parametrize('name', CASES)
def test_against_the_three_step_form_on_the_device(name, fixture):
    from mspl_amd import autograd as ag
    r = _run(name)
    B, C, K, Hm, Wm, H, W, Cl, E = _sizes(r['case'])
    n = ag.nid_heads_plan(B, C, Hm, Wm, H, W, K)['fan']
    out = r['out'].detach().cpu().double().numpy()
    dh = float(np.abs(out - r['out3']).max())
    diff = np.abs(r['gmain'] - r['g3'])
    bound = 2.0 * n * 2.0 ** -24 * r['g3abs']
    worst = float((diff / np.maximum(bound, 1e-300)).max()) if diff.max() > 0 else 0.0
    print('%s: hist fused vs three-step %.3e (bound %.3e); gradient: largest |diff| %.3e, largest diff / bound %.3f, n = %d, non-zero '
          'entries %d' % (name, dh, _hist_bound(fixture, name), diff.max(), worst, n, int((r['g3'] != 0).sum())))
    assert dh <= _hist_bound(fixture, name)
    assert int((r['g3'] != 0).sum()) >= nc.NONZERO_MIN
    assert bool((diff <= bound).all())


def _reference_finalize(hist, K, Cl, C, norm):
    """float64 autograd of the reference's normalisations and nid() (loss_fns/segmentation_loss.py:98-118) on a histogram in the
    (K, Cl) layout, label_bin = C: (loss2, d loss2 / d joint / norm, d loss2 / d p_l / norm)."""
    h = torch.tensor(hist, dtype=torch.float64)
    joint = torch.zeros(K, C, dtype=torch.float64)
    joint[:, :Cl] = h[:K * Cl].reshape(K, Cl)
    p_l = torch.zeros(C, dtype=torch.float64)
    p_l[:Cl] = h[K * Cl + K:]
    p_c = h[K * Cl:K * Cl + K].clone()
    joint.requires_grad_(True)
    p_l.requires_grad_(True)
    eps = 1e-7
    a, b, c = joint / joint.sum(), (p_c / p_c.sum()).reshape(-1, 1), (p_l / p_l.sum()).reshape(-1, 1)
    I = torch.sum(a * (torch.log(a + eps) - torch.log(torch.mm(b, c.t()) + eps)))
    Hh = -torch.sum(a * torch.log(a + eps))
    loss = ((1 - I / Hh) - 0.95) * 20
    loss.backward()
    return float(loss.detach()), (joint.grad[:, :Cl] / norm).numpy().reshape(-1), (p_l.grad[:Cl] / norm).numpy()


@pytest.mark.parametrize('name', CASES)
def test_finalize_against_float64_autograd(name, fixture):
    case = nc.NID_HEADS_CASES[name]
    B, C, K, Hm, Wm, H, W, Cl, E = _sizes(case)
    hist32 = fixture[name + '.hist'].astype(np.float32)
    loss2, gj, gpl = _finalize(torch.from_numpy(hist32).to(DEV), case)
    ref_l, ref_gj, ref_gpl = _reference_finalize(hist32.astype(np.float64), K, Cl, C, float(B * H * W))
    got_l, got_gj, got_gpl = float(loss2[0]), gj.cpu().double().numpy(), gpl.cpu().double().numpy()
    ej = float(np.abs(got_gj - ref_gj).max() / np.abs(ref_gj).max())
    ep = float(np.abs(got_gpl - ref_gpl).max() / np.abs(ref_gpl).max())
    print('%s: loss2 %.9f vs %.9f (%.2e relative)  gjoint %.2e  gpl %.2e of the largest entry'
          % (name, got_l, ref_l, abs(got_l - ref_l) / abs(ref_l), ej, ep))
    assert abs(got_l - ref_l) <= 1e-6 * abs(ref_l)
    assert ej <= 1e-5 and ep <= 1e-5


def test_finalize_with_fewer_label_bins_than_classes():
    """label_bin < C: the bins beyond it do not enter the loss and get zero gradients."""
    case = nc.NID_HEADS_CASES['x2']
    B, C, K, Hm, Wm, H, W, Cl, E = _sizes(case)
    r = _run('x2')
    loss2, gj, gpl = _finalize(r['out'], case, label_bin=3)
    h = r['out'].cpu().double().numpy()
    sub = np.concatenate([h[:K * Cl].reshape(K, Cl)[:, :3].reshape(-1), h[K * Cl:K * Cl + K], h[K * Cl + K:][:3]])
    ref_l, ref_gj, ref_gpl = _reference_finalize(sub, K, 3, 3, float(B * H * W))
    gj = gj.cpu().double().numpy().reshape(K, Cl)
    assert abs(float(loss2[0]) - ref_l) <= 1e-6 * abs(ref_l)
    assert np.abs(gj[:, :3].reshape(-1) - ref_gj).max() <= 1e-5 * np.abs(ref_gj).max()
    assert not gj[:, 3:].any() and not gpl.cpu().numpy()[3:].any()


@pytest.mark.parametrize('name', ['x2', 'many_bands', 'odd_k_below_c'])
def test_forward_is_bit_identical_and_backward_accumulates(name):
    _, check, lib, _p, _stream = _lib()
    r = _run(name)
    case = r['case']
    B, C, K, Hm, Wm, H, W, Cl, E = _sizes(case)
    out2, ws2 = _fused_forward(r['cam'], r['main'], case)
    assert torch.equal(out2, r['out']) and not bool(torch.isnan(out2).any())
    assert torch.equal(ws2, r['ws']) and not bool(torch.isnan(ws2).any())          # partials and camera columns, every element written
    # accumulated into: twice into one buffer, upstream gradients 0.5 and 2 -> 2.5 x the gradient on top of what was there
    gj, gpl = (torch.from_numpy(r[k]).float().to(DEV) for k in ('gj', 'gpl'))
    base = torch.full_like(r['main'], 3.0)
    buf = base.clone()
    for s in (0.5, 2.0):
        gs = torch.tensor([s], device=DEV)
        check(lib.mspl_nid_heads_bwd(_p(r['main']), B, C, Hm, Wm, H, W, K, nc.BW_LABEL, _p(r['ws']), _p(gj), _p(gpl), _p(gs), _p(buf), _stream()))
    want = 3.0 + 2.5 * r['gmain']
    tol = 1e-5 * np.abs(want).max()
    assert np.abs(buf.cpu().double().numpy() - want).max() <= tol


def test_unsupported_plan_launches_nothing():
    CONSTANTS, check, lib, _p, _stream = _lib()
    B, C, K, (Hm, Wm), (H, W) = nc.REFUSED_SHAPE
    Cl, E = min(C, K), K * min(C, K) + K + min(C, K)
    cam = torch.rand((B, 3, H, W), device=DEV)
    main = torch.randn((B, C, Hm, Wm), device=DEV)
    ws = torch.full((lib.mspl_nid_heads_workspace_floats(C, H, W, K),), 7.0, device=DEV)
    out = torch.full((E,), 7.0, device=DEV)
    gmain = torch.full_like(main, 7.0)
    gj, gpl = torch.zeros(K * Cl, device=DEV), torch.zeros(Cl, device=DEV)
    plan = (__import__('ctypes').c_int32 * CONSTANTS['NH_PLAN_LEN'])()
    assert lib.mspl_nid_heads_plan(B, C, Hm, Wm, H, W, K, plan) == CONSTANTS['ERR_UNSUPPORTED']
    assert lib.mspl_nid_heads_fwd(_p(cam), _p(main), B, C, Hm, Wm, H, W, K, nc.BW_CAMERA, nc.BW_LABEL, _p(ws), _p(out), _stream()) == CONSTANTS['ERR_UNSUPPORTED']
    assert lib.mspl_nid_heads_bwd(_p(main), B, C, Hm, Wm, H, W, K, nc.BW_LABEL, _p(ws), _p(gj), _p(gpl), None, _p(gmain), _stream()) == CONSTANTS['ERR_UNSUPPORTED']
    torch.cuda.synchronize()
    assert bool((ws == 7.0).all()) and bool((out == 7.0).all()) and bool((gmain == 7.0).all())
    # the public surface says the same, and forward_loss's fallback is NIDLoss.forward on the up-sampled head
    from mspl_amd import losses
    assert not losses.NIDLoss(image_bin=K, label_bin=C).heads_supported(cam, main)


def test_twenty_classes_with_32_bins_follow_the_plan():
    """The plan covers a 20-class head with K = 32 (84 KB of LDS): it runs, and agrees with the three-step form and the float64 oracle."""
    from mspl_amd import autograd as ag
    name, case = nc.WIDE_CASE
    B, C, K, Hm, Wm, H, W, Cl, E = _sizes(case)
    plan = ag.nid_heads_plan(B, C, Hm, Wm, H, W, K)
    assert plan is not None and plan['lds_fwd'] > 64 * 1024
    r = _run(name)
    cam, main = nc.case_inputs(case)
    ref_l, ref_g = nc.oracle_nid_at_heads(cam, main, K, C)
    dl = abs(float(r['loss2'][0]) - float(ref_l))
    diff = np.abs(r['gmain'] - r['g3'])
    bound = 2.0 * plan['fan'] * 2.0 ** -24 * r['g3abs']
    print('%s: loss2 fused vs float64 oracle %.3e; gradient vs three-step largest |diff| %.3e' % (name, dl, diff.max()))
    assert dl <= 1e-4 * abs(float(ref_l)) + 2e-4
    assert bool((diff <= bound).all()) and int((r['g3'] != 0).sum()) >= nc.NONZERO_MIN
    assert float(np.abs(r['out'].cpu().double().numpy() - r['out3']).max()) <= 1e-5


@pytest.mark.parametrize('name', ['x2', 'odd_k_below_c'])
def test_autograd_node_and_loss_surface(name, fixture):
    """losses.NIDLoss.at_heads / autograd.nid_heads: value and gradient (through a scaled sum, so the upstream gradient is not 1)."""
    from mspl_amd import losses
    r = _run(name)
    case = r['case']
    B, C, K = case[:3]
    nid = losses.NIDLoss(image_bin=K, label_bin=C, bw_camera=nc.BW_CAMERA, bw_label=nc.BW_LABEL)
    assert nid.heads_supported(r['cam'], r['main'])
    m = r['main'].clone().requires_grad_(True)
    loss2 = nid.at_heads(r['cam'], m)
    (0.25 * loss2).backward()
    loss2 = loss2.detach()
    assert abs(float(loss2) - float(r['loss2'][0])) == 0.0
    want = 0.25 * r['gmain']
    assert np.abs(m.grad.cpu().double().numpy() - want).max() <= 1e-5 * np.abs(want).max()
    # and NIDLoss.forward on the up-sampled head (the three-step surface) gives the same loss within the reference bound
    from mspl_amd import autograd as ag
    full = nid(r['cam'], ag.bilinear(r['main'], tuple(r['cam'].shape[2:])))
    assert abs(float(full) - float(loss2)) <= 1e-4 * abs(float(loss2)) + 2e-4
