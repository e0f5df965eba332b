"""mspl_ce_meters_fwd / mspl_ce_flood_finalize (mspl_amd/csrc/ce_meters.hip) and autograd.flooded_ce_meters: the cross-entropy sums and
the MIOU areas of train_seg_ue from one read of the logits, the flooding and the loss meter on the device.

Sums: against float64 torch.nn.functional.cross_entropy(weight, ignore_index, reduction='sum') on the CPU, relative 1e-6 -- the
sums are double, so the float32 log-sum-exp per pixel is the whole error (a few 1e-7 relative per term, not accumulating in sign).
Areas: integer, exactly tests.train_loop_cases.reference_areas and exactly mspl_miou_areas_fwd on the same logits."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.train_loop_cases import reference_areas

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SUMS_RTOL = 1e-6
# the bounds of tests/test_gpu_supervised_grad_parity.py for the loss (LOSS_TAU) and for a gradient tensor against float64
# (SUP_TAU_REL: relative norm error, SUP_TAU_EL: largest element error / largest element)
LOSS_TAU, GRAD_TAU_REL, GRAD_TAU_EL = 5e-6, 2e-4, 2.5e-4
CLASSES = (2, 5, 13, 20, 21)
PIXELS = (1, 63, 257, 3 * 256 + 17)


def _lib():
    from mspl_amd._native import check, lib
    from mspl_amd.ops import _p, _stream
    return check, lib, _p, _stream


def _inputs(C, HW, seed, ties=False, N=2):
    """logits (N,C,HW) float32, targets (N,HW) int64 mixing classes 0..C-1 (C-1 is the ignored one), and 255; class weights."""
    g = torch.Generator().manual_seed(7000 + 31 * C + HW + seed)
    x = torch.randn((N, C, HW), generator=g) * 3
    t = torch.randint(0, C, (N, HW), generator=g)
    t[torch.rand((N, HW), generator=g) < 0.1] = 255
    if ties:            # every 7th pixel: a second class takes the value of the maximum (the first of the two must win)
        top, am = x.max(1)
        other = (am + 1 + torch.randint(0, C - 1, am.shape, generator=g)) % C
        sel = (torch.arange(HW) % 7 == 0)[None, :].expand(N, HW)
        x.scatter_(1, torch.where(sel, other, am)[:, None, :], top[:, None, :])
    cw = torch.rand(C, generator=g) + 0.5
    return x, t, cw


def _reference(x, t, cw, ignore, K):
    """(num, den) in float64 through F.cross_entropy, and the (3,K) areas.  Labels outside 0..C-1 contribute nothing to the sums (the
    rule of wce_fwd_kernel): F.cross_entropy refuses them, so they are handed to it as the ignored class."""
    C = x.shape[1]
    tt = torch.where((t < 0) | (t >= C), torch.full_like(t, ignore), t)
    w = torch.ones(C, dtype=torch.float64) if cw is None else cw.double()
    num = float(F.cross_entropy(x.double(), tt, weight=w, ignore_index=ignore, reduction='sum'))
    den = float(w[tt[tt != ignore]].sum())
    return num, den, reference_areas(torch.max(x, 1)[1].numpy(), t.numpy(), K)


def _fwd(x, t, cw, ignore, K, sums=None, areas=None, with_areas=True):
    check, lib, _p, _stream = _lib()
    N, C, HW = x.shape
    sums = torch.zeros(2, dtype=torch.float64, device=DEV) if sums is None else sums
    areas = torch.zeros(3 * K, dtype=torch.int64, device=DEV) if (areas is None and with_areas) else areas
    check(lib.mspl_ce_meters_fwd(_p(x), _p(t), _p(cw), ignore, N, C, HW, K, _p(sums), _p(areas) if with_areas else None, _stream()))
    return sums, areas


@pytest.mark.parametrize('HW', PIXELS)
@pytest.mark.parametrize('C', CLASSES)
def test_sums_and_areas(C, HW):
    from mspl_amd.metrics import MIOU
    K, ignore = C - 1, C - 1
    # Conditioning of the one-pixel shapes: a term is lse - x[t], which cancels when the label is the dominant class, and a sum of
    # one or two such terms carries the rounding of ITS float32 log-sum-exp (half an ulp of |lse| ~ 3e-7 at these logits) relative to
    # a value that can be 100 times smaller.  The first seed whose float64 sum is at least 1 is taken (seed 0 at every larger shape).
    for seed in range(0, 1000, 100):
        x, t, cw = _inputs(C, HW, seed)
        num, den, want = _reference(x, t, cw, ignore, K)
        if num >= 1.0:
            break
    assert num >= 1.0
    xd, td, cwd = x.to(DEV), t.to(DEV), cw.to(DEV)
    sums, areas = _fwd(xd, td, cwd, ignore, K)
    s = sums.cpu().numpy()
    print('C=%d HW=%d: num %.12g against %.12g, den %.12g against %.12g' % (C, HW, s[0], num, s[1], den))
    assert abs(s[0] - num) <= SUMS_RTOL * abs(num) and abs(s[1] - den) <= SUMS_RTOL * abs(den)
    got = areas.cpu().numpy().reshape(3, K)
    assert np.array_equal(got, want)
    assert np.array_equal(got, MIOU(K).areas(xd.view(2, C, 1, HW), td).cpu().numpy())
    # without class weights, and the NULL-areas form
    num1, den1, _ = _reference(x, t, None, ignore, K)
    s1 = _fwd(xd, td, None, ignore, K, with_areas=False)[0].cpu().numpy()
    assert abs(s1[0] - num1) <= SUMS_RTOL * abs(num1) and s1[1] == den1


@pytest.mark.parametrize('C', CLASSES)
def test_first_maximum_wins_a_tie(C):
    from mspl_amd.metrics import MIOU
    K, ignore, HW = C - 1, C - 1, 257
    x, t, cw = _inputs(C, HW, 1, ties=True)
    srt = torch.sort(x, dim=1, descending=True)[0]
    assert int((srt[:, 0] == srt[:, 1]).sum()) == 2 * len(range(0, HW, 7))
    num, den, want = _reference(x, t, cw, ignore, K)
    xd, td = x.to(DEV), t.to(DEV)
    sums, areas = _fwd(xd, td, cw.to(DEV), ignore, K)
    got = areas.cpu().numpy().reshape(3, K)
    assert np.array_equal(got, want) and np.array_equal(got, MIOU(K).areas(xd.view(2, C, 1, HW), td).cpu().numpy())
    s = sums.cpu().numpy()
    assert abs(s[0] - num) <= SUMS_RTOL * abs(num) and abs(s[1] - den) <= SUMS_RTOL * abs(den)


def test_ignore_index_outside_the_classes_and_more_bins_than_classes():
    """ignore_index = 255 (bench.py's camvid setting): every in-range label counts; K above C - 1 leaves the extra bins empty."""
    C, HW, K = 13, 785, 20
    x, t, cw = _inputs(C, HW, 2)
    num, den, want = _reference(x, t, cw, 255, K)
    sums, areas = _fwd(x.to(DEV), t.to(DEV), cw.to(DEV), 255, K)
    s = sums.cpu().numpy()
    assert abs(s[0] - num) <= SUMS_RTOL * abs(num) and abs(s[1] - den) <= SUMS_RTOL * abs(den)
    assert np.array_equal(areas.cpu().numpy().reshape(3, K), want)


def test_outputs_are_accumulated_into():
    C, K, ignore = 5, 4, 4
    a, b = _inputs(C, 785, 3), _inputs(C, 63, 4)
    sums, areas = _fwd(a[0].to(DEV), a[1].to(DEV), a[2].to(DEV), ignore, K)
    one = (sums.cpu().numpy().copy(), areas.cpu().numpy().copy())
    _fwd(b[0].to(DEV), b[1].to(DEV), a[2].to(DEV), ignore, K, sums, areas)
    rb = _reference(b[0], b[1], a[2], ignore, K)
    s = sums.cpu().numpy()
    assert abs((s[0] - one[0][0]) - rb[0]) <= SUMS_RTOL * abs(rb[0]) + 1e-12 * abs(s[0])
    assert abs((s[1] - one[0][1]) - rb[1]) <= SUMS_RTOL * abs(rb[1])
    assert np.array_equal(areas.cpu().numpy() - one[1], rb[2].reshape(-1))


def test_unsupported_bin_counts_are_refused():
    x, t, cw = _inputs(5, 63, 5)
    for K in (0, 65):
        with pytest.raises(RuntimeError, match='MIOU classes'):
            _fwd(x.to(DEV), t.to(DEV), None, 4, K)


def _finalize_expected(s0, s1, b, n):
    l = np.float32(s0) / np.float32(s1)
    d = np.float32(l - np.float32(b))
    out0 = np.float32(np.abs(d) + np.float32(b))
    return out0, np.float32(np.sign(d)), np.float32(s1), float(np.float64(out0) * n)


@pytest.mark.parametrize('which', ['above', 'below', 'equal'])
def test_flood_finalize(which):
    check, lib, _p, _stream = _lib()
    (s0, s1), n = {'above': (2.0, 4.0), 'below': (0.04, 4.0), 'equal': (1.0 / 3.0, 7.0)}[which], 5
    b = float(np.float32(s0) / np.float32(s1)) if which == 'equal' else 0.015
    sums = torch.tensor([s0, s1], dtype=torch.float64, device=DEV)
    meter = torch.tensor([1.5, 0.25], dtype=torch.float64, device=DEV)
    out3 = torch.full((3,), -7.0, dtype=torch.float32, device=DEV)
    check(lib.mspl_ce_flood_finalize(_p(sums), b, n, _p(out3), _p(meter), _stream()))
    want = _finalize_expected(s0, s1, b, n)
    got = out3.cpu().numpy()
    assert got[0] == want[0] and got[1] == want[1] and got[2] == want[2]
    assert got[1] == {'above': 1.0, 'below': -1.0, 'equal': 0.0}[which]
    m = meter.cpu().numpy()
    assert m[0] == 1.5 + want[3] and m[1] == 0.25
    assert sums.cpu().numpy().tolist() == [0.0, 0.0]            # cleared for the next step
    # without a meter
    sums = torch.tensor([s0, s1], dtype=torch.float64, device=DEV)
    check(lib.mspl_ce_flood_finalize(_p(sums), b, n, _p(out3), None, _stream()))
    assert out3.cpu().numpy()[0] == want[0]


class _Meters(object):
    def __init__(self, K):
        self.classes = K
        self.areas = torch.zeros(3 * K, dtype=torch.int64, device=DEV)
        self.meter = torch.zeros(2, dtype=torch.float64, device=DEV)
        self.sums = torch.zeros(2, dtype=torch.float64, device=DEV)


@pytest.mark.parametrize('with_meters', [True, False])
@pytest.mark.parametrize('b', [0.015, 10.0])
@pytest.mark.parametrize('C,H,W', [(5, 9, 29), (13, 3, 263), (21, 5, 7)])
def test_autograd_node_against_float64(C, H, W, b, with_meters):
    """Loss and d loss / d logits of flood(CrossEntropyLoss) against float64 autograd, on both branches of the flood (b = 10 is above
    every loss here: the value is 2b - ce and the gradient changes sign), with the meters filled by the same launches."""
    from mspl_amd import autograd as ag
    K, ignore, N = C - 1, C - 1, 2
    x, t, cw = _inputs(C, H * W, 6)
    x, t = x.view(N, C, H, W), t.view(N, H, W)
    t = torch.where(t == 255, torch.full_like(t, ignore), t)         # (CrossEntropyLoss takes no other label outside 0..C-1)
    x64 = x.double().requires_grad_()
    ce = F.cross_entropy(x64, t, weight=cw.double(), ignore_index=ignore)
    ref = (ce - b).abs() + b
    ref.backward()
    assert (float(ce.detach()) < b) == (b == 10.0)
    xd = x.to(DEV).requires_grad_()
    meters = _Meters(K) if with_meters else None
    loss = ag.flooded_ce_meters(xd, t.to(DEV), cw.to(DEV), ignore, b, meters)
    (loss * 1.0).backward()
    lerr = abs(float(loss.detach()) - float(ref.detach())) / abs(float(ref.detach()))
    g, g64 = xd.grad.cpu().double(), x64.grad
    rel = float((g - g64).norm() / g64.norm())
    el = float((g - g64).abs().max() / g64.abs().max())
    print('C=%d %dx%d b=%g: loss %.9g against %.9g (%.2e), gradient rel %.2e element %.2e' % (C, H, W, b, float(loss.detach()), float(ref.detach()), lerr, rel, el))
    assert lerr <= LOSS_TAU and rel <= GRAD_TAU_REL and el <= GRAD_TAU_EL
    n0, h0, w0 = [int(v) for v in (t != ignore).nonzero()[0]]
    at_target = float(g[n0, int(t[n0, h0, w0]), h0, w0])             # softmax - 1 < 0 at the label; flipped below the flood level
    assert at_target > 0 if b == 10.0 else at_target < 0
    if with_meters:
        want = reference_areas(torch.max(x, 1)[1].numpy(), t.numpy(), K)
        assert np.array_equal(meters.areas.cpu().numpy().reshape(3, K), want)
        m = meters.meter.cpu().numpy()
        assert m[0] == float(np.float64(np.float32(float(loss.detach()))) * N) and m[1] == 0.0
        assert meters.sums.cpu().numpy().tolist() == [0.0, 0.0]
