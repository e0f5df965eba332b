"""The one-launch fusion gate (mspl_fusion_gate_conv_fwd / _bwd_weight, autograd.FusionGateConvFn, models.FusionGate) on the GPU, at
the seams of tests/fusion_gate_cases.py.

Integer data: z and gw must EQUAL float64, element for element (every sum is exact in float32 in any order).
Random data: out and, through the node, d rgb, d depth and d w against oracle.net.fusion_gate in float64, per tensor within
MARGIN = 4 units, a unit being the float32 oracle's own error against float64 on the case (the CPU, ATen), floored at one rounding
of the largest value (2**-23 * max|ref|) -- the rule of tests/test_gpu_confident_logits.py.  Each test prints what it measured."""
import ctypes

import pytest
import torch

from oracle import net as onet
from tests import fusion_gate_cases as fc

pytestmark = pytest.mark.gpu
DEV = 'cuda'
MARGIN = 4
GUARD = -777.0
KEY = 'g.conv_1x1.conv.weight'


def _lib():
    from mspl_amd._native import check, lib
    from mspl_amd.ops import _p, _stream
    return check, lib, _p, _stream


def _f(t):
    return t.to(DEV, torch.float32).contiguous()


# ------------------------------------------------------------------ exact, integer data
@pytest.mark.parametrize('name', fc.NAMES)
def test_forward_z_equals_float64(name):
    check, lib, _p, _stream = _lib()
    c, r = fc.BY_NAME[name], fc.integer_problem(name)
    rgb, depth, w = _f(r['rgb']), _f(r['depth']), _f(r['w'])
    z, out = torch.full_like(rgb, GUARD), torch.full_like(rgb, GUARD)
    check(lib.mspl_fusion_gate_conv_fwd(_p(rgb), _p(depth), _p(w), c.N, c.C, c.H * c.W, _p(z), _p(out), _stream()))
    zc = z.cpu().double()
    bad = int((zc != r['z']).sum())
    print('%s: %d of %d z values differ from float64' % (name, bad, zc.numel()))
    assert bad == 0
    # the blend of that exact z, in float64.  Bound: g = 1 / (1 + expf(-z)) within 4 roundings of a value <= 1 (expf, the sum, the
    # quotient, one spare), times |rgb - depth| <= 8; plus three roundings (two products, one sum) of values <= 4
    g = torch.sigmoid(r['z'])
    ref = r['rgb'] * g + r['depth'] * (1 - g)
    err = float((out.cpu().double() - ref).abs().max())
    print('%s: out within %.2e of the float64 blend' % (name, err))
    assert err <= 2.0 ** -23 * (8 * 4 + 4 * 3)
    # inference form (z == NULL): the same output bits
    out2 = torch.full_like(rgb, GUARD)
    check(lib.mspl_fusion_gate_conv_fwd(_p(rgb), _p(depth), _p(w), c.N, c.C, c.H * c.W, None, _p(out2), _stream()))
    assert torch.equal(out, out2)


@pytest.mark.parametrize('accumulate', [0, 1])
@pytest.mark.parametrize('name', fc.NAMES)
def test_weight_gradient_equals_float64(name, accumulate):
    check, lib, _p, _stream = _lib()
    c, r = fc.BY_NAME[name], fc.integer_problem(name)
    rgb, depth, gz = _f(r['rgb']), _f(r['depth']), _f(r['gz'])
    gw = _f(r['gw0'])                                       # accumulate = 0 must overwrite it, accumulate = 1 add to it
    check(lib.mspl_fusion_gate_conv_bwd_weight(_p(gz), _p(rgb), _p(depth), c.N, c.C, c.H * c.W, accumulate, _p(gw), _stream()))
    want = r['gw'] + (r['gw0'] if accumulate else 0)
    bad = int((gw.cpu().double() != want).sum())
    print('%s accumulate=%d: %d of %d gw values differ from float64' % (name, accumulate, bad, want.numel()))
    assert bad == 0


# ------------------------------------------------------------------ random data against float64
def _oracle(rgb, depth, w, gy, dtype):
    rgb, depth, w = [t.to(dtype).clone().requires_grad_(True) for t in (rgb, depth, w)]
    out = onet.fusion_gate(rgb, depth, {KEY: w}, 'g')
    out.backward(gy.to(dtype))
    return [t.detach().double() for t in (out, rgb.grad, depth.grad, w.grad)]


def _check(tag, names, got, ref64, ref32):
    worst = 0.0
    for n, a, r64, r32 in zip(names, got, ref64, ref32):
        unit = max(float((r32 - r64).abs().max()), 2.0 ** -23 * float(r64.abs().max()))
        ratio = float((a.cpu().double() - r64).abs().max()) / unit
        print('%s %s: %.2f units of %.3e (float32 oracle)' % (tag, n, ratio, unit))
        worst = max(worst, ratio)
        assert torch.isfinite(a).all()
    assert worst <= MARGIN


@pytest.mark.parametrize('sinks', [False, True], ids=['autograd', 'sink'])
@pytest.mark.parametrize('name', fc.NAMES)
def test_node_against_float64(name, sinks):
    from mspl_amd import autograd as ag
    rgb, depth, w, gy = fc.random_problem(name)
    ref64 = _oracle(rgb, depth, w, gy, torch.float64)
    ref32 = _oracle(rgb, depth, w, gy, torch.float32)
    a, b, ww = [_f(t).requires_grad_(True) for t in (rgb, depth, w)]
    if sinks:
        ww.grad = torch.zeros_like(ww)
    with ag.grad_sinks(sinks):
        out = ag.fusion_gate_conv(a, b, ww)
        out.backward(_f(gy))
    torch.cuda.synchronize()
    _check(name, ('out', 'd rgb', 'd depth', 'd w'), (out.detach(), a.grad, b.grad, ww.grad), ref64, ref32)


# ------------------------------------------------------------------ decline path and switch
@pytest.mark.parametrize('shape', fc.DECLINED)
def test_declined_shape_launches_nothing(shape):
    check, lib, _p, _stream = _lib()
    from mspl_amd import _native as nv
    N, C, HW = shape
    rgb = torch.randn(N, C, 1, HW, device=DEV)
    w = torch.randn(C, 2 * C, device=DEV)
    z, out, gw = torch.full_like(rgb, GUARD), torch.full_like(rgb, GUARD), torch.full_like(w, GUARD)
    assert lib.mspl_fusion_gate_conv_fwd(_p(rgb), _p(rgb), _p(w), N, C, HW, _p(z), _p(out), _stream()) == nv.ERR_UNSUPPORTED
    assert lib.mspl_fusion_gate_conv_bwd_weight(_p(rgb), _p(rgb), _p(rgb), N, C, HW, 0, _p(gw), _stream()) == nv.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    for t in (z, out, gw):
        assert bool((t == GUARD).all())


def _gate(C, seed):
    from mspl_amd import models
    torch.manual_seed(seed)
    m = models.FusionGate(nchannel=C).to(DEV)
    with torch.no_grad():
        m.conv_1x1.conv.weight.normal_(0, (1.0 / C) ** 0.5)
    return m


class _Spy(object):
    def __init__(self, fn):
        self.fn, self.calls = fn, 0

    def __call__(self, *a):
        self.calls += 1
        return self.fn(*a)


def _run_gate(m, rgb, depth, train):
    if not train:
        with torch.no_grad():
            return m(rgb, depth), None
    for p in m.parameters():
        p.grad = None
    a, b = rgb.clone().requires_grad_(True), depth.clone().requires_grad_(True)
    out = m(a, b)
    out.square().sum().backward()
    return out.detach(), (a.grad, b.grad, m.conv_1x1.conv.weight.grad.clone())


@pytest.mark.parametrize('train', [False, True], ids=['inference', 'training'])
def test_module_takes_todays_path_where_declined(monkeypatch, train):
    """A gate of 48 channels (no multiple of the 32-row tile).  The library declines; FusionGate gives exactly today's result."""
    from mspl_amd import _native as nv, layers
    m = _gate(48, 3)
    rgb, depth = torch.randn(2, 48, 2, 3, device=DEV), torch.randn(2, 48, 2, 3, device=DEV)
    spy = _Spy(nv.lib.mspl_fusion_gate_conv_fwd)
    monkeypatch.setattr(nv.lib, 'mspl_fusion_gate_conv_fwd', spy)
    out, grads = _run_gate(m, rgb, depth, train)
    assert spy.calls == 0
    monkeypatch.setattr(layers, '_FUSED_FUSION_GATE', False)
    out0, grads0 = _run_gate(m, rgb, depth, train)
    assert torch.equal(out, out0)
    if train:
        for a, b in zip(grads, grads0):
            assert torch.equal(a, b)


@pytest.mark.parametrize('train', [False, True], ids=['inference', 'training'])
@pytest.mark.parametrize('C,hw', [(32, (6, 10)), (512, (6, 10)), (512, (2, 3))])
def test_switch_off_never_calls_the_new_launcher(monkeypatch, C, hw, train):
    from mspl_amd import _native as nv, layers
    m = _gate(C, 5)
    rgb, depth = torch.randn(2, C, *hw, device=DEV), torch.randn(2, C, *hw, device=DEV)
    spy = _Spy(nv.lib.mspl_fusion_gate_conv_fwd)
    spyw = _Spy(nv.lib.mspl_fusion_gate_conv_bwd_weight)
    monkeypatch.setattr(nv.lib, 'mspl_fusion_gate_conv_fwd', spy)
    monkeypatch.setattr(nv.lib, 'mspl_fusion_gate_conv_bwd_weight', spyw)
    assert layers._FUSED_FUSION_GATE                    # the default
    out, grads = _run_gate(m, rgb, depth, train)
    assert spy.calls == 1 and spyw.calls == int(train)
    monkeypatch.setattr(layers, '_FUSED_FUSION_GATE', False)
    out0, grads0 = _run_gate(m, rgb, depth, train)
    assert spy.calls == 1 and spyw.calls == int(train)  # not called again
    # the two paths differ in the order of the K sums only
    assert float((out - out0).abs().max()) <= 1e-5 * float(out0.abs().max())
    if train:
        for a, b in zip(grads, grads0):
            assert float((a - b).abs().max()) <= 1e-4 * float(b.abs().max())
