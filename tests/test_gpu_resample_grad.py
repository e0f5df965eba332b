"""The backward kernels of the resampling family (mspl_bilinear_bwd in its six forms, mspl_adaptive_avgpool_bwd,
mspl_avgpool3x3s2_bwd in its two, TwoHeadSumFn) on the cases of tests/resample_cases.py; tests/test_resample_cases.py proves on the
CPU that each case reaches the form and seam it is in the table for and that the probe sets are valid.

(a) test_backward_is_the_forward_transposed: one-hot probes read the operator off the forward (its columns) and off the backward
    (its rows), one term per element, so no summation order exists: the two must be EQUAL, bit for bit -- the backward evaluates
    the forward's own weights, and a candidate dropped at a window, tile or thread boundary is a zero where the forward has a
    weight.  Everything a probe plane writes outside its hot elements' receivers must be exactly 0.
    (The tiled and the per-thread bilinear forms are both held to the forward's operator; the product build reaches the per-thread
    form only for shapes the tiles do not take, so the two are never compared on one shape.)
(b) test_dense_against_float64: random data through the C ABI, destinations pre-filled with NaN, per plane
    |kernel - float64| <= 4 * max(err32, 2^-23 * M) (tests/resample_cases.py), and a second call gives the same bits."""
import ctypes

import pytest
import torch

from tests import resample_cases as rc

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAN = float('nan')
LINEAR = [c.id for c in rc.CASES if c.op in rc.LINEAR]
CHUNK = 1 << 24                     # floats of probe gradient per launch


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _sync(what):
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:          # a device fault: nothing more is started on this GPU
        pytest.exit('%s: %s' % (what, e), returncode=3)


def _forward(case, *xs):
    """The operation through mspl_amd.autograd, on (1, planes, H, W) tensors."""
    from mspl_amd import autograd as ag
    s = case.shape
    if case.op == 'bilinear':
        return ag.bilinear(xs[0], tuple(s[3:5]))
    if case.op == 'avgpool':
        return ag.avgpool(xs[0])
    if case.op == 'adaptive':
        return ag.adaptive_avgpool(xs[0], tuple(s[3:5]))
    return ag.two_head_sum(xs[0], xs[1], tuple(s[5:7]))


def _forward_operator(case, k):
    """(Ho*Wo, Hi*Wi): column j = the forward's output for input k one-hot at j (the other input zero).  With more planes than
    basis vectors (the grid-wrap cases) plane p carries vector p % (Hi*Wi) and every repetition must give the same bits."""
    if case.cfg.get('forward_refused'):
        # mspl_bilinear_fwd does not take rows this wide.  Its weights along an axis depend on that axis' two sizes alone, so the
        # forward of the TRANSPOSED shape (Wi x Hi -> Wo x Ho, which it takes) is the same operator with the axes swapped
        pl, Hi, Wi, Ho, Wo = case.shape
        with pytest.raises(RuntimeError, match='do not fit'):
            _forward(case, torch.zeros(1, 1, Hi, Wi, device=DEV))
        At = _forward_operator(rc.Case(case.op, case.id, (pl, Wi, Hi, Wo, Ho), None, case.where, {}), k)
        return At.view(Wo, Ho, Wi, Hi).permute(1, 0, 3, 2).reshape(Ho * Wo, Hi * Wi).contiguous()
    shapes = rc.in_shapes(case)
    Ni = shapes[k][0] * shapes[k][1]
    planes = max(case.shape[0], Ni) if case.shape[0] > 65535 else Ni
    xs = [torch.zeros(1, planes, *hw, device=DEV) for hw in shapes]
    idx = torch.arange(planes, device=DEV)
    xs[k].view(planes, Ni)[idx, idx % Ni] = 1.0
    with torch.no_grad():
        y = _forward(case, *xs).view(planes, -1)
    _sync(case.id)
    if planes > Ni:
        assert torch.equal(y, y[:Ni][idx % Ni]), '%s: the forward differs between planes that carry the same probe' % case.id
    return y[:Ni].t().contiguous()


def _backward_operator(case, k):
    """(Ho*Wo, Hi*Wi): row o = the backward's input gradient k for the output gradient one-hot at o."""
    shapes = rc.in_shapes(case)
    Ho, Wo = rc.out_shape(case)
    Hi, Wi = shapes[k]
    No, Ni = Ho * Wo, Hi * Wi
    A = torch.zeros(No, Ni, device=DEV)
    if case.shape[0] > 65535:           # the full basis, repeated over all planes
        planes = case.shape[0]
        hot = (torch.arange(planes) % No)[:, None]
        owner = hot.expand(planes, Ni)
    else:
        hot, owner = rc.bwd_probes(case.id, k)
    planes = hot.shape[0]
    step = max(1, min(planes, CHUNK // No))
    col = torch.arange(Ni, device=DEV)[None, :]
    seen = torch.zeros(No, Ni, dtype=torch.bool, device=DEV)
    for p0 in range(0, planes, step):
        h, own = hot[p0:p0 + step].to(DEV), owner[p0:p0 + step].to(DEV)
        c = h.shape[0]
        gy = torch.zeros(c, No, device=DEV).scatter_add_(1, h.clamp_min(0), (h >= 0).float())
        if case.cfg.get('forward_refused'):     # no forward, no autograd node: the C ABI
            from mspl_amd._native import check, lib
            gx = torch.full((c, Ni), NAN, device=DEV)
            check(lib.mspl_bilinear_bwd(_p(gy), 1, c, Hi, Wi, Ho, Wo, _p(gx), _stream()))
        else:
            xs = [torch.zeros(1, c, *hw, device=DEV, requires_grad=True) for hw in shapes]
            gx = torch.autograd.grad(_forward(case, *xs), xs, gy.view(1, c, Ho, Wo))[k].view(c, Ni)
        _sync(case.id)
        stray = (own < 0) & (gx != 0)
        assert not bool(stray.any()), '%s: %d elements outside every receiver are not 0 (first: plane %d input %d = %r)' % (
            (case.id, int(stray.sum())) + tuple(torch.nonzero(stray)[0].tolist()) + (float(gx[stray][0]),))
        m = own >= 0
        rows, cols = own[m], col.expand(c, Ni)[m]
        if case.shape[0] > 65535:       # every repetition gives the same bits
            first = gx[:No]
            assert torch.equal(gx, first[torch.arange(c, device=DEV) % No]), '%s: planes with the same probe differ' % case.id
        A[rows, cols] = gx[m]
        seen[rows, cols] = True
    return A, seen


def _describe(case, k, Ab, Af):
    Ho, Wo = rc.out_shape(case)
    Hi, Wi = rc.in_shapes(case)[k]
    bad = torch.nonzero(Ab != Af)
    lines = ['%s input %d (%s; %s): %d operator entries differ between backward and forward' % (case.id, k, rc.plan(case), case.where, len(bad))]
    for o, i in bad[:8].tolist():
        b, f = float(Ab[o, i]), float(Af[o, i])
        ulp = abs(torch.tensor(b).view(torch.int32).item() - torch.tensor(f).view(torch.int32).item()) if b * f > 0 else None
        lines.append('  output (%d, %d) <- input (%d, %d): backward %r forward %r (%s ulp)' % (o // Wo, o % Wo, i // Wi, i % Wi, b, f, ulp))
    return '\n'.join(lines)


@pytest.mark.parametrize('cid', LINEAR)
def test_backward_is_the_forward_transposed(cid):
    case = rc.BY_ID[cid]
    for k in range(len(rc.in_shapes(case))):
        Af = _forward_operator(case, k)
        Ab, seen = _backward_operator(case, k)
        # what no probe could reach is 0 in the forward as well (the receivers are wide enough)
        assert not bool(((~seen) & (Af != 0)).any()), '%s: the forward has weights outside the probes\' receivers' % cid
        A64 = rc.dense_operator(case, k).to(DEV)
        print('%s input %d: %d weights, forward vs float64 %.3g, backward vs float64 %.3g' % (
            cid, k, int((Af != 0).sum()), float((Af.double() - A64).abs().max()), float((Ab.double() - A64).abs().max())))
        assert torch.equal(Ab, Af), _describe(case, k, Ab, Af)
        # ... and they are the operation's weights: the source position o * ratio carries two float32 roundings (2^-23 of a position of
        # up to max(Hi, Wi) pixels), a weight moves by as much; times 2 for the product of two weights and its rounding
        Hi, Wi = rc.in_shapes(case)[k]
        assert float((Af.double() - A64).abs().max()) <= 2.0 ** -22 * max(Hi, Wi, 4)


def _dev(t, misalign=False):
    if not misalign:
        return t.to(DEV, torch.float32).contiguous()
    buf = torch.empty(t.numel() + 1, device=DEV, dtype=torch.float32)
    d = buf[1:].view(t.shape)
    d.copy_(t)
    assert d.data_ptr() % 16 == 4 and d.is_contiguous()
    return d


def _run_dense(case, p):
    from mspl_amd._native import check, lib
    s = case.shape
    gy = _dev(p['gy'], bool(case.cfg.get('misalign')))
    if case.op == 'two_head':
        xs = [_dev(p['x%d' % k]).requires_grad_(True) for k in range(2)]
        g = torch.autograd.grad(_forward(case, *xs), xs, gy)
        return {'gx0': g[0], 'gx1': g[1]}
    gx = torch.full((1, s[0], s[1], s[2]), NAN, device=DEV)
    if case.op == 'bilinear':
        check(lib.mspl_bilinear_bwd(_p(gy), 1, s[0], s[1], s[2], s[3], s[4], _p(gx), _stream()))
    elif case.op == 'adaptive':
        check(lib.mspl_adaptive_avgpool_bwd(_p(gy), 1, s[0], s[1], s[2], s[3], s[4], _p(gx), _stream()))
    else:
        check(lib.mspl_avgpool3x3s2_bwd(_p(gy), 1, s[0], s[1], s[2], _p(gx), _stream()))
    return {'gx0': gx}


def assert_within(cid, got, refs, note=''):
    """Per plane |got - float64| <= the case's bound; prints the worst ratio before it asserts."""
    worst = {}
    for name, r in refs.items():
        g = got[name].detach().cpu().double()
        assert g.shape == r.r64.shape, (cid, name, tuple(g.shape), tuple(r.r64.shape))
        err = rc.plane_max(name, torch.nan_to_num(g - r.r64, nan=float('inf'), posinf=float('inf'), neginf=float('inf')))
        worst[name] = float((err / r.bound.clamp_min(1e-300)).max()) if float(r.mag.max()) > 0 else float(err.max())
    print('%s%s: worst error / bound %s' % (cid, note, {n: '%.3f' % v for n, v in worst.items()}))
    for name, v in worst.items():
        assert v <= 1.0, '%s %s%s: error %.3f x the bound 4 * max(err32, 2^-23 M)' % (cid, name, note, v)


@pytest.mark.parametrize('cid', LINEAR)
def test_dense_against_float64(cid):
    case = rc.BY_ID[cid]
    p = rc.inputs(case)
    got = _run_dense(case, p)
    _sync(cid)
    assert_within(cid, got, rc.refs(cid), ' (%s)' % (rc.plan(case),))
    again = _run_dense(case, p)
    _sync(cid)
    for name in got:
        assert torch.equal(again[name], got[name]), '%s %s: a second call gives other bits' % (cid, name)
