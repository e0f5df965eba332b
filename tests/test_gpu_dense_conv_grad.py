"""mspl_dense_conv_wgrad / mspl_dense_conv_dgrad (the backward of K13) through the C ABI against torch.nn.functional.conv2d autograd
on the CPU in float64.

Bound per tensor: 4 x the error of the SAME CPU computation in float32 against float64 (max |difference|, computed here) -- the margin
DESIGN section 2 uses for the softmax family against a float32 oracle.  Shapes are the smallest that reach each guard of the kernels.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _problem(N, Cin, Cout, H, W, k, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) * (Cin * k * k) ** -0.5
    gy = torch.randn(N, Cout, H, W, generator=g)
    return x, w, gy


def _cpu_grads(x, w, gy, k, dil, dtype):
    """(gx, gw, gb) of conv2d(x, w, b, padding = dilation) for the cotangent gy, by ATen autograd on the CPU in `dtype`."""
    x, w, gy = x.detach().clone().to(dtype).requires_grad_(True), w.detach().clone().to(dtype).requires_grad_(True), gy.to(dtype)
    b = torch.zeros(w.shape[0], dtype=dtype, requires_grad=True)
    F.conv2d(x, w, b, 1, dil * (k // 2), dil).backward(gy)
    return x.grad, w.grad, b.grad


def _within(name, got, r64, r32):
    """max |got - float64| <= 4 * max |float32 CPU - float64|; prints both figures."""
    err = float((got.double().cpu() - r64).abs().max())
    ref = float((r32.double() - r64).abs().max())
    print('%-28s error %.3e   float32 CPU error %.3e   ratio %.2f' % (name, err, ref, err / ref if ref else float('inf')))
    assert err <= 4.0 * ref, '%s: error %.3e exceeds 4 x the float32 CPU error %.3e' % (name, err, ref)


def _wgrad(gy, x, k, dil, split=0, bias=True):
    """-> (dw as (Cout, Cin, k, k), db) through mspl_dense_conv_wgrad; the workspace is sized by the library's own query."""
    from mspl_amd import ops
    from mspl_amd._native import check, lib
    N, Cin, H, W = x.shape
    Cout = gy.shape[1]
    args = (N, Cin, Cout, H, W, k, dil, split)
    nbytes = int(lib.mspl_dense_conv_wgrad_workspace_bytes(*args))
    assert nbytes >= 0
    ws = torch.empty(nbytes // 4, device=DEV) if nbytes else None
    dw = torch.full((k * k, Cout, Cin), float('nan'), device=DEV)
    db = torch.full((Cout,), float('nan'), device=DEV) if bias else None
    check(lib.mspl_dense_conv_wgrad(_p(gy), _p(x), *args, _p(ws), nbytes, _p(dw), _p(db), _stream()))
    return ops.unpack_dense_weight(dw, k), db


def _dgrad(gys, ws, ks, dils, Cx, out=None):
    """-> gx through mspl_dense_conv_dgrad on ops.pack_dense_weight_dgrad packs."""
    from mspl_amd import ops
    from mspl_amd._native import check, lib
    n = len(gys)
    wts = [ops.pack_dense_weight_dgrad(w) for w in ws]
    N, Cg, H, W = gys[0].shape
    gx = torch.full((N, Cx, H, W), float('nan'), device=DEV) if out is None else out
    arr = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])          # noqa: E731
    ints = lambda vs: (ctypes.c_int32 * n)(*vs)                                    # noqa: E731
    check(lib.mspl_dense_conv_dgrad(arr(gys), arr(wts), ints(ks), ints(dils), n, N, Cg, Cx, H, W, int(out is not None), _p(gx), _stream()))
    return gx


@pytest.mark.parametrize('shape', [(3, 64, 48, 7, 9, 3, 2),        # 189 pixels: no tile multiple; Cout below one tile, not a multiple of 32
                                   (1, 32, 130, 9, 8, 1, 1),       # 1x1, Cout one row past a tile
                                   (2, 96, 256, 5, 6, 3, 6)])      # Cin = 96: half a column tile is masked; only the centre tap lives
def test_wgrad_shapes(shape):
    N, Cin, Cout, H, W, k, dil = shape
    x, w, gy = _problem(N, Cin, Cout, H, W, k, 11)
    _, w64, b64 = _cpu_grads(x, w, gy, k, dil, torch.float64)
    _, w32, b32 = _cpu_grads(x, w, gy, k, dil, torch.float32)
    dw, db = _wgrad(gy.to(DEV), x.to(DEV), k, dil)
    _within('dw %s' % (shape,), dw, w64, w32)
    _within('db %s' % (shape,), db, b64, b32)
    if dil >= H and dil >= W:
        off = [t for t in range(9) if t != 4]
        flat = dw.reshape(Cout, Cin, 9).cpu()
        assert torch.all(flat[:, :, off] == 0.0) and not torch.any(torch.signbit(flat[:, :, off])), 'dead taps must be exactly +0.0'
        assert float(w64.reshape(Cout, Cin, 9)[:, :, off].abs().max()) == 0.0
    dw2, _ = _wgrad(gy.to(DEV), x.to(DEV), k, dil, bias=False)       # without the bias gradient: the same weight gradient
    assert torch.equal(dw2, dw)


def test_dgrad_through_transposed_pack():
    N, Cin, Cout, H, W, k, dil = 2, 96, 256, 5, 6, 3, 6
    x, w, gy = _problem(N, Cin, Cout, H, W, k, 12)
    x64, _, _ = _cpu_grads(x, w, gy, k, dil, torch.float64)
    x32, _, _ = _cpu_grads(x, w, gy, k, dil, torch.float32)
    gx = _dgrad([gy.to(DEV)], [w.to(DEV)], [k], [dil], Cin)
    _within('gx centre tap only', gx, x64, x32)
    # the same into an existing tensor: accumulate adds
    base = torch.randn(N, Cin, H, W, generator=torch.Generator().manual_seed(5))
    acc = _dgrad([gy.to(DEV)], [w.to(DEV)], [k], [dil], Cin, out=base.to(DEV))
    assert torch.equal(acc.cpu(), gx.cpu() + base)


def test_wgrad_split_paths_agree_and_repeat_bitwise():
    N, Cin, Cout, H, W, k, dil = 4, 32, 32, 40, 40, 3, 3
    x, w, gy = _problem(N, Cin, Cout, H, W, k, 13)
    _, w64, b64 = _cpu_grads(x, w, gy, k, dil, torch.float64)
    _, w32, b32 = _cpu_grads(x, w, gy, k, dil, torch.float32)
    xd, gd = x.to(DEV), gy.to(DEV)
    for split in (1, 2, 5, 0):                 # 200 pixel chunks: 5 divides them, 0 is the library's own choice
        dw, db = _wgrad(gd, xd, k, dil, split)
        _within('dw split %d' % split, dw, w64, w32)
        _within('db split %d' % split, db, b64, b32)
        dw2, db2 = _wgrad(gd, xd, k, dil, split)
        assert torch.equal(dw, dw2) and torch.equal(db, db2), 'split %d is not bit-identical from run to run' % split
    dw3, _ = _wgrad(gd, xd, k, dil, 3)        # 200 chunks in 3 ranges: a split that does not divide them
    _within('dw split 3', dw3, w64, w32)
    gx = _dgrad([gd], [w.to(DEV)], [k], [dil], Cin)
    x64, _, _ = _cpu_grads(x, w, gy, k, dil, torch.float64)
    x32, _, _ = _cpu_grads(x, w, gy, k, dil, torch.float32)
    _within('gx 40x40 dil 3', gx, x64, x32)


def test_dgrad_four_branches_into_one_gx():
    N, Cin, Cout, H, W = 2, 64, 32, 11, 13
    specs = [(1, 1), (3, 1), (3, 2), (3, 3)]
    x = None
    ws, gys, s64, s32 = [], [], 0, 0
    for i, (k, dil) in enumerate(specs):
        x, w, gy = _problem(N, Cin, Cout, H, W, k, 20 + i)
        ws.append(w)
        gys.append(gy)
        s64 = s64 + _cpu_grads(x, w, gy, k, dil, torch.float64)[0]
        s32 = s32 + _cpu_grads(x, w, gy, k, dil, torch.float32)[0]
    gx = _dgrad([g.to(DEV) for g in gys], [w.to(DEV) for w in ws], [k for k, _ in specs], [d for _, d in specs], Cin)
    _within('gx of four branches', gx, s64, s32)


def test_unsupported_shapes_launch_nothing():
    from mspl_amd import _native
    from mspl_amd._native import lib
    N, H, W = 1, 4, 5
    gy, x = torch.zeros(N, 32, H, W, device=DEV), torch.zeros(N, 48, H, W, device=DEV)
    dw = torch.full((1, 32, 48), 7.0, device=DEV)
    db = torch.full((32,), 7.0, device=DEV)
    assert lib.mspl_dense_conv_wgrad_workspace_bytes(N, 48, 32, H, W, 1, 1, 0) == _native.ERR_UNSUPPORTED
    assert lib.mspl_dense_conv_wgrad(_p(gy), _p(x), N, 48, 32, H, W, 1, 1, 0, None, 0, _p(dw), _p(db), _stream()) == _native.ERR_UNSUPPORTED
    assert lib.mspl_dense_conv_wgrad(_p(gy), _p(x), N, 32, 32, H, W, 5, 1, 0, None, 0, _p(dw), _p(db), _stream()) == _native.ERR_UNSUPPORTED
    # data gradient of a convolution with Cout = 48
    g48 = torch.zeros(N, 48, H, W, device=DEV)
    wt = torch.zeros(1, 32, 48, device=DEV)
    gx = torch.full((N, 32, H, W), 7.0, device=DEV)
    one = (ctypes.c_int32 * 1)(1)
    rc = lib.mspl_dense_conv_dgrad((ctypes.c_void_p * 1)(g48.data_ptr()), (ctypes.c_void_p * 1)(wt.data_ptr()), one, one, 1, N, 48, 32, H, W, 0,
                                   _p(gx), _stream())
    assert rc == _native.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.all(dw == 7.0) and torch.all(db == 7.0) and torch.all(gx == 7.0)


def test_forward_is_undisturbed_by_the_backward_entries():
    """mspl_dense_conv_fwd before and after the new entry points ran: the same bits (the data gradient shares K13's kernels)."""
    from mspl_amd import ops
    N, Cin, Cout, H, W, k, dil = 2, 64, 160, 9, 11, 3, 2
    x, w, gy = _problem(N, Cin, Cout, H, W, k, 14)
    xd, wp = x.to(DEV), ops.pack_dense_weight(w.to(DEV))
    ep = ops.Epi(torch.rand(Cout, device=DEV) + 0.5, torch.randn(Cout, device=DEV), torch.zeros(Cout, device=DEV))
    before = ops.dense_conv(xd, wp, k, dil, ep).clone()
    _wgrad(gy.to(DEV), xd, k, dil, 2)
    _dgrad([gy.to(DEV)], [w.to(DEV)], [k], [dil], Cin)
    after = ops.dense_conv(xd, wp, k, dil, ep)
    assert torch.equal(before, after)
    ref = F.relu(F.conv2d(x.double(), w.double(), None, 1, dil, dil) * ep.scale.cpu().double().view(1, -1, 1, 1) + ep.shift.cpu().double().view(1, -1, 1, 1))
    torch.testing.assert_close(after.cpu().double(), ref, rtol=1e-4, atol=2e-4)
