"""mspl_dense_conv_split_fwd (K13 in split-bf16 arithmetic) through the C ABI against the CPU oracles of tests/split_cases.py.

Structure: the kernel against the float64 emulation of the SAME plane products, within MARGIN x E32, where E32 is the maximum error of
torch's CPU float32 conv2d against the float64 convolution on that case -- a yardstick the kernel has no part in.  A wrong lane or k
mapping gives O(1) errors and a dropped cross term about 2^-9 of the result: both >= 1000 x E32.
MARGIN: the project's standing 4 x for an fp32 accumulation order.  The plane products are exact in fp32, so what differs from the
emulation is summation alone -- the bf16 matrix instruction's own sum of its 16 products, and the 3 (bf16x3) or 6 (bf16x6)
instruction results per k-step that go through one fp32 accumulator.  Measured |kernel - emulation| / E32 per shape (bf16x3,
bf16x6), in SHAPES order: 1.29 2.62 | 0.52 1.06 | 1.16 1.62 | 2.29 2.70 | 0.95 1.25.
Accuracy: the same output against the float64 convolution of the unsplit operands, within C_SPLIT[planes] * conv(|x|, |w|) + 4 x E32.
"""
import ctypes

import pytest
import torch

from tests.split_cases import BATCH_SHAPE, C_SPLIT, PLANES, SHAPES, reference

pytestmark = pytest.mark.gpu
DEV = 'cuda'
MARGIN = 4.0


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _epilogue(ctot, coff, scale=None, shift=None, alpha=None):
    from mspl_amd._native import Epilogue
    s = Epilogue()
    s.struct_size = ctypes.sizeof(Epilogue)
    s.out_ctot, s.out_coff = ctot, coff
    s.scale, s.shift, s.alpha = [None if t is None else t.data_ptr() for t in (scale, shift, alpha)]
    return s


def _run(x, pack, shape, planes, ep=None, out=None):
    """One call of the C entry point; x and pack on the device.  Returns (status, destination)."""
    from mspl_amd._native import lib
    N, Cin, Cout, H, W, k, d = shape
    dst = torch.full((N, Cout, H, W), float('nan'), device=DEV) if out is None else out
    rc = lib.mspl_dense_conv_split_fwd(_p(x), _p(pack), N, Cin, Cout, H, W, k, d, planes, None if ep is None else ctypes.byref(ep), _p(dst),
                                       _stream())
    return rc, dst


@pytest.fixture(scope='module')
def device_case():
    """index, planes -> (reference dict, x on the device, split pack on the device, bare kernel output); built once per module."""
    from mspl_amd import ops
    cache = {}

    def get(index, planes):
        if (index, planes) not in cache:
            ref = reference(index)
            x = ref['x'].to(DEV)
            pack = ops.pack_dense_weight_split(ref['w'], planes).to(DEV)
            rc, y = _run(x, pack, ref['shape'], planes)
            assert rc == 0
            cache[(index, planes)] = (ref, x, pack, y)
        return cache[(index, planes)]
    return get


@pytest.mark.parametrize('planes', PLANES)
@pytest.mark.parametrize('index', range(len(SHAPES)))
def test_structure_and_accuracy(index, planes, device_case):
    ref, x, pack, y = device_case(index, planes)
    got = y.double().cpu()
    assert torch.isfinite(got).all()
    err_s = float((got - ref['emu'][planes]).abs().max())
    print('%s planes %d: |kernel - emulation| %.3e, E32 %.3e, ratio %.2f' % (ref['shape'], planes, err_s, ref['e32'], err_s / ref['e32']))
    err_a = (got - ref['true']).abs()
    allow = C_SPLIT[planes] * ref['mag'] + 4.0 * ref['e32']
    print('%s planes %d: |kernel - float64| %.3e, worst fraction of the allowance %.3f' % (ref['shape'], planes, float(err_a.max()),
                                                                                          float((err_a / allow).max())))
    assert err_s <= MARGIN * ref['e32']
    assert torch.all(err_a <= allow)


@pytest.mark.parametrize('planes', PLANES)
@pytest.mark.parametrize('index', range(len(SHAPES)))
def test_epilogue_and_channel_slice(index, planes, device_case):
    ref, x, pack, _ = device_case(index, planes)
    N, Cin, Cout, H, W, k, d = ref['shape']
    g = torch.Generator().manual_seed(7 + index)
    sc, sh = torch.rand(Cout + 7, generator=g) + 0.5, torch.randn(Cout + 7, generator=g) * 0.1
    scd, shd, zero = sc.to(DEV), sh.to(DEV), torch.zeros(Cout + 7, device=DEV)
    dst = torch.full((N, Cout + 7, H, W), -3.0, device=DEV)
    rc, _ = _run(x, pack, ref['shape'], planes, _epilogue(Cout + 7, 3, scd, shd, zero), out=dst)
    assert rc == 0
    s64, b64 = sc[3:3 + Cout].double().view(1, -1, 1, 1), sh[3:3 + Cout].double().view(1, -1, 1, 1)
    want = torch.relu(ref['emu'][planes] * s64 + b64)
    err = (dst[:, 3:3 + Cout].double().cpu() - want).abs()
    tol = (MARGIN * ref['e32'] * s64.abs()).expand_as(err)          # the structure tolerance scaled by |scale|
    print('%s planes %d: epilogue error %.3e, worst fraction of the tolerance %.3f' % (ref['shape'], planes, float(err.max()),
                                                                                      float((err / tol).max())))
    assert torch.all(err <= tol)
    assert torch.all(dst[:, :3] == -3.0) and torch.all(dst[:, 3 + Cout:] == -3.0)


@pytest.mark.parametrize('planes', PLANES)
def test_batch_independence_and_repeatability(planes, device_case):
    index = SHAPES.index(BATCH_SHAPE)
    ref, x, pack, y = device_case(index, planes)
    N, Cin, Cout, H, W, k, d = ref['shape']
    rc, again = _run(x, pack, ref['shape'], planes)
    assert rc == 0 and torch.equal(again, y)
    for i in range(N):
        rc, one = _run(x[i:i + 1].contiguous(), pack, (1,) + tuple(ref['shape'][1:]), planes)
        assert rc == 0 and torch.equal(one[0], y[i]), 'image %d alone differs from image %d of the batch' % (i, i)


def test_pack_layout_matches_pack_dense_weight():
    from mspl_amd import ops
    from tests.split_cases import split_planes
    w = reference(0)['w']
    for planes in PLANES:
        pk = ops.pack_dense_weight_split(w.to(DEV), planes)
        for p, plane in enumerate(split_planes(w, planes)):
            assert torch.equal(pk[p].float(), ops.pack_dense_weight(plane.to(DEV)))


def test_refusals():
    """Everything the kernel does not take is refused on the host, with nothing launched."""
    from mspl_amd import _native, ops
    from mspl_amd._native import lib
    x = torch.zeros(1, 64, 6, 6, device=DEV)
    out = torch.full((1, 16, 6, 6), -3.0, device=DEV)
    buf = torch.zeros(3 * 25 * 16 * 64 + 8, device=DEV, dtype=torch.bfloat16)
    S = _stream()
    assert lib.mspl_dense_conv_split_fits(32, 16, 3, 2) == 1 and lib.mspl_dense_conv_split_fits(32, 16, 1, 3) == 1
    for Cin, k, planes in [(48, 3, 2), (32, 5, 2), (32, 3, 1), (32, 3, 4)]:
        assert lib.mspl_dense_conv_split_fits(Cin, 16, k, planes) == 0
        rc = lib.mspl_dense_conv_split_fwd(_p(x), _p(buf), 1, Cin, 16, 6, 6, k, 1, planes, None, _p(out), S)
        assert rc == _native.ERR_UNSUPPORTED
    off = ctypes.c_void_p(buf.data_ptr() + 2)          # a pack offset by one bf16 element
    assert lib.mspl_dense_conv_split_fwd(_p(x), off, 1, 32, 16, 6, 6, 3, 1, 2, None, _p(out), S) == _native.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.all(out == -3.0)
    with pytest.raises(RuntimeError, match='does not match'):
        ops.dense_conv_split(x, buf[:2 * 9 * 16 * 32].view(2, 9, 16, 32), 3)
    with pytest.raises(RuntimeError, match='bfloat16'):
        ops.dense_conv_split(x, torch.zeros(2, 9, 16, 64, device=DEV), 3)
