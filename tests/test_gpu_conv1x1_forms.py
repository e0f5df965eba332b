"""mspl_conv1x1_fwd in every kernel form at its K / M / pixel seams (tests/conv1x1_cases.py; tests/test_conv1x1_cases.py proves from
the library's plan query which form and variant each case reaches, and that the data are exact) against float64.

Integer data: the destination, raw_out included, must EQUAL the float64 reference cast to float32 -- bare, and with every term set
the case lists; the channels of a wider destination the call does not write, and the floats around a displaced destination, keep
their sentinel.  A refused case raises and writes nothing.  One random-data pass per form at the standing tolerance of
tests/epilogue_cases.py (tests/test_conv1x1_cases.py shows that torch's own float32 evaluation stays within a quarter of it)."""
import pytest
import torch
import torch.nn.functional as F

from tests import conv1x1_cases as cc
from tests import epilogue_cases as ec

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _dev(t, off=0):
    """float32 copy on the device; off: the tensor starts one float into its allocation (4 bytes off a 16-byte boundary)."""
    t = t.float()
    if not off:
        d = t.to(DEV)
        assert d.data_ptr() % 16 == 0
        return d
    buf = torch.zeros(t.numel() + 1, device=DEV)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def _destination(case):
    """(the flat allocation, the destination view in it), all sentinel."""
    N, Cin, Cout, G, H, W = case.shape
    ctot = case.ctot or Cout
    n = N * ctot * H * W
    flat = torch.full((n + 8,), cc.SENTINEL, device=DEV)
    lo = 4 + case.out_off
    dst = flat[lo:lo + n].view(N, ctot, H, W)
    assert dst.data_ptr() % 16 == (4 if case.out_off else 0) and dst.is_contiguous()
    return flat, dst, lo, n


def _epi(case, terms, t_dev, raw):
    from mspl_amd.ops import Epi
    kw = {k: v for k, v in cc.select(t_dev, terms).items()}
    return Epi(raw_out=raw, **kw)


def _operands_dev(case, t):
    off = lambda k: case.op_off if k in ('pre_add', 'residual', 'reinf_r') else 0      # noqa: E731
    return {k: _dev(v, off(k)) for k, v in t.items()}


@pytest.mark.parametrize('name', cc.NAMES)
def test_equals_float64(name):
    from mspl_amd import ops
    case = cc.BY_NAME[name]
    N, Cin, Cout, G, H, W = case.shape
    x64, w64 = cc.inputs(name)
    x, w = _dev(x64, case.x_off), _dev(w64, case.w_off)
    t_dev = _operands_dev(case, cc.operands(name))
    acc = None if case.refused is not None else cc.accumulate(case)
    for ts in (frozenset(),) + case.termsets + case.leaves:
        flat, dst, lo, n = _destination(case)
        raw = torch.full((N, Cout, H, W), cc.SENTINEL, device=DEV) if 'raw_out' in ts else None
        ep = _epi(case, ts, t_dev, raw) if ts else None
        what = '%s %s' % (name, ec.term_id(ts) + ('+raw_out' if raw is not None else ''))
        if case.refused is not None:
            with pytest.raises(RuntimeError, match=r'mspl_hip \(%d\)' % case.refused):
                ops.conv1x1(x, w, G, ep, out=(dst, case.coff))
            torch.cuda.synchronize()
            assert bool((flat == cc.SENTINEL).all()), '%s: a refused call wrote to its destination' % what
            continue
        ops.conv1x1(x, w, G, ep, out=(dst, case.coff))
        want = cc.reference(case, acc, ts).float()
        got = dst[:, case.coff:case.coff + Cout].cpu()
        bad = int((got != want).sum())
        assert torch.equal(got, want), '%s: %d of %d outputs differ from float64 (first at %s)' % (
            what, bad, want.numel(), tuple(int(v) for v in (got != want).nonzero()[0]))
        rest = flat.clone()
        rest[lo:lo + n].view(N, -1, H, W)[:, case.coff:case.coff + Cout] = cc.SENTINEL
        assert bool((rest == cc.SENTINEL).all()), '%s: wrote outside its channel slice' % what
        if raw is not None:
            assert torch.equal(raw.cpu(), acc.float()), '%s: raw_out differs from the bare float64 convolution' % what


@pytest.mark.parametrize('name', cc.RANDOM)
def test_random_data_within_the_standing_tolerance(name):
    from mspl_amd import ops
    case = cc.BY_NAME[name]
    N, Cin, Cout, G, H, W = case.shape
    form = cc.plan(case)['form']
    for ts in (frozenset(), ec.AFFINE, ec.ALL):
        if cc.plan(case, ts)['form'] != form:              # (split-K with every term: the other forms' pass covers that kernel)
            continue
        inp, t = cc.random_problem(name, ts)
        ref = ec.ref_epilogue(F.conv2d(inp['x'].double(), inp['w'].double(), None, 1, 0, 1, G), t)
        ep = ops.Epi(**{k: v.to(DEV) for k, v in t.items()}) if ts else None
        got = ops.conv1x1(inp['x'].to(DEV), inp['w'].to(DEV), G, ep).cpu().double()
        err = (got - ref).abs()
        print('%s %s %s: max error against float64 %.3e' % (name, form, ec.term_id(ts), float(err.max())))
        assert bool((err <= ec.ATOL + ec.RTOL * ref.abs()).all()), '%s %s: max error %.3e' % (name, ec.term_id(ts), float(err.max()))
