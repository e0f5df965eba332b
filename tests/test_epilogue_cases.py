"""The epilogue case table (tests/epilogue_cases.py) checked without a GPU: it names every entry point that takes an epilogue, its
reference epilogue is epi_apply's order of operations, and every term of every case is visible in the float64 reference -- a term
the inputs cannot show is no test."""
import pytest
import torch
import torch.nn.functional as F

from mspl_amd import _native as nv
from tests import epilogue_cases as ec

CONTRACT = [(op, ci, ts) for op in ec.CONTRACT_OPS for ci in range(len(ec.OPS[op]['cases'])) for ts in ec.termsets(op)]
OTHERS = [(op, ci, ts) for op in ec.OPS if op not in ec.CONTRACT_OPS and op != 'dense_conv_split'
          for ci in range(len(ec.OPS[op]['cases'])) for ts in ec.termsets(op)] + \
    [(op, ci, ts) for op, ci, ts in ec.FALLBACKS if op == 'conv1x1'] + \
    [('conv1x1', ci, ec.ALL) for ci in range(len(ec.OPS['conv1x1']['cases']))] + [('conv1x1', ci, ec.AFFINE) for ci in (0, 1, 3)]


def _id(v):
    op, ci, ts = v
    return '%s-%d-%s' % (op, ci, ec.term_id(ts))


def test_every_entry_point_with_an_epilogue_is_in_the_table():
    with_ep = {name for name, argtypes in nv.SIGNATURES.items() if nv._EP in argtypes}
    assert len(with_ep) >= 16
    in_table = {d['entry'] for d in ec.OPS.values()}
    assert with_ep == in_table, 'state the epilogue contract of %s in tests/epilogue_cases.py' % sorted(with_ep ^ in_table)


@pytest.mark.parametrize('op', sorted(ec.OPS))
def test_contract_is_complete(op):
    """Every term, the slice and raw_out are either accepted or refused, never both or neither; every case names its form."""
    d = ec.OPS[op]
    assert d['accepts'] | d['refuses'] == ec.EVERYTHING and not (d['accepts'] & d['refuses'])
    assert d['cases'] and all(c.form and ':' in c.where for c in d['cases'])
    for ts in ec.termsets(op):
        assert ts <= d['accepts'], '%s is tested with a term it refuses: %s' % (op, ec.term_id(ts))
    if op in ec.CONTRACT_OPS:                     # every accepted operand term alone, and all of them together
        sets = ec.termsets(op)
        acc = frozenset(t for t in ec.TERMS if t in d['accepts'])
        assert acc in sets
        if op != 'pyrpool_fused_train':           # (the training entry point shares its kernels' epilogue code with pyrpool_fused)
            assert all(frozenset((t,)) in sets for t in acc)
    assert (op in ec.RAW_OPS) == ('raw_out' in d['accepts'])
    assert (op in ec.REFUSING_OPS) == bool(d['refuses'])


def test_reference_epilogue_is_the_hand_written_one():
    """In float32 on the CPU the one reference epilogue reproduces, bit for bit, the expected values test_conv1x1_epilogues writes out by
    hand for its reinforcement + channel slice + gate + pre_add block (tests/test_gpu_kernels.py)."""
    N, Cin, Cout, G, H, W = 2, 32, 24, 4, 16, 30
    g = torch.Generator().manual_seed(1)
    rn = lambda *s: torch.randn(*s, generator=g)                                # noqa: E731
    x, w = rn(N, Cin, H, W), rn(Cout, Cin // G, 1, 1) * (Cin // G) ** -0.5
    base = F.conv2d(x, w, None, 1, 0, 1, G)
    ctot, coff = Cout + 5, 3
    r, rw, gate, pre = rn(N, 3, H, W), rn(ctot, 3), torch.sigmoid(rn(N, ctot)), rn(N, ctot, H, W)
    sc, sh, al = rn(ctot).abs() + 0.5, rn(ctot) * 0.1, rn(ctot).abs() * 0.3
    s = slice(coff, coff + Cout)
    v = (base + pre[:, s]) * sc[s].view(1, -1, 1, 1) + sh[s].view(1, -1, 1, 1)
    v = v + torch.einsum('cj,njhw->nchw', rw[s], r)
    v = F.prelu(v, al[s]) * gate[:, s, None, None]
    t = {'scale': sc, 'shift': sh, 'alpha': al, 'pre_add': pre, 'reinf_r': r, 'reinf_w': rw, 'gate': gate}
    got = ec.ref_epilogue(base, t, coff)
    assert got.dtype == torch.float32 and torch.equal(got, v)
    # the residual goes in after the affine step and the reinforcement, before PReLU
    res = rn(N, ctot, H, W)
    u = (base + pre[:, s]) * sc[s].view(1, -1, 1, 1) + sh[s].view(1, -1, 1, 1) + torch.einsum('cj,njhw->nchw', rw[s], r) + res[:, s]
    assert torch.equal(ec.ref_epilogue(base, dict(t, residual=res), coff), F.prelu(u, al[s]) * gate[:, s, None, None])
    # ... and the float64 evaluation of the same float32 operands is the float32 one up to float32 rounding
    torch.testing.assert_close(ec.ref_epilogue(base.double(), t, coff), v.double(), rtol=1e-5, atol=1e-5)


def test_embedding_keeps_absolute_channels():
    t = ec.make_operands(2, 4, 3, 5, ec.ALL, 9)
    big = ec.embed(t, 4, 9, 3)
    acc = torch.randn(2, 4, 3, 5, dtype=torch.float64)
    assert torch.equal(ec.ref_epilogue(acc, big, 3), ec.ref_epilogue(acc, t))
    assert big['scale'].shape == (9,) and big['pre_add'].shape == (2, 9, 3, 5) and big['gate'].shape == (2, 9) and big['reinf_w'].shape == (9, 3)
    assert float(t['scale'].min()) >= 0.5 and float(t['alpha'].max()) <= 0.3


@pytest.mark.parametrize('case', CONTRACT + OTHERS, ids=_id)
def test_every_term_is_visible(case):
    """problem() finds a seed at which each term of the set moves at least half of the float64 outputs by more than 100 x the
    comparison tolerance (it raises otherwise); the reference is finite and of the op's output shape."""
    op, ci, ts = case
    p = ec.problem(op, ci, ts)
    assert set(p.shares) == set(ts) and all(v >= ec.VISIBLE_SHARE for v in p.shares.values()), p.shares
    assert torch.isfinite(p.ref).all() and p.ref.dtype == torch.float64
    for k, v in p.t.items():
        assert v.dtype == torch.float32 and v.is_contiguous()


@pytest.mark.parametrize('op', ec.CONTRACT_OPS)
def test_tolerance_comes_from_the_reference(op):
    """Nothing is fitted to a kernel: torch's own float32 evaluation of each reference (bare and with every term set) stays within a
    quarter of the standing tolerance, so an accumulation order of the kernel's own has room -- or the case records that float32 gap
    (pinned here: not below the computed one, not more than a quarter above it) and is allowed 4 x the gap."""
    for ci, case in enumerate(ec.OPS[op]['cases']):
        gaps = [ec.f32_gap(ec.problem(op, ci, ts)) for ts in [frozenset()] + ec.termsets(op)]
        if case.gap is None:
            assert 4.0 * gaps[0] <= ec.tolerance(op, ci, bare=True)[0] and 4.0 * max(gaps) <= ec.tolerance(op, ci)[0], (case.args, gaps)
        else:
            assert max(gaps) <= case.gap <= 1.25 * max(gaps), (case.args, max(gaps))
            assert ec.tolerance(op, ci)[0] == 4.0 * case.gap
