"""The table of tests/conv1x1_cases.py, checked without a GPU: (a) the loop invariants of every kernel form over a dense sweep of
shapes, read from the library's plan query alone (mspl_conv1x1_fwd_plan: the host function the launcher itself switches on);
(b) every case reaches the form and variant it is in the table for, and the table as a whole reaches every form and instantiation;
(c) every 1x1 convolution the segmentation networks send through ops.conv1x1 is in the table; (d) the data are exact: the bound of
tests/exact_cases.py holds and float32 equals float64 on the CPU.  A case whose property is not met FAILS."""
import argparse
import ctypes
import itertools
import re

import pytest
import torch
import torch.nn as nn

from mspl_amd import _native as nv
from mspl_amd import ops
from tests import conv1x1_cases as cc
from tests import epilogue_cases as ec

PIPE_NG = {2, 3, 4, 6, 8, 12, 16, 32, 64}


def _code(err):
    return int(re.search(r'mspl_hip \((-?\d+)\)', str(err.value)).group(1))


@pytest.mark.parametrize('name', cc.NAMES)
def test_case_reaches_its_form(name):
    case = cc.BY_NAME[name]
    if case.refused is not None:
        for ts in (frozenset(),) + case.termsets:
            with pytest.raises(RuntimeError) as err:
                cc.plan(case, ts)
            assert _code(err) == case.refused, name
        return
    p = cc.plan(case)
    got = {k: p[k] for k in case.expect}
    assert got == case.expect, '%s (%s): the library plans %s' % (name, case.why, p)
    for ts in case.termsets:
        q = cc.plan(case, ts)
        assert q['form'] == p['form'], '%s with %s: %s' % (name, ec.term_id(ts), q)
        if not (case.op_off and ts & cc.OPERAND_TERMS):
            assert q == p, 'operands that are aligned change nothing'
    for ts in case.leaves:
        assert cc.plan(case, ts)['form'] != p['form'], '%s with %s stays on %s' % (name, ec.term_id(ts), p['form'])
    if case.ctot:
        assert not any('raw_out' in ts for ts in case.termsets), 'raw_out is for un-sliced destinations'
        assert 0 < case.coff and case.coff + case.shape[2] < case.ctot, 'channels on both sides of the slice'
    assert case.shape[0] >= 2, 'a read into the next image must be visible'


def test_misalignment_is_what_moves_the_misaligned_cases():
    """Each displaced pointer changes the plan against the same call with aligned pointers: nothing falls back by accident."""
    moved = 0
    for case in cc.CASES:
        if not (case.x_off or case.w_off or case.out_off or case.op_off) or case.refused is not None:
            continue
        aligned = case._replace(x_off=0, w_off=0, out_off=0, op_off=0)
        sets = (frozenset(),) + case.termsets + case.leaves
        assert any(cc.plan(case, ts) != cc.plan(aligned, ts) for ts in sets), case.name
        moved += 1
    assert moved >= 6
    both = cc.BY_NAME['pipe_operand_misaligned']
    assert cc.plan(both)['nsub'] == 2 and cc.plan(both, ec.ALL)['nsub'] == 1 and cc.plan(both, ec.AFFINE)['nsub'] == 2
    thin = cc.BY_NAME['thin_operand_misaligned']
    assert cc.plan(thin, ec.AFFINE | {'residual'})['form'] == 'small_k'
    assert cc.plan(thin._replace(op_off=0), ec.AFFINE | {'residual'})['form'] == 'thin'
    # raw_out and gate are looked at by the thin form alone
    shape = (50, 64, 8, 8, 4)
    assert ops.conv1x1_plan(shape, terms=('raw_out',), side_align=8)['form'] == 'small_k'
    assert ops.conv1x1_plan(shape, terms=('raw_out',), side_align=16)['form'] == 'thin'
    assert ops.conv1x1_plan((2, 64, 24, 2, 42), terms=('gate',), side_align=4) == ops.conv1x1_plan((2, 64, 24, 2, 42), terms=('gate',))


def test_table_reaches_every_form_and_instantiation():
    plans = {}
    for c in cc.CASES:
        if c.refused is None:
            for ts in (frozenset(),) + c.termsets + c.leaves:
                plans[(c.name, ts)] = cc.plan(c, ts)
    by = lambda form: [p for p in plans.values() if p['form'] == form]         # noqa: E731
    # the register-weights form is behind a tuning variable (pipe_shape is always true): no case, and no plan ever names it
    assert {p['form'] for p in plans.values()} == {'thin', 'small_k', 'split_k', 'pipe', 'ring'}
    assert {p['mt'] for p in by('thin')} == {8, 16}
    assert {p['mt'] for p in by('small_k')} == {2, 4, 8} and any(p['mtiles'] > 1 for p in by('small_k'))
    assert {(p['nsub'], p['ch']) for p in by('split_k')} == {(1, 8), (1, 16), (2, 8), (2, 16)}
    assert {(p['nsub'], p['ng']) for p in by('pipe')} == {(ns, ng) for ns in (1, 2) for ng in PIPE_NG}
    assert {p['mb'] for p in by('pipe')} == {32, 64, 128} and {p['wm'] for p in by('pipe')} == {1, 2, 4}
    assert any(p['tpw'] > 1 for p in by('pipe')) and any(p['tpw'] > 1 for p in by('ring'))
    assert {p['nsub'] for p in by('ring')} == {1, 2, 4} and {p['vecw'] for p in by('ring')} == {0, 1}
    assert {p['mb'] for p in by('ring')} == {32, 64, 96, 128} and {p['ring'] for p in by('ring')} == {4}
    assert any(p['lds_bytes'] > 64 * 1024 for p in by('ring')), 'a launch that needs the raised dynamic-LDS limit'
    assert any(p['grid_z'] > 1 for p in by('small_k'))
    assert {c.refused for c in cc.CASES} == {None, nv.ERR_UNSUPPORTED}
    # the seams the table is there for
    sk = {c.shape[1] for c in cc.CASES if c.expect and c.expect.get('form') == 'split_k'}
    assert sk >= {64, 128, 192, 256, 320, 384, 512, 640}
    not_sk = {c.shape[1] for c in cc.CASES if c.name.startswith('sk_not_')}
    assert not_sk >= {96, 160, 224}
    assert {c.shape[4] * c.shape[5] for c in cc.CASES if c.name.startswith('sk_')} >= {1, 31, 32, 33, 77}
    assert {c.shape[4] * c.shape[5] % 4 for c in cc.CASES if c.name.startswith('small_')} >= {0, 1, 3}
    assert set(cc.RANDOM) <= set(cc.NAMES) and {cc.plan(cc.BY_NAME[n])['form'] for n in cc.RANDOM} == {'thin', 'small_k', 'split_k', 'pipe', 'ring'}


def test_epilogue_table_rows_reach_the_forms_they_name():
    """The conv1x1 rows of tests/epilogue_cases.py (raw_out and the split-K fall-back are tested on them) name a form: the plan's."""
    rows = ec.OPS['conv1x1']['cases']
    assert len(rows) == len(ec.CONV1X1_PLAN_FORMS)
    for row, form in zip(rows, ec.CONV1X1_PLAN_FORMS):
        N, Cin, Cout, G, H, W = row.args
        assert ops.conv1x1_plan((N, Cin, Cout, G, H * W))['form'] == form, row
        assert ops.conv1x1_plan((N, Cin, Cout, G, H * W), terms=sorted(ec.AFFINE | {'raw_out'}))['form'] == form, row
    for op, ci, lean in ec.FALLBACKS:
        if op == 'conv1x1':
            N, Cin, Cout, G, H, W = rows[ci].args
            assert ec.CONV1X1_PLAN_FORMS[ci] == 'split_k' and lean == ec.AFFINE
            for extra in ('pre_add', 'residual', 'reinf', 'gate'):
                assert ops.conv1x1_plan((N, Cin, Cout, G, H * W), terms=sorted(lean | {extra}))['form'] == 'pipe', extra


# ------------------------------------------------------------------------------------------------------------------ the sweep
SWEEP_M = (1, 8, 16, 17, 32, 33, 64, 128, 129)
SWEEP_MAPS = ((2, 35), (2, 48), (2, 4066), (3, 34560), (2, 32737))             # (N, HW): N * HW * 4096 channels stays below 2^32 bytes


def _expected_refusal(K, M, G):
    """The launcher's refusals on the sweep's range, from its documented rules (no map of the sweep reaches a grid or byte limit):
    an odd K whose weights do not fit 48 KiB; a K beyond the tile-pipelined instantiations whose 32-row weight tile, padded to 32
    columns plus one, exceeds 96 KiB -- unless split-K takes the shape (decided by the caller)."""
    if (K < 16 or K % 2) and G * M * K * 4 <= 48 * 1024:
        return 0
    if K % 2:
        return nv.ERR_UNSUPPORTED
    if K % 8 == 0 and K // 8 in (PIPE_NG - {32, 64}):
        return 0
    if K in (256, 512) and M <= 32 and (min(M, 32) * (K + 1) + 192) * 4 <= 64 * 1024:
        return 0
    return nv.ERR_UNSUPPORTED if 32 * ((K + 31) // 32 * 32 + 1 + 6) * 4 > 96 * 1024 else 0


def _sweep_check(K, M, G, N, HW, terms, out):
    """One shape of the sweep: plan it and assert its form's invariants."""
    f = nv
    rc = nv.lib.mspl_conv1x1_fwd_plan(N, K * G, M * G, G, HW, 0, terms, 16, 16, 16, 16, 16, out)
    where = (K, M, G, N, HW, terms)
    lean = not terms & (f.PW_TERM_PRE_ADD | f.PW_TERM_RESIDUAL | f.PW_TERM_REINF | f.PW_TERM_GATE)
    if rc != 0:
        splitk = M <= 32 and G == 1 and K % 64 == 0 and K >= 4 * M and lean and N * -(-HW // 32) <= 6000
        assert not splitk and rc == _expected_refusal(K, M, G), where
        assert all(v == 0 for v in out), where
        return 'refused'
    form = out[f.PW_PLAN_FORM]
    lds, gx, gy, gz = out[f.PW_PLAN_LDS_BYTES], out[f.PW_PLAN_GRID_X], out[f.PW_PLAN_GRID_Y], out[f.PW_PLAN_GRID_Z]
    assert 1 <= gx < 2 ** 31 and 1 <= gy <= 65535 and 1 <= gz <= 65535, where
    nsub, mb, tpw = out[f.PW_PLAN_NSUB], out[f.PW_PLAN_MB], out[f.PW_PLAN_TPW]
    if form == f.PW_FORM_SPLIT_K:
        ks, ch, tiles = out[f.PW_PLAN_KS], out[f.PW_PLAN_CH], out[f.PW_PLAN_TILES]
        assert ks * 4 == K and ch in (8, 16) and ks % (2 * ch) == 0, where       # the k-loop steps by 2*CH and has no tail
        assert M <= 32 and G == 1 and K >= 4 * M and lean and nsub in (1, 2), where
        assert tiles == -(-HW // (32 * nsub)) and gx == N * G * tiles and lds == 0, where
    elif form == f.PW_FORM_TILE_PIPELINED:
        ng, ar = out[f.PW_PLAN_NG], out[f.PW_PLAN_AR]
        assert K == 8 * ng and ng in PIPE_NG and nsub in (1, 2) and HW % nsub == 0, where
        assert mb in (32, 64, 128) and 1 <= ar <= mb and ar == min(M, mb) and out[f.PW_PLAN_VECW] == 1, where
        assert lds == 4 * (6 * mb + ar * (K | 1)) and lds <= 96 * 1024, where
        assert lds <= 64 * 1024 or ng in (8, 12, 16), where                      # the instantiations whose dynamic-LDS limit is raised
        assert out[f.PW_PLAN_WM] == {32: 1, 64: 2, 128: 4}[mb] and tpw >= 1, where
        wp = 4 // out[f.PW_PLAN_WM]
        assert gx == G * -(-M // mb) * -(-(-(-N * HW // (32 * nsub))) // (wp * tpw)) and gx <= 768, where
    elif form == f.PW_FORM_LDS_RING:
        ks = out[f.PW_PLAN_KS]
        assert K % 2 == 0 and ks == (K + 31) // 32 * 32 + 1 and nsub in (1, 2, 4) and HW % nsub == 0 and tpw in (1, 2, 4), where
        assert mb in (32, 64, 96, 128) and lds == 4 * mb * (ks + 6) and lds <= 96 * 1024, where
        assert out[f.PW_PLAN_VECW] == int(K % 4 == 0) and out[f.PW_PLAN_RING] == 4, where
        assert _expected_refusal(K, M, G) == 0, where
    elif form == f.PW_FORM_SMALL_K:
        mt, mtiles = out[f.PW_PLAN_MT], out[f.PW_PLAN_MTILES]
        assert (K < 16 or K % 2) and lds == 4 * G * M * K and lds <= 48 * 1024, where
        assert mt in (2, 4, 8) and mtiles == -(-M // mt) and gx == -(-(-(-HW // 4)) // 256), where
        assert gy * gz >= N * G * mtiles > gy * (gz - 1), where
    elif form == f.PW_FORM_THIN:
        mt = out[f.PW_PLAN_MT]
        assert K % 8 == 0 and 8 <= K <= 64 and M <= mt and mt in (8, 16) and HW % 4 == 0, where
        assert lds == 4 * G * K * mt and lds <= 48 * 1024 and gx * gy * gz >= 400 and gx == -(-(HW // 4) // 256), where
    else:
        raise AssertionError('%s: form %d (the register-weights form is not reachable without a tuning variable)' % (where, form))
    return form


def _sweep():
    out = (ctypes.c_int32 * nv.PW_PLAN_LEN)()
    seen = set()
    for K in range(2, 1025):
        for M, G in itertools.product(SWEEP_M, (1, 4)):
            for N, HW in SWEEP_MAPS:
                seen.add(_sweep_check(K, M, G, N, HW, 0, out))
            seen.add(_sweep_check(K, M, G, 2, 48, nv.PW_TERM_RESIDUAL, out))
    return seen


def test_loop_invariants_over_a_dense_sweep():
    seen = _sweep()
    assert seen == {'refused', nv.PW_FORM_THIN, nv.PW_FORM_SMALL_K, nv.PW_FORM_SPLIT_K, nv.PW_FORM_TILE_PIPELINED, nv.PW_FORM_LDS_RING}


def test_split_k_declines_a_slice_its_chunks_do_not_divide():
    """Chunks of 2*CH k with CH = 16 when K/4 is a multiple of 32, else 8: for K % 64 == 32 the slice K/4 is no whole number of
    chunks (K/4 = 24 in chunks of 16 ends 8 k past the slice, in the next wave's slice, the next weight row, the next image).  Those K
    are not split-K, at the shapes that meet every other condition of the form."""
    bad = [K for K in range(64, 1025, 32) if (K // 4) % (2 * (16 if (K // 4) % 32 == 0 else 8))]
    assert bad[:4] == [96, 160, 224, 288] and all(K % 64 == 32 for K in bad)
    out = (ctypes.c_int32 * nv.PW_PLAN_LEN)()
    for K in bad:
        assert _sweep_check(K, 10, 1, 2, 77, 0, out) != nv.PW_FORM_SPLIT_K, K


def test_plan_rejects_what_the_launcher_rejects():
    out = (ctypes.c_int32 * nv.PW_PLAN_LEN)()
    plan = lambda *a: nv.lib.mspl_conv1x1_fwd_plan(*a)                           # noqa: E731
    assert plan(2, 64, 16, 1, 35, 0, 0, 16, 16, 16, 16, 16, None) == nv.ERR_NULL_POINTER
    assert plan(0, 64, 16, 1, 35, 0, 0, 16, 16, 16, 16, 16, out) == nv.ERR_BAD_SHAPE
    assert plan(2, 64, 16, 3, 35, 0, 0, 16, 16, 16, 16, 16, out) == nv.ERR_BAD_SHAPE          # channels not divisible by groups
    assert plan(2, 64, 16, 1, 35, 8, 0, 16, 16, 16, 16, 16, out) == nv.ERR_BAD_SHAPE          # destination narrower than the output
    assert plan(2, 64, 16, 1, 35, 0, 0, 16, 12, 16, 16, 16, out) == nv.ERR_BAD_SHAPE          # an alignment that is no power of two
    # 32-bit byte offsets of the matrix-core forms: N * Cin * HW floats (or the destination's) at 4 GiB
    assert plan(4, 128, 64, 1, 2 ** 21, 0, 0, 16, 16, 16, 16, 16, out) == nv.ERR_UNSUPPORTED
    assert plan(4, 64, 64, 1, 2 ** 21, 128, 0, 16, 16, 16, 16, 16, out) == nv.ERR_UNSUPPORTED
    assert plan(4, 64, 64, 1, 2 ** 21, 0, 0, 16, 16, 16, 16, 16, out) == 0 and out[nv.PW_PLAN_FORM] == nv.PW_FORM_TILE_PIPELINED
    # the refusals test_gpu_kernels.py expects from the launcher
    assert plan(1, 1024, 64, 1, 32, 0, 0, 16, 16, 16, 16, 16, out) == nv.ERR_UNSUPPORTED
    assert 'exceeds the LDS weight tile' in nv.last_error()


# ------------------------------------------------------------------------------------------------------------------ the models
def _model_triples():
    from mspl_amd import layers, models
    found = set()

    def collect(m):
        gates = {id(mod.wt_layer[1]) for mod in m.modules() if isinstance(mod, layers.EfficientPWConv)}     # ops.gap_gate, not conv1x1
        for mod in m.modules():
            if isinstance(mod, nn.Conv2d) and mod.kernel_size == (1, 1) and id(mod) not in gates:
                found.add((mod.in_channels, mod.out_channels, mod.groups))
            if isinstance(mod, models.FusionGate):                                                          # two c -> c halves
                found.add((mod.nchannel, mod.nchannel, 1))
    for s, ds, classes in itertools.product(sorted(models.sc_ch_dict), ('pascal', 'coco'), (5, 21)):
        args = argparse.Namespace(s=s, channels=3, num_classes=1000)
        assert models.DEC_FEAT[ds] == {'pascal': 16, 'coco': 32}[ds]
        for fix in (False, True):
            collect(models.ESPDNetwithUncertaintyEstimation(args, classes=classes, dataset=ds, fix_pyr_plane_proj=fix))
        collect(models.ESPDNetSegmentation(args, classes=classes, dataset=ds))
        collect(models.ESPNetv2Segmentation(args, classes=classes, dataset=ds))
    return found


def test_every_model_shape_is_in_the_table():
    found = _model_triples()
    table = {(a, b, g) for a, b, g, _ in cc.MODEL_SHAPES}
    assert found == table, 'missing from the table: %s; not in any model: %s' % (sorted(found - table), sorted(table - found))
    for cin, cout, g, form in cc.MODEL_SHAPES:
        case = cc.BY_NAME['model_%d_%d_g%d' % (cin, cout, g)]
        assert (case.refused is not None) == (form == 'refused')
    # the widths the s = 2.0 / s = 0.5 'pascal' shapes of the older tests never had
    ks = {a // g for a, b, g in found}
    assert ks >= {20, 40, 80, 24, 48, 96, 320, 384}
    # the shape whose split-K launch read out of bounds: dataset 'coco', 21 classes, bu_dec_l3's projection
    assert (96, 10, 1) in found and cc.plan(cc.BY_NAME['model_96_10_g1'])['form'] == 'pipe'


# ------------------------------------------------------------------------------------------------------------------ the data
@pytest.mark.parametrize('name', cc.NAMES)
def test_data_are_exact(name):
    case = cc.BY_NAME[name]
    acc64 = cc.accumulate(case)
    acc32 = cc.accumulate(case, torch.float32)
    assert acc32.dtype == torch.float32 and torch.equal(acc32.double(), acc64), 'float32 and float64 convolutions differ'
    mag_acc = cc.accumulate(case, magnitude=True)
    x, w = cc.inputs(name)
    assert x.abs().min() >= 1 and w.abs().min() >= 1, 'no zeros: every term counts'
    assert not torch.equal(x[0], x[1]), 'the images differ'
    for ts in (frozenset(),) + case.termsets + case.leaves + (ec.ALL,):
        # precondition: the same expression on the absolute values, on the 2^-Q grid, stays below 2^24 (scale and gate may be 0.5:
        # the bound of a term set is its own, and the one with every term present is among them)
        mag = cc.reference(case, mag_acc, ts, magnitude=True)
        top = float(mag.max()) * 2.0 ** cc.Q
        assert top < 2.0 ** 24, '%s %s: |.| expression %.2f on the 2^-%d grid reaches 2^%.2f' % (name, ec.term_id(ts), float(mag.max()), cc.Q,
                                                                                              torch.tensor(top).log2())
        r64 = cc.reference(case, acc64, ts)
        assert torch.all(r64.abs() <= mag), 'the magnitude evaluation is not a bound'
        scaled = r64 * 2.0 ** cc.Q
        assert torch.equal(scaled, scaled.round()), 'the reference leaves the 2^-%d grid' % cc.Q
        r32 = cc.reference(case, acc32, {t for t in ts})
        assert r32.dtype == torch.float32 and torch.equal(r32.double(), r64), '%s %s: float32 and float64 CPU results differ' % (name, ec.term_id(ts))


@pytest.mark.parametrize('name', cc.RANDOM)
def test_random_pass_tolerance_comes_from_the_reference(name):
    """The random-data pass compares at the standing tolerance of tests/epilogue_cases.py; torch's own float32 evaluation of the
    reference stays within a quarter of it (bare and with every term), so a kernel's summation order has room."""
    import torch.nn.functional as F
    case = cc.BY_NAME[name]
    for ts in (frozenset(), ec.AFFINE, ec.ALL):
        inp, t = cc.random_problem(name, ts)
        G = case.shape[3]
        r64 = ec.ref_epilogue(F.conv2d(inp['x'].double(), inp['w'].double(), None, 1, 0, 1, G), t)
        r32 = ec.ref_epilogue(F.conv2d(inp['x'], inp['w'], None, 1, 0, 1, G), t)
        gap = float((r32.double() - r64).abs().max())
        print('%s %s: float32 gap %.3e' % (name, ec.term_id(ts), gap))
        assert 4.0 * gap <= ec.ATOL, '%s %s: 4 x the float32 gap (%.3e) exceeds the standing tolerance' % (name, ec.term_id(ts), gap)
