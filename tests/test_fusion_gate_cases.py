"""The case table of tests/fusion_gate_cases.py against the library's plan queries: no GPU, no kernel runs.  The table must cover
every seam the plans report for each channel count, the integer data must be exact, and what the node declines is declined by all
four host entry points alike."""
import ctypes

import pytest

from mspl_amd import _native as nv
from mspl_amd import ops
from tests import fusion_gate_cases as fc


@pytest.mark.parametrize('C', fc.CHANNELS)
def test_table_covers_every_reported_seam(C):
    covered = set()
    for case in fc.CASES:
        if case.C == C:
            got = fc.seams(case)
            # the `why` column is what the table promises; the plans must agree with it
            promised = {w.split()[0] for w in case.why.split(', ')}
            assert promised <= got, (case.name, promised - got)
            covered |= got
    assert covered == fc.reported_seams(C), (C, fc.reported_seams(C) - covered)


@pytest.mark.parametrize('C', fc.CHANNELS)
def test_forward_plan(C):
    p = ops.fusion_gate_conv_plan(2, C, 64)
    rows = 32 if C in (32, 512) else 64
    assert p['form'] == nv.FGC_FORM_MFMA_X4 and p['rows'] == rows and p['wave_pixels'] == 128
    assert p['pixels'] == 128 * 4 // (rows // 32)
    # one source's weight tile with an odd row stride: never more than the 1x1 kernel stages at K = 512 (32 rows of 513 + 6 floats)
    assert p['lds_bytes'] == 4 * rows * (C + 1) <= 4 * 32 * (513 + 6)
    assert p['grid_x'] == (C // rows) * -(-1 // (p['pixels'] // 128))
    big = ops.fusion_gate_conv_plan(16, C, 256 * 480 * 32 // C // 4)
    assert big['grid_x'] == (C // rows) * -(-(16 * (256 * 480 * 32 // C // 4)) // p['pixels'])


def test_weight_gradient_plan():
    for case in fc.CASES:
        p = ops.fusion_gate_conv_bwd_weight_plan(case.N, case.C, case.H * case.W)
        if case.H * case.W % 4:
            assert p == {'form': nv.FGC_WGRAD_SCALAR, 'parts': 1, 'ngroups': 0}, case.name
            f = ops.fusion_gate_conv_plan(case.N, case.C, case.H * case.W)
            assert f == {'form': nv.FGC_FORM_SCALAR, 'rows': 0, 'pixels': 0, 'wave_pixels': 0, 'lds_bytes': 0,
                         'grid_x': -(-case.N * case.C * case.H * case.W // 256)}, case.name
            continue
        ngroups = case.N * -(-case.H * case.W // 64)
        want = max(4, min(-(-3072 // (case.C // 32) ** 2), ngroups))
        assert p == {'form': nv.FGC_WGRAD_MFMA_PAIR, 'parts': (want + 3) // 4 * 4, 'ngroups': ngroups}, case.name


def test_declined_shapes_are_declined_everywhere():
    f, p, g = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    out = (ctypes.c_int32 * nv.FGC_PLAN_LEN)()
    for N, C, HW in fc.DECLINED:
        assert not ops.fusion_gate_conv_fits(N, C, HW)
        assert nv.lib.mspl_fusion_gate_conv_plan(N, C, HW, out) == nv.ERR_UNSUPPORTED
        assert list(out) == [0] * nv.FGC_PLAN_LEN
        assert nv.lib.mspl_fusion_gate_conv_bwd_weight_plan(N, C, HW, ctypes.byref(f), ctypes.byref(p), ctypes.byref(g)) == nv.ERR_UNSUPPORTED
        assert ops.fusion_gate_conv_plan(N, C, HW) is None and ops.fusion_gate_conv_bwd_weight_plan(N, C, HW) is None
    for case in fc.CASES:
        assert ops.fusion_gate_conv_fits(case.N, case.C, case.H * case.W)
    assert nv.lib.mspl_fusion_gate_conv_plan(0, 32, 16, out) == nv.ERR_BAD_SHAPE
    assert nv.lib.mspl_fusion_gate_conv_bwd_weight_plan(2, 32, 16, ctypes.byref(f), ctypes.byref(p), None) == 0      # ngroups optional


def test_integer_data_is_exact_in_float32():
    """The precondition of the EQUAL checks: on absolute values, in units of 1/8, every sum stays below 2^24."""
    for case in fc.CASES:
        hw = case.N * case.H * case.W
        assert 2 * case.C * 4 * 8 < 2 ** 24                      # |z| * 8
        assert hw * 16 + 4 < 2 ** 24                             # |gw| with the non-zero start
        r = fc.integer_problem(case.name)
        assert float((r['z'] * 8).abs().max()) < 2 ** 24 and float(((r['z'] * 8) % 1).abs().max()) == 0
        assert float(r['gw'].abs().max()) + 4 < 2 ** 24 and float((r['gw'] % 1).abs().max()) == 0
