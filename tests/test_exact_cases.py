"""The integer-data cases of tests/exact_cases.py, checked without a GPU: the data are exact (the bound, and float32 == float64 on
the CPU in ATen's own summation order), and the library's plan queries confirm that every case reaches the kernel form and the seam
(chunks, bands, padded slots, slots across images) it is in the table for.  A case whose property is not met FAILS."""
import pytest
import torch

from mspl_amd import _native as nv
from tests import exact_cases as ec

IDS = [c.id for c in ec.CASES]


@pytest.mark.parametrize('cid', IDS)
def test_data_are_exact(cid):
    case = ec.BY_ID[cid]
    r64 = ec.reference64(cid)
    # precondition: every partial sum of every output is a multiple of 2^-Q below 2^24 * 2^-Q in magnitude
    mag = ec.reference(case, ec.magnitude_inputs(case))
    assert set(mag) == set(r64)
    for name, m in mag.items():
        q = ec.grid_q(case, name)
        top = float(m.abs().max()) * 2.0 ** q
        assert top < 2.0 ** 24, '%s %s: |.| sum %.0f on the 2^-%d grid reaches 2^%.2f' % (cid, name, float(m.abs().max()), q, torch.tensor(top).log2())
        assert torch.all(r64[name].abs() <= m.abs()), '%s %s: the magnitude evaluation is not a bound' % (cid, name)
        scaled = r64[name] * 2.0 ** q
        assert torch.equal(scaled, scaled.round()), '%s %s: the reference leaves the 2^-%d grid' % (cid, name, q)
    # a second summation order: the same reference in float32
    r32 = ec.reference(case, dtype=torch.float32)
    for name, r in r64.items():
        assert r32[name].dtype == torch.float32
        assert torch.equal(r32[name].double(), r), '%s %s: float32 and float64 CPU results differ' % (cid, name)
    # PReLU branches are never in doubt
    p = ec.inputs(case)
    if case.op in ('eesp_fused', 'hff_bn'):
        assert torch.all(ec._bn(p['z'], p, '', torch.float64)[0] != 0)
    if case.op == 'eesp_fused' and case.cfg['tail']:
        assert torch.all(ec._bn(p['c'], p, 'p', torch.float64)[0] != 0)


WGRAD = [c.id for c in ec.CASES if c.op == 'conv_wgrad']


@pytest.mark.parametrize('cid', WGRAD)
def test_weight_gradient_plan(cid):
    case = ec.BY_ID[cid]
    e, shape = case.expect, case.cfg['shape']
    N, Cin, Cout, G, H, W, K, s = shape
    form, parts, ngroups = ec.wgrad_plan(shape, e.get('aligned16', True))
    assert form == e['form'], '%s: form %d, the table wants %d' % (cid, form, e['form'])
    if 'cin_g' in e:
        assert Cin // G == e['cin_g']
    if 'parts_min' in e:
        assert parts >= e['parts_min'] and ngroups == 0
    if e.get('seam_inside_image'):
        # ceil(total / parts) is no multiple of the plane: a chunk ends inside an image, and the last chunk is shorter
        npix, unit = ec.conv_out(H, K, s) * ec.conv_out(W, K, s), 4 if form in (nv.WGRAD_STRIP, nv.WGRAD_STEM_S2_STRIP) else 1
        assert (N * npix // unit) % parts != 0 and (-(-N * npix // unit // parts)) % (npix // unit) != 0
    if e.get('padded_pairs'):
        assert (G * parts) % 8 != 0
    if e.get('slots') == 'span':
        gpi = -(-H * W // 64)
        assert parts < ngroups and ngroups % parts != 0 and parts % gpi != 0          # slot q and q + parts lie in different images
    if e.get('slots') == 'empty':
        assert parts > ngroups
    if cid.startswith('conv_wgrad-mfma_partial'):
        assert (Cout // G) % 32 and (Cin // G) % 32 and (H * W) % 64
    if case.cfg.get('misalign'):
        assert ec.wgrad_plan(shape, True)[0] != form, 'the aligned call takes the same form: nothing falls back'


def test_every_form_is_reached_in_parts():
    """Every mspl_wgrad_form_t value at least once with parts >= 2 (all seven forms can split their reduction)."""
    seen = {}
    for cid in WGRAD:
        case = ec.BY_ID[cid]
        form, parts, _ = ec.wgrad_plan(case.cfg['shape'], case.expect.get('aligned16', True))
        seen[form] = max(seen.get(form, 0), parts)
    forms = [nv.WGRAD_1X1_MFMA, nv.WGRAD_1X1_LDS, nv.WGRAD_STEM_S2_STRIP, nv.WGRAD_STEM_COB4, nv.WGRAD_STRIP, nv.WGRAD_G3X3, nv.WGRAD_GENERIC]
    assert sorted(seen) == forms
    assert all(seen[f] >= 2 for f in forms), seen
    # strip<c> and g3x3<c> are compiled per cin_g: each instantiation in two chunks
    for form in (nv.WGRAD_STRIP, nv.WGRAD_G3X3):
        got = {ec.BY_ID[c].cfg['shape'][1] // ec.BY_ID[c].cfg['shape'][3] for c in WGRAD
               if ec.wgrad_plan(ec.BY_ID[c].cfg['shape'], ec.BY_ID[c].expect.get('aligned16', True))[0] == form}
        assert got >= {1, 2, 3, 4, 5, 8}, (form, got)


def test_plan_rejects_what_the_launcher_rejects():
    import ctypes
    f, p = ctypes.c_int32(), ctypes.c_int32()
    assert nv.lib.mspl_conv_bwd_weight_plan(2, 8, 8, 3, 9, 9, 3, 1, 1, 1, ctypes.byref(f), ctypes.byref(p), None) == -1       # groups
    assert nv.lib.mspl_conv_bwd_weight_plan(2, 8, 8, 1, 9, 9, 5, 1, 1, 1, ctypes.byref(f), ctypes.byref(p), None) == nv.ERR_UNSUPPORTED
    assert nv.lib.mspl_conv_bwd_weight_plan(2, 8, 8, 1, 9, 9, 3, 1, 1, 1, ctypes.byref(f), ctypes.byref(p), None) == 0        # ngroups optional
    assert ec.dw_chunks((0, 4, 8, 8), 1) == 0 and ec.dw_chunks((1, 4, 8, 8), 3) == 0
    assert ec.fused_bands((1, 4, 9, 15), [1, 2, 3, 5]) == (0, 0)                # a dilation the fused backward does not cover
    for shape, dil in [((1, 4, 9, 15), [1, 2, 3, 4]), ((2, 4, 37, 60), [1, 2, 3, 4]), ((1, 4, 18, 4000), [1, 1, 2, 3])]:
        fits = nv.lib.mspl_eesp_bwd_fused_fits(*shape, (ctypes.c_int32 * 4)(*dil))
        assert bool(ec.fused_bands(shape, dil)[0]) == bool(fits)


@pytest.mark.parametrize('cid', [c.id for c in ec.CASES if c.op == 'eesp_dw'])
def test_depthwise_plan(cid):
    case = ec.BY_ID[cid]
    assert ec.dw_chunks(case.cfg['shape'], case.cfg['stride']) >= case.expect['chunks_min']


@pytest.mark.parametrize('cid', [c.id for c in ec.CASES if c.op == 'eesp_fused'])
def test_fused_bands_plan(cid):
    case = ec.BY_ID[cid]
    bands, rows = ec.fused_bands(case.cfg['shape'], case.cfg['dil'])
    H = case.cfg['shape'][2]
    assert (bands, rows, H - (bands - 1) * rows) == (case.expect['bands'], case.expect['band_rows'], case.expect['last_rows'])
