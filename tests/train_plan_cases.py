"""The sweep of the training kernels' host-side plan queries -- the convolution weight gradient (conv_bwd.hip), the bilinear and
avg-pool backward (resample_bwd.hip) -- shared by tests/golden/make_train_plans_golden.py (which records what the library answers)
and tests/test_train_plans_golden.py (which asks again).  No GPU: every query looks at shapes only.

`records()` is a dict query -> list of argument tuples; `answers(query, record)` is a tuple of ints:
    wgrad     (N, Cin, Cout, groups, H, W, K, stride, dilation, aligned16)  -> (form, parts, ngroups)
    bilinear  (planes, Hi, Wi, Ho, Wo)                                      -> (form, tiles_x, tiles_y, FH, FW)
    avgpool   (planes, H, W, aligned16)                                     -> (form,)"""
import ctypes
import itertools

from mspl_amd import _native as nv
from tests import exact_cases as X
from tests import resample_cases as R

QUERIES = ('wgrad', 'bilinear', 'avgpool')

# every enumerator of the three form enums (include/mspl_hip.h)
WGRAD_FORMS = {nv.WGRAD_1X1_MFMA, nv.WGRAD_1X1_LDS, nv.WGRAD_STEM_S2_STRIP, nv.WGRAD_STEM_COB4, nv.WGRAD_STRIP, nv.WGRAD_G3X3,
               nv.WGRAD_GENERIC}
BILINEAR_FORMS = set(R.BIL)
AVGPOOL_FORMS = set(R.AVG)

# ------------------------------------------------------------------------------------------------------------------ weight gradient
# channels per group -> (Cin, Cout, groups).  3 comes three times: cout_g % 4 != 0, and the stem shape with Cout of 12 and 16 (the
# planner asks for Cout >= 16)
CHANNELS = [(1, (8, 8, 8)), (2, (8, 8, 4)), (3, (12, 12, 4)), (3, (3, 12, 1)), (3, (3, 16, 1)), (4, (8, 8, 2)), (5, (10, 4, 2)),
            (6, (12, 12, 2)), (8, (16, 8, 2)), (16, (32, 32, 2)), (64, (64, 64, 1))]
WIDTHS = (7, 8, 9, 11, 12, 13, 15, 16, 17, 23, 24, 25)          # multiples of 8 and of 4, +/- 1 around them: odd ones among those
HEIGHTS = (16, 17)
# `chunks *= 2` goes on while units / (2 * chunks) >= T, units = N * Ho * Wo pixels or a quarter of that in strips; T per form:
# 256 (1x1 LDS), 512 (stem stride-2 strips), 1024 (strips), 2048 (stem cob4, g3x3), 4096 (generic)
DOUBLINGS = (1, 2, 8, 64)


def _seams(T):
    return [2 * c * T + d for c in DOUBLINGS for d in (-1, 0, 1)]


def _wgrad_records():
    out = []
    for (cg, (ci, co, g)), W, H, N, al in itertools.product(CHANNELS, WIDTHS, HEIGHTS, (1, 3), (0, 1)):
        for s in (1, 2):
            out.append((N, ci, co, g, H, W, 1, s, 1, al))
            for d in (1, 2):
                out.append((N, ci, co, g, H, W, 3, s, d, al))
    # units on both sides of every doubling: one row (two for the stride-2 strips, whose H must be even) of exactly that many units
    for u in _seams(256):
        out.append((1, 4, 4, 1, 1, u, 1, 1, 1, 1))                    # 1x1 LDS (fewer than 8 channels per group)
    for u in _seams(512):
        out.append((1, 3, 16, 1, 2, 8 * u, 3, 2, 1, 1))               # stem, stride-2 strips
    for u in _seams(1024):
        out.append((1, 8, 8, 8, 1, 4 * u, 3, 1, 1, 1))                # strips
    for u in _seams(2048):
        out.append((1, 3, 16, 1, 1, u, 3, 1, 1, 1))                   # stem, four output channels per workgroup
        out.append((1, 8, 8, 8, 1, u, 3, 1, 2, 1))                    # g3x3 (dilated)
    for u in _seams(4096):
        out.append((1, 12, 12, 2, 1, u, 3, 1, 1, 1))                  # generic
    # the workgroup limits (2048; 4096 for g3x3), the reduction range long enough for every doubling: 4 x 64x64
    for C in (1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097):
        out.append((4, C, C, C, 64, 64, 3, 1, 1, 1))                  # strips, depthwise: workgroups = Cout * chunks
        out.append((4, C, C, C, 64, 64, 3, 1, 2, 1))                  # g3x3
        out.append((4, 4 * C, 4 * C, C, 64, 64, 1, 1, 1, 1))          # 1x1 LDS: one 16x16 tile per group
    for co in (2044, 2048, 2052, 4092, 4096, 4100, 8188, 8192, 8196):
        out.append((4, 3, co, 1, 64, 64, 3, 2, 1, 1))                 # stem stride-2 strips: Cout / 2 workgroups per chunk
        out.append((4, 3, co, 1, 64, 64, 3, 1, 1, 1))                 # stem cob4: Cout / 4
    for g in (3, 6, 7, 12, 13):
        out.append((4, 6 * g, 6 * g, g, 64, 64, 3, 1, 1, 1))          # generic: Cout * cin_g * 9 = 324 * groups weights
    # the shapes tests/exact_cases.py names (N, Cin, Cout, groups, H, W, K, stride)
    for _name, shape, _expect in X.CONV_SHAPES:
        for al in (0, 1):
            out.append(tuple(shape) + (1, al))
    return out


# ------------------------------------------------------------------------------------------------------------------ bilinear backward
FACTORS = (0.4, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 4.5, 5.0, 8.0)
IN_HEIGHTS = (3, 4, 5, 7, 8, 9)             # the tile heights, 4 and 8, +/- 1
IN_WIDTHS = (63, 64, 65)                    # the tile width +/- 1


def _bilinear_records():
    out = []
    for Hi, Wi, fy, fx in itertools.product(IN_HEIGHTS, IN_WIDTHS, FACTORS, FACTORS):
        out.append((3, Hi, Wi, max(1, int(Hi * fy)), max(1, int(Wi * fx))))
    for Hi, Wi in itertools.product(IN_HEIGHTS, IN_WIDTHS):
        out += [(3, Hi, Wi, 1, 2 * Wi), (3, Hi, Wi, 2 * Hi, 1), (3, Hi, Wi, 1, 1)]
    out.append((2, 3, 2, 8, 8193))          # Wo > 8192: the wave form
    out.append((2, 3, 2, 8, 8192))
    # (a tile of more than 64 KiB of LDS: see UNREACHABLE)
    out.append((1, 128, 4096, 512, 16384))  # x4 in both directions at 64 column tiles: the tile form has no limit on Wo
    for c in R.CASES:
        if c.op == 'bilinear':
            out.append(tuple(c.shape))
    return out


# ------------------------------------------------------------------------------------------------------------------ avg-pool backward
def _avgpool_records():
    out = []
    for H, W, al in itertools.product((1, 2, 7, 16, 17), (1, 7, 8, 9, 15, 16, 17, 20, 23, 24, 25), (0, 1)):
        out.append((3, H, W, al))
    for c in R.CASES:
        if c.op == 'avgpool':
            out.append(tuple(c.shape) + (0 if c.cfg.get('misalign') else 1,))
    return out


# (planes, H, W): H * W * W at 2^32 - 65536 (answered) and at 2^32 (refused); tests/test_resample_cases.py has the second
AVGPOOL_EDGE = [((1, 65535, 256), 0), ((1, 65536, 256), nv.ERR_BAD_SHAPE), ((1, 70000, 300), nv.ERR_BAD_SHAPE)]

# Decisions of the planners that no plan query can show, with the reason (the generator prints them instead of passing silently)
UNREACHABLE = {
    'bilinear tile of more than 64 KiB of LDS': (
        'the tile forms are taken only for windows 2 / s + 3 <= 12 (8) with tiles of 4 (8) x 64 input pixels, so FH <= (TLH + 1) / s + 3 '
        '<= 25 rows and FW <= 65 / s + 3 <= 295 columns, FWS <= 316: at most (25 * 316 + 37 * 64 + 12 * 64 + 48 + 68) * 4 = 44 608 bytes'),
}


def records():
    return {'wgrad': _wgrad_records(), 'bilinear': _bilinear_records(), 'avgpool': _avgpool_records()}


def _ints(n):
    return [ctypes.c_int32() for _ in range(n)]


def answers(query, rec):
    lib = nv.lib
    if query == 'wgrad':
        f, parts, ng = _ints(3)
        nv.check(lib.mspl_conv_bwd_weight_plan(*rec, ctypes.byref(f), ctypes.byref(parts), ctypes.byref(ng)))
        return f.value, parts.value, ng.value
    if query == 'bilinear':
        v = _ints(5)
        nv.check(lib.mspl_bilinear_bwd_plan(1, *rec, 1, *[ctypes.byref(x) for x in v]))
        return tuple(x.value for x in v)
    planes, H, W, al = rec
    f = ctypes.c_int32()
    nv.check(lib.mspl_avgpool3x3s2_bwd_plan(1, planes, H, W, al, ctypes.byref(f)))
    return (f.value,)


def avgpool_edge(shape):
    """The return code of the avg-pool query at the 32-bit index limit."""
    f = ctypes.c_int32()
    return nv.lib.mspl_avgpool3x3s2_bwd_plan(1, *shape, 1, ctypes.byref(f))
