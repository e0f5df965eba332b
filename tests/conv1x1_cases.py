"""Integer-data cases for the forward 1x1 convolution (mspl_conv1x1_fwd) at the K / M / pixel seams of each of its kernel forms, with
the float64 reference every check compares against.  Shared by tests/test_conv1x1_cases.py (no GPU: the table against the library's
plan query, the exactness precondition, the model-derived shapes) and tests/test_gpu_conv1x1_forms.py (the kernels).  Nothing here
touches the code under test except the plan query (ops.conv1x1_plan: the host function the launcher itself switches on).

Data rule (tests/exact_cases.py): activations, weights, pre_add, residual and the reinforcement from {-2, -1, 1, 2}, scale and gate
from {0.5, 1, 2}, shift from odd multiples of 0.25, PReLU slopes from {0.25, 0.5}: every product and every partial sum of every form
(matrix cores, four-way split K, vector unit) is exact in float32, so the kernel's output must EQUAL the float64 reference.  N >= 2
with different data per image and per output row: a k-loop that runs past its slice, into the next weight row or the next image,
changes an integer.  The bound (checked on the CPU, a condition on the data and no tolerance): the same expression on the absolute
values of all operands, times 2^Q with Q = 5 (scale 2^-1, shift 2^-2, slope 2^-2 on the 2^-2 grid -> 2^-4, gate 2^-1), stays below
2^24 for every output.  With K = 1024 it is (4 * 1024 + 2) * 2 + 1.25 + 12 + 2 = 8211.25, times 2 for the gate, times 2^5: 2^19.

A case names the form and the variant parameters the plan must answer for it (`expect`: a subset of the plan's fields, for the bare
call); `termsets` are the epilogue term sets it is run with besides the bare call; `leaves` are term sets that must move the call to
another form (split-K takes scale / shift / alpha / raw_out only; the thin form wants 16-byte aligned operands).  `refused`: the
launcher's error code, nothing is launched.  ctot / coff: a wider destination, written at channel coff.  *_off: that pointer is
displaced by one float (4 bytes) from its 16-byte aligned base.
"""
import collections
import functools

import torch
import torch.nn.functional as F

from mspl_amd import _native as nv
from mspl_amd import ops
from tests.epilogue_cases import AFFINE, ALL, ATOL, RTOL, TERMS, ref_epilogue, term_id  # noqa: F401
from tests.exact_cases import SCALES, SHIFTS, SLOPES, VALS, draw

Q = 5
RAW = AFFINE | {'raw_out'}
OPERAND_TERMS = frozenset(('pre_add', 'residual', 'reinf'))
SENTINEL = -777.0

Case = collections.namedtuple('Case', 'name shape expect why termsets leaves refused ctot coff x_off w_off out_off op_off')

CASES = []


def _c(name, shape, expect, why, termsets=None, leaves=(), refused=None, ctot=0, coff=0, x_off=0, w_off=0, out_off=0, op_off=0):
    if termsets is None:
        termsets = (AFFINE, ALL) if ctot else (AFFINE, RAW, ALL)
    if isinstance(expect, str):
        expect = {'form': expect}
    CASES.append(Case(name, shape, expect, why, tuple(frozenset(t) for t in termsets), tuple(frozenset(t) for t in leaves), refused,
                      ctot, coff, x_off, w_off, out_off, op_off))


# shape: (N, Cin, Cout, groups, H, W)
# ---------------------------------------------------------------------------------------------------------------- split-K
# M <= 32, ungrouped, K >= 4M, K % 64 == 0, N * ceil(HW / 32) <= 6000, scale / shift / alpha / raw_out only.  CH = 16 when K/4 is a
# multiple of 32, else 8.  K = 96, 160, 224 have K/4 = 24, 40, 56: no whole number of 16-k chunks -- not this form's.
SK_TERMS = (AFFINE, RAW)
for K, hw_a, hw_b in ((64, (1, 1), (7, 11)), (128, (1, 31), (4, 8)), (192, (3, 11), (1, 1)), (256, (7, 11), (1, 31)),
                      (320, (4, 8), (3, 11)), (384, (1, 1), (7, 11)), (512, (1, 31), (4, 8)), (640, (3, 11), (1, 31))):
    ch = 16 if (K // 4) % 32 == 0 else 8
    Mtop = min(K // 4, 32)
    _c('sk_k%d_m10' % K, (2, K, 10, 1) + hw_a, dict(form='split_k', ch=ch, ks=K // 4, nsub=1, tiles=-(-hw_a[0] * hw_a[1] // 32)),
       'split-K, 10 of 32 rows', SK_TERMS)
    _c('sk_k%d_m%d' % (K, Mtop), (2, K, Mtop, 1) + hw_b, dict(form='split_k', ch=ch, ks=K // 4, nsub=1), 'split-K, K = 4M or M = 32', SK_TERMS)
for K, form in ((96, 'pipe'), (160, 'ring'), (224, 'ring')):
    _c('sk_not_k%d_m10' % K, (2, K, 10, 1, 7, 11), form, 'K/4 = %d is no multiple of 16: not split-K (the shape that read out of bounds)' % (K // 4),
       SK_TERMS)
    _c('sk_not_k%d_m%d' % (K, min(K // 4, 32)), (2, K, min(K // 4, 32), 1, 1, 33), form, 'K % 64 = 32 at the largest M split-K would take', SK_TERMS)
_c('sk_not_k64_m17', (2, 64, 17, 1, 7, 11), dict(form='pipe', ng=8), 'M = K/4 + 1: K < 4M, not split-K', SK_TERMS)
_c('sk_not_k128_m33', (2, 128, 33, 1, 1, 33), dict(form='pipe', ng=16), 'M = K/4 + 1 = 33 > 32: not split-K', SK_TERMS)
_c('sk_not_k256_m33', (2, 256, 33, 1, 1, 31), 'ring', 'M = 33 > 32: not split-K, and no K = 256 tile-pipelined instantiation above 32 rows', SK_TERMS)
_c('sk_not_grouped', (2, 256, 20, 2, 4, 8), dict(form='pipe', ng=16), 'grouped: not split-K', SK_TERMS)
_c('sk_k128_nsub2', (2, 128, 20, 1, 1, 32737), dict(form='split_k', ch=16, ks=32, nsub=2, tiles=512),
   'two sub-tiles per workgroup (N * ceil(HW/64) = 1024), the last tile has 33 of 64 pixels', SK_TERMS)
_c('sk_k64_nsub2', (2, 64, 16, 1, 1, 32737), dict(form='split_k', ch=8, ks=16, nsub=2, tiles=512), 'the <2, 8> instantiation', SK_TERMS)
_c('sk_not_k96_big', (2, 96, 10, 1, 1, 32737), dict(form='pipe', ng=12, nsub=1, tpw=1, grid_x=512),
   'K = 96 at the map where split-K would have taken two sub-tiles: tile-pipelined, 2047 tiles on 512 workgroups', SK_TERMS)
_c('sk_over_6000', (2, 64, 10, 1, 1, 96001), dict(form='pipe', ng=8), 'N * ceil(HW/32) = 6002 > 6000: not split-K', (AFFINE,))
_c('sk_leaves_with_residual', (2, 128, 20, 1, 7, 11), dict(form='split_k', ch=16), 'a further term leaves the form', SK_TERMS,
   leaves=(AFFINE | {'residual'}, AFFINE | {'gate'}, ALL))
_c('sk_slice', (2, 128, 10, 1, 1, 33), dict(form='split_k'), 'split-K into a channel slice', (AFFINE,), ctot=17, coff=5)

# ---------------------------------------------------------------------------------------------------------------- tile-pipelined
# K = 8 * NG, NG in {2, 3, 4, 6, 8, 12, 16} (and 32, 64 with M <= 32), 16-byte aligned weights.  MB = min(128, M rounded up to 32),
# 96 -> 64.  Two pixels per lane when HW is even and x / out / the operands are 8-byte aligned.
for ng, M, G in ((2, 24, 2), (3, 32, 2), (4, 33, 2), (6, 64, 4), (8, 65, 2), (12, 96, 2), (16, 128, 2)):
    mb = {24: 32, 32: 32, 33: 64, 64: 64, 65: 64, 96: 64, 128: 64 if ng == 16 else 128}[M]
    _c('pipe_ng%d_m%d_odd' % (ng, M), (2, 8 * ng * G, M * G, G, 5, 7), dict(form='pipe', ng=ng, nsub=1, mb=mb, ar=min(M, mb)), 'odd map: one pixel per lane')
    _c('pipe_ng%d_m%d_even' % (ng, M), (2, 8 * ng * G, M * G, G, 6, 7), dict(form='pipe', ng=ng, nsub=2, mb=mb), 'even map: two pixels per lane')
_c('pipe_ng4_m160', (2, 32, 160, 1, 5, 7), dict(form='pipe', ng=4, mb=128, ar=128, wm=4), 'two row blocks of 128, the second with 32 rows')
_c('pipe_ng4_m128', (2, 32, 128, 1, 6, 7), dict(form='pipe', ng=4, mb=128, ar=128, wm=4, nsub=2), 'one row block of 128: four waves along M')
_c('pipe_ng32_m24', (2, 512, 48, 2, 5, 7), dict(form='pipe', ng=32, mb=32, ar=24), 'K = 256 per group, grouped so that split-K declines')
_c('pipe_ng32_m32_even', (2, 512, 64, 2, 6, 7), dict(form='pipe', ng=32, nsub=2, ar=32), 'K = 256, all 32 rows')
_c('pipe_ng64_m24', (2, 1024, 48, 2, 5, 7), dict(form='pipe', ng=64, ar=24, lds_bytes=4 * (32 * 6 + 24 * 513)), 'K = 512 per group')
_c('pipe_ng64_m32_ring', (2, 1024, 64, 2, 5, 7), 'ring', 'K = 512 with 32 rows: 32 * 513 + 192 floats exceed the 64 KiB the tile-pipelined form asks for')
_c('pipe_ng64_even', (2, 1024, 20, 2, 6, 8), dict(form='pipe', ng=64, nsub=2, ar=10), 'K = 512, two pixels per lane')
_c('pipe_slice_misaligned', (2, 64, 24, 2, 6, 7), dict(form='pipe', ng=4, nsub=1), 'a destination 4 bytes off an 8-byte boundary, written at a '
   'channel offset: one pixel per lane although the map is even', ctot=31, coff=3, out_off=1)
_c('pipe_slice', (2, 64, 24, 2, 6, 7), dict(form='pipe', ng=4, nsub=2), 'the same slice in an aligned destination', ctot=31, coff=3)
_c('pipe_operand_misaligned', (2, 64, 24, 2, 6, 7), dict(form='pipe', ng=4, nsub=2), 'a pre_add / residual 4 bytes off: one pixel per lane with '
   'them (the plan of the full term set says nsub = 1)', (AFFINE, ALL), op_off=1)
_c('pipe_tpw2', (2, 16, 160, 1, 1, 12290), dict(form='pipe', ng=2, nsub=2, mb=128, tpw=2, grid_x=386), '2 x 385 tiles are more than 768 workgroups: two per wave')

# ---------------------------------------------------------------------------------------------------------------- LDS ring
# every other even K >= 16 (and the K the tile-pipelined form has no instantiation for).  Weight rows padded to 32 columns in LDS;
# MB shrinks until MB * (KS + 6) floats fit 40 KiB; K % 4 != 0 or a weight pointer off 16 bytes: scalar weight staging.
for K, M, G, hw in ((18, 5, 2, (5, 7)), (20, 32, 4, (5, 7)), (22, 33, 1, (6, 7)), (26, 128, 1, (5, 7)), (40, 129, 1, (5, 7)), (56, 10, 2, (6, 7)),
                    (80, 20, 4, (5, 7)), (160, 20, 1, (5, 7)), (192, 48, 2, (5, 7)), (320, 128, 1, (5, 7)), (384, 33, 2, (5, 7)),
                    (640, 40, 1, (1, 33)), (256, 64, 1, (5, 7)), (512, 33, 1, (5, 7))):
    K32 = (K + 31) // 32 * 32
    mb = min(128, (M + 31) // 32 * 32)
    while mb > 32 and mb * (K32 + 1 + 6) * 4 > 40 * 1024:
        mb -= 32
    _c('ring_k%d_m%d' % (K, M), (2, K * G, M * G, G) + hw, dict(form='ring', ks=K32 + 1, mb=mb, vecw=int(K % 4 == 0), nsub=1, ring=4,
                                                                lds_bytes=4 * mb * (K32 + 7)),
       'LDS ring' + ('' if K % 4 == 0 else ', scalar weight staging (K % 4 != 0)'))
_c('ring_w_off', (2, 40, 33, 1, 5, 7), dict(form='ring', vecw=0), 'a weight pointer 4 bytes off a 16-byte boundary: scalar weight staging', w_off=1)
_c('ring_w_off_k32', (2, 64, 24, 2, 5, 7), dict(form='ring', vecw=0, ks=33), 'K = 32 with misaligned weights leaves the tile-pipelined form', w_off=1)
_c('ring_m96', (2, 20, 96, 1, 5, 7), dict(form='ring', mb=96, wm=4), 'three 32-row chunks on four waves')
_c('ring_nsub2', (2, 288, 80, 16, 1, 4066), dict(form='ring', nsub=2, tpw=1, vecw=0), 'HW % 4 == 2 and 4096 waves: two pixels per lane')
_c('ring_nsub2_x_off', (2, 288, 80, 16, 1, 4066), dict(form='ring', nsub=1), 'the same with x 4 bytes off: one pixel per lane', (AFFINE,), x_off=1)
_c('ring_nsub4', (2, 288, 80, 16, 1, 8192), dict(form='ring', nsub=4, tpw=1), 'HW % 4 == 0 and 2048 waves of 128 pixels: four pixels per lane')
_c('ring_tpw2', (2, 288, 16, 16, 1, 16369),dict(form='ring', nsub=1, tpw=2, mb=32, grid_x=16 * 128), '16384 wave tiles: two per wave', (AFFINE,))
_c('ring_k768_m48', (2, 768, 48, 1, 5, 7), None, 'K = 768 with more than 32 rows: a 32-row tile of 769 + 6 columns exceeds 96 KiB', (AFFINE,),
   refused=nv.ERR_UNSUPPORTED)
_c('ring_k1024_m64', (2, 1024, 64, 1, 1, 32), None, 'K = 1024 ungrouped beyond split-K', (AFFINE,), refused=nv.ERR_UNSUPPORTED)
_c('sk_k768_m10', (2, 768, 10, 1, 5, 7), dict(form='split_k', ch=16, ks=192), 'K = 768 with few rows is split-K', SK_TERMS)
_c('sk_k1024_m32', (2, 1024, 32, 1, 1, 33), dict(form='split_k', ch=16, ks=256), 'K = 1024 with few rows is split-K', SK_TERMS)

# ---------------------------------------------------------------------------------------------------------------- small-K vector
# K < 16 or odd K, all weights in LDS (<= 48 KiB).  MT = 2 / 4 / 8 rows per thread, mtiles = ceil(M / MT) row tiles; four pixels per
# thread, 16-byte accesses when HW % 4 == 0; grid y/z = (image, group, row tile) slabs, split over z past 65535.
for K, M, G, hw in ((1, 1, 3, (3, 4)), (3, 2, 1, (5, 7)), (5, 3, 2, (3, 7)), (8, 4, 4, (5, 7)), (12, 5, 2, (4, 8)), (15, 8, 1, (5, 7)),
                    (17, 9, 2, (3, 5)), (33, 13, 1, (4, 8)), (3, 128, 1, (5, 7))):
    mt = 2 if M <= 2 else 4 if M <= 4 else 8
    _c('small_k%d_m%d' % (K, M), (2, K * G, M * G, G) + hw, dict(form='small_k', mt=mt, mtiles=-(-M // mt), lds_bytes=4 * K * M * G),
       'vector unit, HW %% 4 = %d' % (hw[0] * hw[1] % 4))
_c('small_slice', (2, 16, 26, 2, 5, 7), dict(form='small_k', mt=8, mtiles=2), 'two row tiles, the second with 5 rows, into a channel slice', ctot=30, coff=3)
_c('small_slabs_over_65535', (6, 12288, 12288, 12288, 1, 3), dict(form='small_k', mt=2, grid_y=65535, grid_z=2), '73728 slabs: the grid splits over y and z',
   (AFFINE,))
_c('small_odd_k_over_48k', (2, 33, 400, 1, 5, 7), None, 'odd K whose weights (52800 B) exceed 48 KiB: refused, nothing launched', (AFFINE,),
   refused=nv.ERR_UNSUPPORTED)

# ---------------------------------------------------------------------------------------------------------------- thin
# M <= 16 per group, K in 8..64 (multiple of 8), HW % 4 == 0, N * groups * ceil(HW/4 / 256) >= 400 workgroups, everything 16-byte aligned.
_c('thin_k8_m1', (50, 64, 8, 8, 1, 4), dict(form='thin', mt=8, grid_x=1, grid_y=400), 'exactly 400 workgroups', (AFFINE, RAW, ALL))
_c('thin_not_399', (57, 56, 7, 7, 1, 4), dict(form='small_k'), '399 workgroups: not thin (K = 8: vector unit)')
_c('thin_k64_m8', (50, 512, 64, 8, 1, 4), dict(form='thin', mt=8, lds_bytes=8 * 64 * 8 * 4), 'K = 64, all 8 rows of the instantiation')
_c('thin_k64_m9_not_392', (49, 512, 72, 8, 1, 4), dict(form='pipe', ng=8), '392 workgroups: not thin (K = 64 grouped: tile-pipelined)')
_c('thin_k8_m9_q256', (25, 128, 144, 16, 1, 1024), dict(form='thin', mt=16, grid_x=1, grid_y=400), '256 pixel quads: one column block', (AFFINE, ALL))
_c('thin_k24_m16_q257', (25, 192, 128, 8, 1, 1028), dict(form='thin', mt=16, grid_x=2, grid_y=200), '257 pixel quads: a second column block with one quad',
   (AFFINE, ALL), leaves=())
_c('thin_not_q256', (25, 192, 128, 8, 1, 1024), dict(form='pipe', ng=3), 'the same with 256 quads: 200 workgroups, not thin', (AFFINE,))
_c('thin_operand_misaligned', (50, 64, 8, 8, 1, 4), dict(form='thin'), 'a residual 4 bytes off a 16-byte boundary leaves the form', (AFFINE,),
   leaves=(AFFINE | {'residual'},), op_off=1)
_c('thin_slice', (50, 64, 72, 8, 1, 4), dict(form='thin', mt=16), 'thin into a channel slice', ctot=80, coff=5)

# ---------------------------------------------------------------------------------------------------------------- the models
# (Cin, Cout, groups) of every 1x1 convolution the segmentation networks of mspl_amd/models.py send through ops.conv1x1, at every
# width multiplier, both decoder widths and 5 / 21 classes (tests/test_conv1x1_cases.py rebuilds the set), with the form each takes
# on a 5 x 7 map at batch 2.  The fusion gate's 2c -> c convolution runs as two c -> c halves; level 4's whole (1024 -> 512) is
# refused (the training path uses the halves there too).
MODEL_SHAPES = [
    (2, 5, 1, 'small_k'), (2, 32, 1, 'small_k'), (2, 48, 1, 'small_k'), (2, 64, 1, 'small_k'), (2, 96, 1, 'small_k'),
    (2, 128, 1, 'small_k'), (3, 32, 1, 'small_k'), (3, 64, 1, 'small_k'), (3, 80, 1, 'small_k'), (3, 96, 1, 'small_k'),
    (3, 128, 1, 'small_k'), (3, 160, 1, 'small_k'), (3, 192, 1, 'small_k'), (3, 256, 1, 'small_k'), (3, 320, 1, 'small_k'),
    (3, 384, 1, 'small_k'), (3, 512, 1, 'small_k'), (10, 21, 1, 'small_k'), (10, 32, 1, 'small_k'), (10, 48, 1, 'small_k'),
    (10, 64, 1, 'small_k'), (10, 96, 1, 'small_k'), (10, 128, 1, 'small_k'), (16, 5, 1, 'pipe'), (16, 21, 1, 'pipe'),
    (16, 32, 1, 'pipe'), (16, 48, 1, 'pipe'), (16, 64, 1, 'pipe'), (32, 2, 1, 'pipe'), (32, 5, 1, 'pipe'), (32, 10, 1, 'pipe'),
    (32, 16, 1, 'pipe'), (32, 21, 1, 'pipe'), (32, 32, 1, 'pipe'), (32, 64, 1, 'pipe'), (32, 96, 1, 'pipe'),
    (32, 128, 1, 'pipe'), (48, 2, 1, 'pipe'), (48, 10, 1, 'pipe'), (48, 16, 1, 'pipe'), (64, 2, 1, 'split_k'),
    (64, 10, 1, 'split_k'), (64, 16, 1, 'split_k'), (64, 32, 1, 'pipe'), (96, 2, 1, 'pipe'), (96, 10, 1, 'pipe'),
    (96, 32, 1, 'pipe'), (128, 2, 1, 'split_k'), (128, 10, 1, 'split_k'), (128, 16, 1, 'split_k'), (128, 32, 1, 'split_k'),
    (128, 128, 1, 'pipe'), (256, 2, 1, 'split_k'), (256, 10, 1, 'split_k'), (256, 16, 1, 'split_k'), (256, 32, 1, 'split_k'),
    (256, 128, 1, 'ring'), (256, 256, 1, 'ring'), (320, 2, 1, 'split_k'), (320, 10, 1, 'split_k'), (320, 16, 1, 'split_k'),
    (320, 32, 1, 'split_k'), (384, 2, 1, 'split_k'), (384, 10, 1, 'split_k'), (384, 16, 1, 'split_k'), (384, 32, 1, 'split_k'),
    (512, 2, 1, 'split_k'), (512, 10, 1, 'split_k'), (512, 16, 1, 'split_k'), (512, 32, 1, 'split_k'), (512, 256, 1, 'ring'),
    (512, 512, 1, 'ring'), (1024, 512, 1, 'refused'), (16, 4, 4, 'small_k'), (16, 16, 4, 'small_k'), (32, 8, 4, 'small_k'),
    (32, 12, 4, 'small_k'), (32, 16, 4, 'small_k'), (32, 24, 4, 'small_k'), (32, 32, 4, 'small_k'), (48, 48, 4, 'small_k'),
    (64, 16, 4, 'pipe'), (64, 64, 4, 'pipe'), (80, 20, 4, 'ring'), (80, 80, 4, 'ring'), (96, 24, 4, 'pipe'), (96, 96, 4, 'pipe'),
    (128, 32, 4, 'pipe'), (128, 128, 4, 'pipe'), (160, 40, 4, 'ring'), (160, 160, 4, 'ring'), (192, 48, 4, 'pipe'),
    (192, 192, 4, 'pipe'), (256, 64, 4, 'pipe'), (256, 256, 4, 'pipe'), (320, 80, 4, 'ring'), (320, 320, 4, 'ring'),
    (384, 96, 4, 'pipe'), (384, 384, 4, 'pipe'), (512, 128, 4, 'pipe'), (512, 512, 4, 'pipe'),
]
for cin, cout, g, form in MODEL_SHAPES:
    _c('model_%d_%d_g%d' % (cin, cout, g), (2, cin, cout, g, 5, 7), None if form == 'refused' else form, 'a 1x1 convolution of the networks',
       (AFFINE,), refused=nv.ERR_UNSUPPORTED if form == 'refused' else None)

NAMES = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
# one random-data pass per form, at the standing tolerance of tests/epilogue_cases.py
RANDOM = ('thin_k24_m16_q257', 'small_k15_m8', 'sk_k192_m10', 'pipe_ng12_m96_even', 'ring_k80_m20')


# ------------------------------------------------------------------------------------------------------------------ the plan
def plan(case, terms=frozenset()):
    """What the library plans for the case's call with these terms (raises what the launcher raises)."""
    N, Cin, Cout, G, H, W = case.shape
    off = lambda o: 4 if o else 16                                             # noqa: E731
    return ops.conv1x1_plan((N, Cin, Cout, G, H * W), terms=sorted(terms), ctot=case.ctot, x_align=off(case.x_off), w_align=off(case.w_off),
                            out_align=off(case.out_off), operand_align=off(case.op_off and terms & OPERAND_TERMS))


# ------------------------------------------------------------------------------------------------------------------ data
def _seed(case):
    return 1000 * NAMES.index(case.name) + 17


@functools.lru_cache(maxsize=2)
def inputs(name):
    """(x, w) in float64: integers from VALS, different per image and per row."""
    case = BY_NAME[name]
    N, Cin, Cout, G, H, W = case.shape
    s = _seed(case)
    return draw((N, Cin, H, W), s), draw((Cout, Cin // G, 1, 1), s + 1)


@functools.lru_cache(maxsize=2)
def operands(name):
    """Every epilogue operand in the geometry of the destination (ctot channels), float64."""
    case = BY_NAME[name]
    N, Cin, Cout, G, H, W = case.shape
    ctot, s = case.ctot or Cout, _seed(case)
    return {'scale': draw(ctot, s + 2, SCALES), 'shift': draw(ctot, s + 3, SHIFTS), 'alpha': draw(ctot, s + 4, SLOPES),
            'pre_add': draw((N, ctot, H, W), s + 5), 'residual': draw((N, ctot, H, W), s + 6), 'reinf_r': draw((N, 3, H, W), s + 7),
            'reinf_w': draw((ctot, 3), s + 8), 'gate': draw((N, ctot), s + 9, SCALES)}


def select(t, terms):
    keep = (set(terms) - {'reinf', 'raw_out'}) | ({'reinf_r', 'reinf_w'} if 'reinf' in terms else set())
    return {k: v for k, v in t.items() if k in keep}


def accumulate(case, dtype=torch.float64, magnitude=False):
    """The bare convolution in `dtype` (what raw_out receives); magnitude: on the absolute values."""
    x, w = inputs(case.name)
    if magnitude:
        x, w = x.abs(), w.abs()
    return F.conv2d(x.to(dtype), w.to(dtype), None, 1, 0, 1, case.shape[3])


def reference(case, acc, terms, magnitude=False):
    """The destination slice for a term set, in the dtype of `acc`."""
    t = select(operands(case.name), terms)
    if magnitude:
        t = {k: v.abs() for k, v in t.items()}
    return ref_epilogue(acc, t, case.coff)


def random_problem(name, terms):
    """Seeded randn inputs with fan-in-scaled weights and the operands of tests/epilogue_cases.py for the shape of a case."""
    from tests import epilogue_cases as ec
    case = BY_NAME[name]
    N, Cin, Cout, G, H, W = case.shape
    inp = ec.make_inputs('conv1x1', case.shape, _seed(case))
    t = ec.make_operands(N, Cout, H, W, terms, _seed(case))
    return inp, t
