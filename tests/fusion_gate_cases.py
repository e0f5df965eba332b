"""Cases for the one-launch fusion gate (mspl_fusion_gate_conv_fwd / _bwd_weight): per channel count of the four gates of the s=2.0
network, the smallest shapes that hit every seam the two plan queries report.  Shared by tests/test_fusion_gate_cases.py (no GPU:
the table against the plans) and tests/test_gpu_fusion_gate_conv.py (the kernels).  Nothing here touches the code under test but
the plan queries (ops.fusion_gate_conv_plan / _bwd_weight_plan: the host functions the launchers themselves call).

Forward (plan: rows, pixels, wave_pixels): a workgroup owns `rows` output rows (two 32-row chunks on two waves when rows == 64) of
`pixels` consecutive pixels of the flattened (image, pixel) axis, a wave `wave_pixels` of them.  Seams:
    tail      N * HW % wave_pixels != 0: the last wave tile is partial;
    idle      the last workgroup along the pixels has a wave with no tile at all (it still stages and meets the barriers);
    image     N = 2 and HW % wave_pixels != 0: an image boundary inside a wave tile;
    rows      C > rows: more than one row block -- the row-chunk seam (C = 32 has one block of 32 rows: no such seam);
    source    k = C - 1 | C, the switch from rgb to depth: in every case; the data differ per channel and per source.
Weight gradient (plan: parts, ngroups): `parts` waves share a pair of 32x32 tiles, wave s takes the 64-pixel groups s, s + parts, ...
    spare     parts > ngroups: slots with no group (parts is rounded up to a multiple of 4);
    stride    ngroups > parts: a wave takes a second group `parts` further on, and ngroups % parts != 0: the last round is partial;
    group     HW % 64 != 0: the last group of an image is partial and the next group starts the next image.
Scalar form (plan form 2, HW % 4 != 0 and N * HW <= 4096 -- level 4 of a 32x48 input, 2 x 3 pixels): one thread per element.
    scalar    the form itself, with N = 2 (the image stride) and more elements than one workgroup of 256 threads;
    limit     N * HW = 4096 exactly, the last size the form takes (one case: the limit does not depend on C).

Integer data: rgb, depth and gz from {-4..4}, weights k/8 with k in {-8..8}; every product is a multiple of 1/8 and every sum stays
far below 2^24 in units of 1/8 (z: 2 * 512 * 4 * 8 = 2^15; gw: N * HW * 16 <= 3.2e6 for the largest case), so z and gw must EQUAL
the float64 reference whatever the order of the sums.
"""
import collections
import functools

import torch

from mspl_amd import ops

Case = collections.namedtuple('Case', 'name N C H W why')
CHANNELS = (32, 128, 256, 512)

CASES = [
    # one partial wave tile that holds both images; two 64-pixel groups on four slots
    Case('c32_small', 2, 32, 6, 6, 'tail, image, spare, group'),
    Case('c128_small', 2, 128, 6, 6, 'tail, image, spare, group, rows'),
    Case('c256_small', 2, 256, 6, 6, 'tail, image, spare, group, rows'),
    Case('c512_small', 2, 512, 6, 6, 'tail, image, spare, group, rows'),
    # more 64-pixel groups than waves per tile pair (3072 / (C/32)^2 waves), several workgroups along the pixels
    Case('c32_stride', 7, 32, 1, 28036, 'stride (3073 groups on 3072 waves), tail, idle, group'),
    Case('c128_stride', 2, 128, 1, 6148, 'stride (194 groups on 192 waves), tail, idle, image, group, rows'),
    Case('c256_stride', 2, 256, 1, 1540, 'stride (50 groups on 48 waves), tail, idle, image, group, rows'),
    Case('c512_stride', 2, 512, 1, 420, 'stride (14 groups on 12 waves), tail, idle, image, group, rows'),
    # level 4 of a 32x48 input
    Case('c32_scalar', 2, 32, 2, 3, 'scalar'),
    Case('c128_scalar', 2, 128, 2, 3, 'scalar'),
    Case('c256_scalar', 2, 256, 2, 3, 'scalar'),
    Case('c512_scalar', 2, 512, 2, 3, 'scalar'),
    Case('c32_scalar_limit', 2048, 32, 1, 2, 'scalar, limit'),
]
SCALAR_MAX_PX = 4096
NAMES = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}

# shapes the node declines (mspl_fusion_gate_conv_fits == 0): planes that are no multiple of 4 pixels above the scalar form's limit,
# channel counts off the 32-row tile or above 512
DECLINED = [(1, 32, 4097), (2, 32, 2049), (3, 512, 1366), (2, 48, 16), (2, 48, 6), (1, 16, 64), (1, 544, 16), (1, 1024, 16)]


def seams(case):
    """The seams of the module docstring a case hits, from the two plans."""
    fp = ops.fusion_gate_conv_plan(case.N, case.C, case.H * case.W)
    wp = ops.fusion_gate_conv_bwd_weight_plan(case.N, case.C, case.H * case.W)
    assert fp is not None and wp is not None, case
    hw, total = case.H * case.W, case.N * case.H * case.W
    if fp['form'] == 2:
        assert wp['form'] == 2 and hw % 4 and total <= SCALAR_MAX_PX
        return ({'scalar'} if case.N >= 2 and total * case.C > 256 else set()) | ({'limit'} if total == SCALAR_MAX_PX else set())
    wpx, px = fp['wave_pixels'], fp['pixels']
    got = {'source'}
    if total % wpx:
        got.add('tail')
    ptiles = -(-total // wpx)
    if ptiles % (px // wpx):
        got.add('idle')
    if case.N >= 2 and hw % wpx:
        got.add('image')
    if case.C > fp['rows']:
        got.add('rows')
    if wp['parts'] > wp['ngroups']:
        got.add('spare')
    if wp['ngroups'] > wp['parts'] and wp['ngroups'] % wp['parts']:
        got.add('stride')
    if hw % 64:
        got.add('group')
    return got


def reported_seams(C):
    """Every seam the plans can report for C channels (the row seam exists only where a row block is smaller than C)."""
    fp = ops.fusion_gate_conv_plan(2, C, 64)
    all_ = {'source', 'tail', 'idle', 'image', 'spare', 'stride', 'group', 'scalar'}
    return all_ | ({'rows'} if C > fp['rows'] else set()) | ({'limit'} if C == CHANNELS[0] else set())


def _draw(shape, seed, lo, hi):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).double()


@functools.lru_cache(maxsize=2)
def integer_problem(name):
    """rgb, depth, w (C, 2C), gz, gw0 (the non-zero start of the accumulate = 1 check) in float64, and the float64 z and gw."""
    c = BY_NAME[name]
    s = 100 * NAMES.index(name) + 7
    shape = (c.N, c.C, c.H, c.W)
    rgb, depth, gz = _draw(shape, s, -4, 4), _draw(shape, s + 1, -4, 4), _draw(shape, s + 2, -4, 4)
    w = _draw((c.C, 2 * c.C), s + 3, -8, 8) / 8
    gw0 = _draw((c.C, 2 * c.C), s + 4, -4, 4)
    cat = torch.cat((rgb, depth), 1).flatten(2)                       # (N, 2C, HW)
    z = torch.einsum('mk,nkp->nmp', w, cat).reshape(shape)
    gw = torch.einsum('nmp,nkp->mk', gz.flatten(2), cat)
    return dict(rgb=rgb, depth=depth, w=w, gz=gz, gw0=gw0, z=z, gw=gw)


def random_problem(name):
    """Seeded random rgb, depth, upstream gradient and a fan-in scaled weight (C, 2C, 1, 1), float64."""
    c = BY_NAME[name]
    g = torch.Generator().manual_seed(500 + NAMES.index(name))
    shape = (c.N, c.C, c.H, c.W)
    rgb = torch.randn(shape, generator=g, dtype=torch.float64)
    depth = torch.randn(shape, generator=g, dtype=torch.float64)
    gy = torch.randn(shape, generator=g, dtype=torch.float64)
    w = torch.randn((c.C, 2 * c.C, 1, 1), generator=g, dtype=torch.float64) * (2.0 / (2 * c.C)) ** 0.5
    return rgb, depth, w, gy
