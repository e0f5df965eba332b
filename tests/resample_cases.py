"""Cases for the backward kernels of the resampling family and of the pyramid's training path, each at the kernel form and the
seam (tile, column block, row segment, thread, grid wrap) it exists for, with float64 references in plain torch.

Shared by tests/test_resample_cases.py (CPU: the library's plan queries confirm form and seam, the probe sets are valid, the float32
CPU evaluation of every reference is finite and its gap to float64 is recorded) and tests/test_gpu_resample_grad.py /
tests/test_gpu_pyramid_grad.py (the kernels).

Two kinds of check use this table.

Operator probes (bilinear, adaptive_avgpool, avgpool3x3s2, two_head_sum): the operation is linear, y = A x, so one-hot inputs read
A's columns off the forward and one-hot output gradients read A's rows off the backward -- with ONE term per element, so no
summation order exists and the backward must hold the forward's own weights bit for bit.  Forward probes use the full basis.  The
backward uses the full basis while Ho * Wo <= FULL_BASIS, coloured probes beyond: A is separable (A = Ay (x) Ax), outputs are
coloured per axis so that two outputs of one colour have disjoint receivers, a plane carries one (row colour, column colour)
pair.  Receivers are taken from the float64 operator and widened by one input on each side (float32 may place a weight of 1e-7
where float64 has an exact zero); everything a plane writes outside its receivers must be exactly 0.

Dense random data against float64: per plane, |kernel - float64| <= MARGIN * max(err32, 2^-23 * M), err32 = the largest gap of
the float32 CPU evaluation of the same reference on that plane, M = the reference on the absolute values of all operands
(largest element of the plane).
"""
import collections
import ctypes
import functools
import math

import torch
import torch.nn.functional as F

from mspl_amd import _native as nv
from tests import exact_cases as ec

MARGIN = 4.0                       # tests/test_gpu_bn_conditioning.py, tests/test_gpu_confident_logits.py
EPS = 2.0 ** -23
FULL_BASIS = 4096

BIL = {nv.BILINEAR_BWD_GENERIC8: 'generic8', nv.BILINEAR_BWD_GENERIC12: 'generic12', nv.BILINEAR_BWD_TILE8: 'tile8',
       nv.BILINEAR_BWD_TILE12: 'tile12', nv.BILINEAR_BWD_WAVE: 'wave', nv.BILINEAR_BWD_ROWS: 'rows'}
AVG = {nv.AVGPOOL_BWD_VEC: 'vec', nv.AVGPOOL_BWD_PLAIN: 'plain'}
BRANCH = {nv.PYR_BRANCH_BWD_STREAM3: 'stream3', nv.PYR_BRANCH_BWD_STREAM: 'stream', nv.PYR_BRANCH_BWD_TILE: 'tile',
          nv.PYR_BRANCH_BWD_UNSUPPORTED: 'unsupported'}

Case = collections.namedtuple('Case', 'op id shape form where cfg')


def _ints(n):
    return [ctypes.c_int32() for _ in range(n)]


# ------------------------------------------------------------------------------------------------------------------ plan queries
def bilinear_plan(planes, Hi, Wi, Ho, Wo):
    """(form name, tiles_x, tiles_y, FH, FW) of mspl_bilinear_bwd, from the library."""
    f, tx, ty, fh, fw = _ints(5)
    nv.check(nv.lib.mspl_bilinear_bwd_plan(1, planes, Hi, Wi, Ho, Wo, 1, *[ctypes.byref(v) for v in (f, tx, ty, fh, fw)]))
    return BIL[f.value], tx.value, ty.value, fh.value, fw.value


def avgpool_plan(planes, H, W, aligned16=True):
    f = ctypes.c_int32()
    nv.check(nv.lib.mspl_avgpool3x3s2_bwd_plan(1, planes, H, W, int(aligned16), ctypes.byref(f)))
    return AVG[f.value]


BranchPlan = collections.namedtuple('BranchPlan', 'form ncb nseg seg taps tiles_x tiles_y')


def branch_plan(N, P, h, w, sizes, aligned8=True):
    nb = len(sizes)
    hs, ws = (ctypes.c_int32 * nb)(*[s[0] for s in sizes]), (ctypes.c_int32 * nb)(*[s[1] for s in sizes])
    f, ncb, nseg, seg, tx, ty = _ints(6)
    taps = (ctypes.c_int32 * 3)()
    nv.check(nv.lib.mspl_pyrpool_branch_bwd_plan(N, P, h, w, nb, hs, ws, int(aligned8), ctypes.byref(f), ctypes.byref(ncb),
                                                 ctypes.byref(nseg), ctypes.byref(seg), taps, ctypes.byref(tx), ctypes.byref(ty)))
    return BranchPlan(BRANCH[f.value], ncb.value, nseg.value, seg.value, tuple(taps), tx.value, ty.value)


def branch_fits(N, P, h, w, sizes):
    nb = len(sizes)
    hs, ws = (ctypes.c_int32 * nb)(*[s[0] for s in sizes]), (ctypes.c_int32 * nb)(*[s[1] for s in sizes])
    return bool(nv.lib.mspl_pyrpool_branch_bwd_fits(N, P, h, w, nb, hs, ws))


def branch_sizes(h, w, scales):
    """EfficientPyrPool.branch_sizes: ceil(size * scale), at least 5."""
    return [(max(int(math.ceil(h * s)), 5), max(int(math.ceil(w * s)), 5)) for s in scales]


# ------------------------------------------------------------------------------------------------------------------ the table
CASES = []


def _add(op, cid, shape, form, where, **cfg):
    CASES.append(Case(op, '%s-%s' % (op, cid), tuple(shape), form, where, cfg))


# bilinear backward: (planes, Hi, Wi, Ho, Wo).  `form` is what mspl_bilinear_bwd_plan must answer.
for _form, _hw, _where in [
        ('tile8', (8, 64, 16, 128), 'one full tile'),
        ('tile8', (8, 65, 16, 130), 'a one-column tile'),
        ('tile8', (9, 70, 18, 140), 'ragged tile in both directions'),
        ('tile8', (17, 33, 29, 57), 'non-integer ratio, three row tiles'),
        ('tile8', (30, 40, 20, 25), 'down-scaling'),
        # x4 as listed: 2 / (4/19) + 3 = 12.5 row candidates, past the tile form's 12 -> the per-thread form with the candidate loop
        ('generic12', (5, 66, 20, 264), 'x4 with a row window of 12.5: not tiled, column window above MAXC'),
        ('tile12', (6, 66, 21, 261), 'x4 with row and column windows of 11'),
        ('tile12', (6, 70, 18, 210), 'x3, two tiles each way'),
        ('generic8', (5, 9, 1, 18), 'Ho = 1: sh = 0, every output row is a candidate'),
        ('generic8', (3, 20, 30, 40), 'row window above 12, column window at most 8'),
        ('generic12', (3, 20, 30, 80), 'row window above 12, column window at most 12'),
        ('rows', (3, 5, 30, 50), 'column window above 12'),
        ('rows', (13, 24, 20, 300), 'more output columns than threads'),
        ('rows', (6, 7, 12, 1), 'Wo = 1: sw = 0'),
        ('wave', (2, 3, 2, 8193), 'Wo > 8192'),
        ('tile8', (5, 6, 5, 6), 'identity'),
        ('tile8', (40, 64, 16, 32), 'ratio 39/15, which float32 cannot hold (tests/epilogue_cases.py)'),
        ('tile8', (33, 47, 66, 94), 'ratios 32/65 and 46/93, which float32 cannot hold (tests/epilogue_cases.py)')]:
    _add('bilinear', '%dx%d-%dx%d' % _hw, (3,) + _hw, _form, _where, forward_refused=_form == 'wave')
_add('bilinear', 'wrap-tile', (65537, 2, 2, 3, 3), 'tile8', 'gyd = 65535 grid wrap, tile form')
_add('bilinear', 'wrap-generic', (65537, 2, 3, 1, 6), 'generic8', 'gyd = 65535 grid wrap, per-thread form')

# avgpool3x3s2 backward: (planes, H, W)
for _form, _hw in [('vec', (2, 8)), ('vec', (6, 8)), ('vec', (16, 24)), ('plain', (15, 21)), ('plain', (16, 20)), ('plain', (1, 7)),
                   ('plain', (7, 1))]:
    _add('avgpool', '%dx%d' % _hw, (3,) + _hw, _form, 'H even and W % 8 == 0' if _form == 'vec' else 'odd H or W % 8 != 0')
_add('avgpool', '6x8-misaligned', (3, 6, 8), 'plain', 'gy one float into a larger buffer: the launcher falls back', misalign=True)
_add('avgpool', 'wrap', (65537, 2, 8), 'vec', 'gyd = 65535 grid wrap')

# adaptive_avgpool backward: (planes, Hi, Wi, Ho, Wo)
for _hw, _where in [((15, 21, 5, 5), 'windows of 3x5'), ((15, 21, 10, 14), 'overlapping windows'), ((15, 21, 30, 42), 'enlarging x2'),
                    ((15, 21, 22, 31), 'enlarging, ragged'), ((15, 21, 1, 1), 'global'), ((7, 9, 7, 9), 'identity'),
                    ((31, 37, 13, 11), 'prime sizes for the magic-number divisions'), ((40, 60, 5, 6), 'windows of 8x10')]:
    _add('adaptive', '%dx%d-%dx%d' % _hw, (3,) + _hw, None, _where)

# two_head_sum: (planes, Hm, Wm, Ha, Wa, H, W); form = (main's, aux's)
_add('two_head', '16x24+8x12-32x48', (2, 16, 24, 8, 12, 32, 48), ('tile8', 'tile12'), 'the supervised loop: x2 and x4')
_add('two_head', '3x5+6x10-30x50', (2, 6, 10, 3, 5, 30, 50), ('rows', 'rows'), 'aux head (3x5) on the rows form; so is the main head')

# pyrpool_merge_bwd: (N, P, h, w, nb)
for _shape, _where in [((1, 4, 16, 64, 5), 'one tile'), ((1, 4, 17, 65, 5), 'a one-row band and a one-column tile'),
                       ((2, 3, 33, 130, 3), 'three bands, three tiles'), ((1, 2, 9, 67, 2), 'w % 4 != 0'), ((1, 1, 5, 6, 1), 'small'),
                       ((1, 2, 17, 65, 4), 'nb = 4')]:
    for _al in (1, 0):
        for _mi in (0, 1):
            _add('pyr_merge', '%dx%dx%dx%d-nb%d-alpha%d-mean%d' % (_shape + (_al, _mi)), _shape, None, _where, m_alpha=bool(_al),
                 mean_inv=bool(_mi))

# pyrpool_branch_bwd: (N, P, h, w), scales; adds = how many of add0 / add1 are given
U3 = (2.0, 1.5, 1.0)
for _cid, _shape, _scales, _form, _where, _kw in [
        ('two-blocks', (1, 4, 17, 126), U3, 'stream3', 'two column blocks, the last 2 wide; row segments', dict(adds=2, ncb=2, nseg_min=2)),
        ('one-block', (1, 4, 9, 124), U3, 'stream3', 'exactly one column block', dict(adds=1, ncb=1)),
        ('three-blocks', (1, 8, 20, 250), U3, 'stream3', 'three column blocks', dict(adds=0, ncb=3, nseg_min=2)),
        ('seg19', (4, 256, 38, 4), (2.0, 1.0), 'stream3', 'full-length segments', dict(adds=2, seg=19, nseg=2)),
        ('nup1', (1, 4, 10, 12), (2.0,), 'stream3', 'one up branch', dict(adds=1)),
        ('nup1-same', (1, 4, 10, 12), (2.0, 1.0), 'stream3', 'one up branch and the same-size one', dict(adds=0)),
        ('stream-three-up', (1, 4, 10, 12), (3.0, 2.0, 1.5), 'stream', 'three up branches: the first launch overwrites', dict(adds=2)),
        ('stream-same-first', (1, 4, 10, 12), (1.0, 2.0), 'stream', 'the same-size branch first', dict(adds=1)),
        ('stream-blocks', (1, 4, 17, 126), (1.0, 2.0), 'stream', 'two column blocks in the per-branch form', dict(adds=0, ncb=2)),
        ('tile-odd-w', (1, 4, 17, 33), U3, 'tile', 'odd w: two tiles each way', dict(adds=2, tiles=(2, 2))),
        ('tile-planes3', (1, 3, 16, 34), U3, 'tile', 'N * P % 4 != 0; columns 32, 33 in a second tile', dict(adds=1, tiles=(2, 1))),
        ('tile-planes15', (3, 5, 17, 32), (2.0, 1.5), 'tile', 'N * P % 4 != 0; row 16 in a second band', dict(adds=0, tiles=(1, 2))),
        ('tile-misaligned', (1, 4, 10, 12), U3, 'tile', 'gx one float into a larger buffer, on a streaming shape', dict(adds=1, misalign=True)),
        ('tile-three-up', (1, 3, 10, 12), (2.0, 1.5, 1.25), 'tile', 'three up branches (with 2.5 the tile leaves LDS)', dict(adds=0)),
        # ceil(3.0 * h) - 1 > 3 * (h - 1) for every h: a 3.0 branch is never tiled
        ('three-up-3x', (1, 3, 10, 12), (3.0, 2.0, 1.5), 'unsupported', 'three up branches, one of them 3.0, N * P % 4 != 0', dict(adds=0)),
        ('refused', (1, 2, 6, 7), (3.0,), 'unsupported', 'ceil(6 * 3) - 1 = 17 > 3 * 5: more than 3x', dict(adds=0))]:
    _add('pyr_branch', _cid, _shape, _form, _where, scales=_scales, **_kw)
for _t, _scales in [((3, 3), (3.0, 2.0)), ((5, 5), (1.5, 1.25)), ((5, 3), (1.5, 2.0)), ((3, 5), (2.0, 1.5))]:
    for _same in (0, 1):
        _add('pyr_branch', 'taps%d%d-same%d' % (_t + (_same,)), (1, 4, 10, 12), 'stream3', 'tap pair %d, %d' % _t,
             scales=_scales + ((1.0,) if _same else ()), taps=_t, adds=_same)

BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
LINEAR = ('bilinear', 'avgpool', 'adaptive', 'two_head')


def sizes_of(case):
    N, P, h, w = case.shape
    return branch_sizes(h, w, case.cfg['scales'])


def plan(case):
    """What the library says this case reaches (the form name; two_head: a pair; adaptive / pyr_merge have one form: None)."""
    if case.op == 'bilinear':
        return bilinear_plan(*case.shape)[0]
    if case.op == 'avgpool':
        return avgpool_plan(*case.shape, aligned16=not case.cfg.get('misalign'))
    if case.op == 'two_head':
        pl, Hm, Wm, Ha, Wa, H, W = case.shape
        return bilinear_plan(pl, Hm, Wm, H, W)[0], bilinear_plan(pl, Ha, Wa, H, W)[0]
    if case.op == 'pyr_branch':
        return branch_plan(*case.shape, sizes_of(case), aligned8=not case.cfg.get('misalign')).form
    return None


# ------------------------------------------------------------------------------------------------------------------ operations
def up(x, size):
    return F.interpolate(x, tuple(size), mode='bilinear', align_corners=True)


def linear_op(case, *xs):
    """The forward operation on (1, planes, ...) tensors."""
    s = case.shape
    if case.op == 'bilinear':
        return up(xs[0], s[3:5])
    if case.op == 'avgpool':
        return F.avg_pool2d(xs[0], 3, 2, 1)
    if case.op == 'adaptive':
        return F.adaptive_avg_pool2d(xs[0], s[3:5])
    if case.op == 'two_head':
        return up(xs[0], s[5:7]) + 0.5 * up(xs[1], s[5:7])
    raise KeyError(case.op)


def in_shapes(case):
    s = case.shape
    return [(s[1], s[2]), (s[3], s[4])] if case.op == 'two_head' else [(s[1], s[2])]


def out_shape(case):
    s = case.shape
    if case.op == 'avgpool':
        return (s[1] - 1) // 2 + 1, (s[2] - 1) // 2 + 1
    return tuple(s[5:7]) if case.op == 'two_head' else tuple(s[3:5])


def _rn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def branch_value(x, w, size, P):
    """One pyramid branch with hs >= h: adaptive_avg_pool2d(dw3x3(bilinear_up(x)))."""
    return F.adaptive_avg_pool2d(F.conv2d(up(x, size), w, None, 1, 1, 1, P), x.shape[2:])


def make(case):
    """The case's operands (float32 values, CPU)."""
    s = case.shape
    if case.op in LINEAR:
        p = {'gy': _rn(2, 1, s[0], *out_shape(case))}
        for k, hw in enumerate(in_shapes(case)):
            p['x%d' % k] = _rn(10 + k, 1, s[0], *hw)
        return p
    if case.op == 'pyr_merge':
        N, P, h, w, nb = s
        p = {'zcat': _rn(1, N, nb * P, h, w), 'gy': _rn(2, N, P, h, w), 'merge_w': 0.4 * _rn(3, P, nb, 3, 3)}
        for pre, C, seed in (('br_', nb * P, 20), ('m_', P, 30)):
            p[pre + 'scale'], p[pre + 'shift'] = 0.5 + torch.rand(C, generator=torch.Generator().manual_seed(seed)), 0.3 * _rn(seed + 1, C)
            p[pre + 'alpha'] = 0.1 + 0.4 * torch.rand(C, generator=torch.Generator().manual_seed(seed + 2))
            if case.cfg['mean_inv']:
                p[pre + 'mean'], p[pre + 'inv'] = 0.3 * _rn(seed + 3, C), 0.5 + torch.rand(C, generator=torch.Generator().manual_seed(seed + 4))
        if not case.cfg['m_alpha']:
            del p['m_alpha']
        p['mraw'] = ec.merge_conv(p, s, torch.float64).float()
        return p
    if case.op == 'pyr_branch':
        N, P, h, w = s
        p = {'x': _rn(1, N, P, h, w)}
        for i in range(len(case.cfg['scales'])):
            p['w%d' % i], p['gt%d' % i] = 0.4 * _rn(20 + i, P, 1, 3, 3), _rn(30 + i, N, P, h, w)
        for k in range(case.cfg['adds']):
            p['add%d' % k] = _rn(40 + k, N, P, h, w)
        return p
    raise KeyError(case.op)


@functools.lru_cache(maxsize=None)
def _inputs(cid):
    return make(BY_ID[cid])


def inputs(case):
    """Shared: do not modify."""
    return _inputs(case.id)


def branch_grads(case, p, dtype):
    """gx = sum_i d<gt_i, branch_i(x)>/dx + add0 + add1, gw<i> = d<gt_i, branch_i(x)>/dw_i."""
    N, P, h, w = case.shape
    x = p['x'].to(dtype).clone().requires_grad_(True)
    ws = [p['w%d' % i].to(dtype).clone().requires_grad_(True) for i in range(len(case.cfg['scales']))]
    loss = sum((p['gt%d' % i].to(dtype) * branch_value(x, ws[i], sz, P)).sum() for i, sz in enumerate(sizes_of(case)))
    g = torch.autograd.grad(loss, [x] + ws)
    gx = g[0]
    for k in range(case.cfg['adds']):
        gx = gx + p['add%d' % k].to(dtype)
    out = {'gx': gx}
    out.update({'gw%d' % i: t for i, t in enumerate(g[1:])})
    return out


def reference(case, p=None, dtype=torch.float64):
    """Gradients of <gy, op(x)> by torch.autograd.grad in `dtype`, from the float32 operands cast up."""
    p = inputs(case) if p is None else p
    if case.op in LINEAR:
        xs = [p['x%d' % k].to(dtype).clone().requires_grad_(True) for k in range(len(in_shapes(case)))]
        g = torch.autograd.grad((p['gy'].to(dtype) * linear_op(case, *xs)).sum(), xs)
        return {'gx%d' % k: t.detach() for k, t in enumerate(g)}
    if case.op == 'pyr_merge':
        return {k: v.detach() for k, v in ec.ref_pyr_merge(dict(shape=case.shape), p, dtype).items()}
    return {k: v.detach() for k, v in branch_grads(case, p, dtype).items()}


def magnitude_inputs(case):
    """Absolute values of all operands (BatchNorm mean: -|mean|; PReLU slopes: 1 on both sides, see exact_cases._prelu)."""
    p = {k: (-v.abs() if k.endswith('mean') else torch.ones_like(v) if k.endswith('alpha') else v.abs()) for k, v in inputs(case).items()}
    if case.op == 'pyr_merge':
        p['magnitude'] = True
        p['mraw'] = ec.merge_conv(p, case.shape, torch.float64).float()
    return p


# leading axes that index planes (the rest is reduced for the per-plane bound)
LEAD = {'gx': 2, 'gx0': 2, 'gx1': 2, 'gt': 3, 'gw0': 1, 'gw1': 1, 'gw2': 1, 'g_merge_w': 2}


def plane_max(name, t):
    lead = LEAD.get(name, t.dim())
    return t.abs().flatten(lead).amax(-1) if t.dim() > lead else t.abs()


Ref = collections.namedtuple('Ref', 'r64 err32 mag bound')


@functools.lru_cache(maxsize=None)
def refs(cid):
    """Per output: the float64 reference, per plane the float32 CPU evaluation's gap to it and the magnitude evaluation, and the
    bound MARGIN * max(err32, 2^-23 * M).  Computed once."""
    case = BY_ID[cid]
    r64, r32, mag = reference(case), reference(case, dtype=torch.float32), reference(case, magnitude_inputs(case))
    out = {}
    for name, r in r64.items():
        assert r32[name].dtype == torch.float32
        err = plane_max(name, r32[name].double() - r)
        m = plane_max(name, mag[name])
        out[name] = Ref(r, err, m, MARGIN * torch.maximum(err, EPS * m))
    return out


# ------------------------------------------------------------------------------------------------------------------ probes
def axis_operator(case, k, axis):
    """The float64 operator of input k of a linear case along one axis, (O, I): the operation on a map that is one pixel
    wide in the other direction (avgpool: times 3, the other axis' share of the 1/9)."""
    I = in_shapes(case)[k][axis]
    eye = torch.eye(I, dtype=torch.float64)
    x = eye.view(1, I, I, 1) if axis == 0 else eye.view(1, I, 1, I)
    s = case.shape
    if case.op == 'avgpool':
        y = 3.0 * F.avg_pool2d(x, 3, 2, 1)
    elif case.op == 'adaptive':
        y = F.adaptive_avg_pool2d(x, (s[3], 1) if axis == 0 else (1, s[4]))
    else:
        O = out_shape(case)[axis]
        y = up(x, (O, 1) if axis == 0 else (1, O))
        if case.op == 'two_head' and k == 1:
            y = y * (0.5 if axis == 0 else 1.0)
    return y.reshape(I, -1).t().contiguous()


def receivers(A1):
    """Per output of a 1-D operator: [lo, hi] input range that holds its non-zero weights, widened by one on each side."""
    I = A1.shape[1]
    nz = A1 != 0
    idx = torch.arange(I)
    lo = torch.where(nz, idx, I).amin(1) - 1
    hi = torch.where(nz, idx, -1).amax(1) + 1
    return lo.clamp_(0, I - 1).tolist(), hi.clamp_(0, I - 1).tolist()


def colours(A1):
    """Greedy colouring of the outputs of a 1-D operator: outputs of one colour have disjoint (widened) receivers.
    -> list of colours, each a list of outputs."""
    lo, hi = receivers(A1)
    cols, ends = [], []                 # ends[c]: last input covered by colour c so far (outputs come in increasing order of lo)
    for o in sorted(range(A1.shape[0]), key=lambda o: (lo[o], hi[o])):
        for c in range(len(cols)):
            if ends[c] < lo[o]:
                cols[c].append(o)
                ends[c] = hi[o]
                break
        else:
            cols.append([o])
            ends.append(hi[o])
    return cols


Probe = collections.namedtuple('Probe', 'hot owner')


@functools.lru_cache(maxsize=None)
def bwd_probes(cid, k=0):
    """Backward probes of input k: hot (planes, K) int64 -- the flat indices of the one-hot elements of each gradient plane, padded
    with -1 --, owner (planes, Hi*Wi) int64 -- the hot output an input element may receive from; -1: none, the kernel must write
    exactly 0 there."""
    case = BY_ID[cid]
    Ho, Wo = out_shape(case)
    Hi, Wi = in_shapes(case)[k]
    Ay, Ax = axis_operator(case, k, 0), axis_operator(case, k, 1)
    if Ho * Wo <= FULL_BASIS:
        cy, cx = [[o] for o in range(Ho)], [[o] for o in range(Wo)]
    else:
        cy, cx = colours(Ay), colours(Ax)

    def axis_tables(A1, cols, I):
        lo, hi = receivers(A1)
        own = torch.full((len(cols), I), -1, dtype=torch.int64)
        hot = torch.full((len(cols), max(len(c) for c in cols)), -1, dtype=torch.int64)
        for c, outs in enumerate(cols):
            hot[c, :len(outs)] = torch.tensor(outs)
            for o in outs:
                own[c, lo[o]:hi[o] + 1] = o
        return own, hot
    (oy, hy), (ox, hx) = axis_tables(Ay, cy, Hi), axis_tables(Ax, cx, Wi)
    oy, ox = oy[:, None, :, None], ox[None, :, None, :]
    owner = torch.where((oy >= 0) & (ox >= 0), oy * Wo + ox, -1)
    hy, hx = hy[:, None, :, None], hx[None, :, None, :]
    hot = torch.where((hy >= 0) & (hx >= 0), hy * Wo + hx, -1)
    return Probe(hot.reshape(len(cy) * len(cx), -1), owner.reshape(len(cy) * len(cx), Hi * Wi))


def dense_operator(case, k=0):
    """The float64 operator of input k, (Ho*Wo, Hi*Wi), from the operation itself on the full basis."""
    Hi, Wi = in_shapes(case)[k]
    eye = torch.eye(Hi * Wi, dtype=torch.float64).view(1, Hi * Wi, Hi, Wi)
    xs = [torch.zeros(1, Hi * Wi, *hw, dtype=torch.float64) for hw in in_shapes(case)]
    xs[k] = eye
    return linear_op(case, *xs).reshape(Hi * Wi, -1).t().contiguous()
