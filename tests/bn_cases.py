"""Inputs, the float64 oracle and the bounds of the batch-statistics BatchNorm kernels at ill-conditioned channels and at the seams
between their forms (a helper, no tests).

The three forms (mspl_amd/csrc/supervised.hip, affine_bwd.hip): the small-plane node (one workgroup per channel), the fused two-launch
node (`parts` ranges per channel, persistent workspace) and the plain statistics pair behind autograd.bn_batch_stats.  The reference
is `bn_train_prelu_oracle` on `.double()` inputs; the yardstick of every bound is the SAME oracle on the float32 inputs on the CPU
against its float64 result (`err32`) and the rounding of float32 (FLOOR) times a magnitude taken from float64 -- never the code under
test.  tests/test_bn_cases.py holds the oracle, the generator and the bounds themselves to the conditions the GPU tests rely on."""
import collections
import functools

import numpy as np
import torch

MARGIN = 4                                  # |kernel - float64| <= MARGIN * max(err32, FLOOR * magnitude), as tests/confident_cases.py
FLOOR = 2.0 ** -23
BAND_FACTOR = 64                            # no pre-activation lies within BAND_FACTOR element bounds of 0 (the PReLU branch is safe)
EPS, MOMENTUM = 1e-5, 0.1                   # nn.BatchNorm2d's defaults

# ------------------------------------------------------------------ the launch rules, restated on the host
SMALL_LIMIT = 40960                         # mspl_bn_train_small_fits: N * HW <= 40960
SMALL_WIDE = 2048                           # the small form takes 1024 threads from this many units on, 256 below
FWD_BLOCKS, BWD_BLOCKS = 768, 384           # workgroups the two-launch forward / backward aim at (parts = ceil(blocks / C))


def units(N, HW):
    """(units per plane L, units per channel): a unit is a quad when HW % 4 == 0 and a float otherwise."""
    L = HW // 4 if HW % 4 == 0 else HW
    return L, N * L


def small_fits(N, HW):
    return N * HW <= SMALL_LIMIT


def small_threads(N, HW):
    return 1024 if units(N, HW)[1] >= SMALL_WIDE else 256


def fused_parts(N, C, HW, blocks=FWD_BLOCKS):
    """parts = min(ceil(blocks / C), units / 512), at least 1."""
    return max(1, min(-(-blocks // C), units(N, HW)[1] // 512))


def fused_ranges(N, C, HW, blocks=FWD_BLOCKS):
    """[(u0, u1)] per workgroup of a channel: per = ceil(units / parts), u0 = r * per, u1 = min(units, u0 + per)."""
    total, parts = units(N, HW)[1], fused_parts(N, C, HW, blocks)
    per = -(-total // parts)
    return [(r * per, min(total, r * per + per)) for r in range(parts)]


def pair_chunks(N, C, HW):
    """Slices per plane of the plain pair's bn_stats_kernel and whether it takes its 16-byte path."""
    per = max(4096, -(-HW // max(1, -(-2048 // (N * C)))))
    per = (per + 3) & ~3
    return -(-HW // per), HW % 4 == 0


# ------------------------------------------------------------------ shapes, one per seam
Shape = collections.namedtuple('Shape', 'name dims form small classes unique')
CLASSES = ('benign', 'offset8', 'offset64', 'tiny', 'huge', 'near_const', 'const', 'outlier_k')
_DIST = {'benign': (0.5, 1.3), 'offset8': (8.0, 1.0), 'offset64': (64.0, 1.0), 'tiny': (1.0, 1e-2), 'huge': (0.0, 1e2),
         'near_const': (0.5, 1e-4), 'const': (3.0, 0.0), 'outlier_k': (0.0, 1.0)}
OUTLIER = 40.0                              # z[0, c, 0] of an outlier_k channel: the shift k of the forward sums, 40 sigma out
# The range of |mean_c| * invstd_c a channel class stands for (near_const and const are governed by eps: invstd = 1 / sqrt(var + eps));
# tests/test_bn_cases.py holds every shape with at least R_MIN_M values per channel to it.  There, too: |z[0,c,0] - mean| * invstd is
# below 6 on every class but outlier_k, where it lies in OUTLIER_RANGE (the outlier itself widens the variance: 1 + 1600 / M).
MEAN_RANGE = {'benign': (0.3, 0.5), 'offset8': (7.0, 9.0), 'offset64': (56.0, 72.0), 'tiny': (85.0, 115.0), 'huge': (0.0, 0.1),
              'near_const': (150.0, 160.0), 'const': (948.0, 949.5), 'outlier_k': (0.0, 0.1)}
OUTLIER_RANGE = (20.0, 41.0)
R_MIN_M = 2047


def _s(name, dims, form, small, classes=None, unique=None):
    """classes: of the channels the generator draws (all of them, or `unique` distinct ones that channel_index spreads over C)."""
    C = unique or dims[1]
    return Shape(name, dims, form, small, tuple(classes) if classes else tuple(CLASSES[c % len(CLASSES)] for c in range(C)), unique)


SHAPES = [
    # ---- the small form: N * HW <= 40960, one workgroup per channel
    _s('s_2047_scalar', (23, 8, 1, 89), 'small', True),      # HW = 89 (scalar units), L = 89, N * L = 2047: the last 256-thread shape
    # HW = 2 (scalar), N * L = 2048: the first 1024-thread shape.  Three channels: the three classes with the largest R that vary
    _s('s_2048_scalar', (1024, 3, 1, 2), 'small', True, ('offset64', 'outlier_k', 'near_const')),
    _s('s_2047_quads', (23, 8, 4, 89), 'small', True),       # HW = 356 = 4 * 89: quads, N * L = 2047, 256 threads
    _s('s_2048_quads', (8, 8, 32, 32), 'small', True),       # HW = 1024, L = 256, N * L = 2048: quads, 1024 threads
    _s('s_largest', (16, 8, 40, 64), 'small', True),         # N * HW = 40960: the largest small shape (10 quads per thread)
    _s('s_L1_scalar', (2, 8, 1, 1), 'small', True),          # HW = 1: L = 1 (step_n = NT, step_q = 0), M = 2 (the backward's double form)
    _s('s_L1_quads', (3, 8, 2, 2), 'small', True),           # HW = 4: one quad per plane, L = 1
    _s('s_L300', (1, 8, 30, 40), 'small', True),             # L = 300 > 256 threads: step_n = 0, step_q = 256 in advance()
    _s('s_L1026', (2, 8, 54, 76), 'small', True),            # L = 1026 > 1024 threads (N * L = 2052 >= 2048): step_n = 0 again
    _s('s_odd', (5, 8, 7, 9), 'small', True),                # HW = 63: an odd plane, N * L = 315
    # ---- the two-launch form: N * HW > 40960
    _s('t_first', (1, 8, 1, 40961), 'two', False),           # N * HW = 40961, the first shape past the rule; scalar, L > 256, 80 ranges
    _s('t_midplane', (2, 8, 144, 144), 'two', False),        # quads: 10368 units in 20 ranges of 519, the plane seam (5184) inside one
    # C = 1, scalar: 307280 units -> parts = min(768, 600) = 600, per = 513, 599 * 513 = 307287 >= 307280: the last range is empty.
    # (An empty range needs parts > per >= 512: the backward, which aims at 384 workgroups, cannot have one.)
    _s('t_empty_range', (16, 1, 115, 167), 'two', False, ('offset64',)),
    # C = 768: parts = ceil(768 / C) = 1; N * HW = 40964 > 40960 with one quad per plane (L = 1 in the range walk too).  parts = 1
    # needs C >= 768 and N * HW > 40960, 31.5 M elements at the least: the generator draws 24 distinct channels (each class three
    # times) and the device tensor repeats them in the irregular order of channel_index, so that the CPU side stays below 1 M elements
    _s('t_parts1', (10241, 768, 2, 2), 'two', False, unique=24),
    # ---- the plain pair (autograd.bn_batch_stats + affine_prelu), whatever the size
    _s('p_scalar3', (2, 8, 67, 131), 'pair', True),          # HW = 8777, HW % 4 = 1: three 4096-element slices on the scalar path
    _s('p_quads2', (1, 8, 64, 120), 'pair', True),           # HW = 7680: two slices (4096 + 3584) on the 16-byte path
    _s('p_one', (1, 8, 48, 80), 'pair', True),               # HW = 3840 <= 4096: one slice
]
# one value per channel (M = 1): nn.BatchNorm2d refuses it, the oracle defines it; tested apart (its float64 gz is exactly 0)
SHAPE_M1 = _s('s_M1', (1, 8, 1, 1), 'small', True)
SHAPE = dict((s.name, s) for s in SHAPES + [SHAPE_M1])
VARIANTS = [(True, True), (True, False), (False, True), (False, False)]      # (with residual, with alpha)
Case = collections.namedtuple('Case', 'shape with_res with_alpha fill')       # fill: 'classes', or 'zeros' (every element 0.0)
CASES = [Case(s.name, r, a, 'classes') for s in SHAPES for r, a in VARIANTS]


def generated_dims(shape):
    N, C, H, W = shape.dims
    return (N, shape.unique or C, H, W)


def channel_index(shape):
    """None, or for a shape with `unique` distinct channels the (C,) map channel -> distinct channel: channel c keeps the class
    c % 8 of the cycle and takes one of that class's unique / 8 draws at random (a fixed seed), so that no two distances between
    channels repeat the same data regularly."""
    if shape.unique is None:
        return None
    C, n = shape.dims[1], len(CLASSES)
    pick = torch.randint(0, shape.unique // n, (C,), generator=torch.Generator().manual_seed(4242))
    return pick * n + torch.arange(C) % n


def expand(t, index, dim=1):
    """A tensor of the distinct channels as the kernel sees it (all C channels), on t's device."""
    return t if (index is None or t is None) else t.index_select(dim if t.dim() > 1 else 0, index.to(t.device))


def case_id(case):
    return '%s-%s-%s%s' % (case.shape, 'res' if case.with_res else 'nores', 'alpha' if case.with_alpha else 'noalpha',
                           '' if case.fill == 'classes' else '-' + case.fill)


# ------------------------------------------------------------------ the oracle
def _bc(v):
    return v[None, :, None, None]


def bn_train_prelu_oracle(z, residual, gamma, beta, alpha, eps, momentum, running_mean, running_var):
    """PReLU(BatchNorm_train(z) + residual) in plain torch ops, in the dtype of its inputs: mean and biased variance over (N,H,W),
    the fold scale = gamma * invstd, shift = beta - mean * scale, u = z * scale + shift + residual, y = prelu(u, alpha); the running
    statistics move by the unbiased variance (the biased one when a channel has ONE value, M = 1: the kernels' documented choice --
    nn.BatchNorm2d refuses that shape).  residual / alpha may be None.  Differentiable through every op."""
    M = z.numel() // z.shape[1]
    mean = z.mean((0, 2, 3))
    d = z - _bc(mean)
    var = (d * d).mean((0, 2, 3))
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma * invstd
    shift = beta - mean * scale
    u = z * _bc(scale) + _bc(shift)
    if residual is not None:
        u = u + residual
    y = u if alpha is None else torch.where(u > 0, u, _bc(alpha) * u)
    with torch.no_grad():
        unbiased = var * (M / (M - 1.0)) if M > 1 else var
        new_mean = (1.0 - momentum) * running_mean + momentum * mean
        new_var = (1.0 - momentum) * running_var + momentum * unbiased
    return {'y': y, 'u': u, 'mean': mean, 'invstd': invstd, 'scale': scale, 'shift': shift, 'running_mean': new_mean,
            'running_var': new_var}


ELEMENTS = ('y', 'gz', 'gres')
REDUCTIONS = ('mean', 'invstd', 'scale', 'shift', 'running_mean', 'running_var', 'dgamma', 'dbeta', 'dalpha')


def evaluate(inp, dtype, eps=EPS, momentum=MOMENTUM, running_mean=None, running_var=None):
    """The oracle and its autograd gradients for the upstream gradient inp['gy'], everything in `dtype`; `gu` is the gradient at the
    pre-activation (after PReLU's backward).  running_mean / running_var: the buffers before the call (default 0 / 1)."""
    C = inp['z'].shape[1]
    leaf = lambda t: None if t is None else t.detach().to(dtype).clone().requires_grad_()      # noqa: E731
    z, res, ga, be, al = [leaf(inp[k]) for k in ('z', 'residual', 'gamma', 'beta', 'alpha')]
    rm = torch.zeros(C, dtype=dtype) if running_mean is None else running_mean.to(dtype)
    rv = torch.ones(C, dtype=dtype) if running_var is None else running_var.to(dtype)
    out = bn_train_prelu_oracle(z, res, ga, be, al, eps, momentum, rm, rv)
    out['u'].retain_grad()
    out['y'].backward(inp['gy'].to(dtype))
    r = dict((k, v.detach()) for k, v in out.items())
    r.update(gz=z.grad, gu=out['u'].grad, gres=None if res is None else res.grad, dgamma=ga.grad, dbeta=be.grad,
             dalpha=None if al is None else al.grad)
    return r


# ------------------------------------------------------------------ the bounds
def _chan(t, f):
    """Per-channel reduction f over (N, H*W) of an (N,C,H,W) tensor."""
    N, C = t.shape[:2]
    return f(t.reshape(N, C, -1).transpose(0, 1).reshape(C, -1), 1)


def _amax(t, dim):
    return t.abs().amax(dim)


def conditioning(z, r64):
    """R_c = max(|mean_c|, |z[0,c,0] - mean_c|) * invstd_c from float64: what one float32 rounding of the fold z * scale + shift, or of
    the uncentred t = sum g z - mean sum g, costs relative to the result."""
    k = z.double().reshape(z.shape[0], z.shape[1], -1)[0, :, 0]
    return torch.maximum(r64['mean'].abs(), (k - r64['mean']).abs()) * r64['invstd']


def element_bound(q64, q32, R, margin):
    return margin * torch.maximum(_chan(q32.double() - q64, _amax), FLOOR * (1.0 + R) * _chan(q64, _amax))


def bounds(inp, r64, r32, eps=EPS, momentum=MOMENTUM, running_mean=None, running_var=None, margin=MARGIN):
    """{quantity: per-channel bound (C,) float64} from the float64 result r64 and the float32 oracle r32 alone.

    Element tensors (y, gz, gres):  margin * max(err32_c, FLOOR * (1 + R_c) * max|ref64_c|).
    Channel reductions:             margin * max(err32_c, FLOOR * S_c), S_c the float64 sum of the absolute values of what the kernel
    adds (the forward-error bound of a float32 sum with the number of terms left out), carried through the formulas behind the sums:
      mean            |k| + sum|z - k| / M                                  (the forward sums are shifted by k = z[0,c,0])
      var             V = sum (z - k)^2 / M + (sum|z - k| / M)^2
      invstd          invstd + invstd^3 V / 2,   scale: |gamma| times that
      shift           |beta| + |mean| S_scale + S_mean |scale|
      running_mean    (1 - m) |before| + m S_mean;  running_var: (1 - m) |before| + m V M / (M - 1)
      d beta          sum|g'|                                               (g' the gradient after PReLU's backward)
      d gamma         invstd (sum|g' z| + |mean| sum|g'|)                   (t = sum g' z - mean sum g', uncentred, times invstd)
      d alpha         sum over u <= 0 of |g| (|u| + |z scale| + |mean scale|)   (a summand g u carries the rounding of u's fold)"""
    z = inp['z'].double()
    C = z.shape[1]
    M = z.numel() // C
    mean, invstd, scale = r64['mean'], r64['invstd'], r64['scale']
    k = z.reshape(z.shape[0], C, -1)[0, :, 0]
    dk = z - _bc(k)
    a1 = _chan(dk.abs(), torch.sum) / M
    a2 = _chan(dk * dk, torch.sum) / M
    s_mean, s_var = k.abs() + a1, a2 + a1 * a1
    s_invstd = invstd + 0.5 * invstd ** 3 * s_var
    s_scale = inp['gamma'].double().abs() * s_invstd
    rm = torch.zeros(C, dtype=torch.float64) if running_mean is None else running_mean.double()
    rv = torch.ones(C, dtype=torch.float64) if running_var is None else running_var.double()
    gu = r64['gu']
    unit = {'mean': s_mean, 'invstd': s_invstd, 'scale': s_scale,
            'shift': inp['beta'].double().abs() + mean.abs() * s_scale + s_mean * scale.abs(),
            'running_mean': (1.0 - momentum) * rm.abs() + momentum * s_mean,
            'running_var': (1.0 - momentum) * rv.abs() + momentum * s_var * (M / (M - 1.0) if M > 1 else 1.0),
            'dbeta': _chan(gu.abs(), torch.sum),
            'dgamma': invstd * (_chan((gu * z).abs(), torch.sum) + mean.abs() * _chan(gu.abs(), torch.sum))}
    if inp['alpha'] is not None:
        u = r64['u']
        neg = (u <= 0).double() * inp['gy'].double().abs()
        unit['dalpha'] = _chan(neg * (u.abs() + (z * _bc(scale)).abs() + _bc((mean * scale).abs())), torch.sum)
    R = conditioning(inp['z'], r64)
    out = {}
    for q in ELEMENTS:
        if r64[q] is None:
            continue
        out[q] = element_bound(r64[q], r32[q], R, margin)
    for q, s in unit.items():
        out[q] = margin * torch.maximum((r32[q].double() - r64[q]).abs(), FLOOR * s)
    return out


def ratios(got, ref64, bound, index=None):
    """Per-channel error / bound of one quantity (0 where the error is 0: an exact result under a zero bound), on got's device, in
    float64; index: channel_index of the shape (ref64 and bound hold the distinct channels)."""
    dev = got.device
    err = (got.detach().double() - expand(ref64.to(dev), index)).abs()
    if err.dim() == 4:
        err = _chan(err, lambda t, d: t.amax(d))
    return torch.where(err == 0, torch.zeros_like(err), err / expand(bound.to(dev), index)).cpu()


# ------------------------------------------------------------------ the generator
def _seed(shape, case, seed):
    N, C, H, W = shape.dims
    return 700001 + 7919 * seed + 13 * N + 101 * C + 31 * H + 37 * W + 3 * case.with_res + 5 * case.with_alpha + 11 * (case.fill == 'zeros')


def _prelu_band(inp, eps):
    """(u64, BAND_c): the float64 pre-activation and BAND_FACTOR element bounds on y per channel (forward only)."""
    r = {}
    for dtype in (torch.float64, torch.float32):
        a = [None if inp[k] is None else inp[k].to(dtype) for k in ('z', 'residual', 'gamma', 'beta', 'alpha')]
        C = a[0].shape[1]
        with torch.no_grad():
            r[dtype] = bn_train_prelu_oracle(*a, eps, 0.0, torch.zeros(C, dtype=dtype), torch.ones(C, dtype=dtype))
    r64, r32 = r[torch.float64], r[torch.float32]
    return r64['u'], BAND_FACTOR * element_bound(r64['y'], r32['y'], conditioning(inp['z'], r64), MARGIN)


def conditioned_input(case, seed, eps=EPS):
    """{z, residual, gy, gamma, beta, alpha, classes}: float32 CPU tensors (generated_dims(shape): the distinct channels) from a torch.Generator, every channel class side by side.

    Channel c of class (mean, std) holds mean + std * randn; offset8 / offset64 take the sign (-1)^(seed + c // 8) (offset8 the
    opposite one); const is 3.0 everywhere; outlier_k is randn with z[0,c,0] = 40.  fill = 'zeros': every element 0.0 (a bias-free
    convolution of a blank input).  gamma in [0.5, 1.5], |beta| in [0.25, 1] (a constant channel's output is PReLU(beta): it has a
    scale of its own), alpha in [0, 0.3], gy = randn, residual = randn * the channel's y scale sqrt(gamma^2 var invstd^2 + beta^2).

    PReLU branch safety (with alpha): every element whose float64 pre-activation u has |u| < BAND_c = 64 element bounds on y is drawn
    again -- the residual's element where there is a residual (the statistics stay), else z's (not on constant channels, where u = beta
    is out of the band by construction; never z[0,c,0]) -- until none is left.  Deterministic, on the CPU; no element is left out of
    any comparison afterwards."""
    shape = SHAPE[case.shape]
    N, C, H, W = generated_dims(shape)
    g = torch.Generator().manual_seed(_seed(shape, case, seed))
    mu = torch.tensor([_DIST[c][0] for c in shape.classes])
    sd = torch.tensor([_DIST[c][1] for c in shape.classes])
    for c, cls in enumerate(shape.classes):
        if cls in ('offset8', 'offset64'):
            mu[c] *= (1.0 if cls == 'offset64' else -1.0) * (-1.0) ** (seed + c // len(CLASSES))
    outl = [c for c, cls in enumerate(shape.classes) if cls == 'outlier_k']
    zeros = case.fill == 'zeros'

    def draw_z(n=None):
        if n is None:
            z = _bc(mu) + _bc(sd) * torch.randn(N, C, H, W, generator=g)
            z[0, outl, 0, 0] = OUTLIER
            return torch.zeros_like(z) if zeros else z
        return torch.randn(n, generator=g)

    z = draw_z()
    gamma = torch.rand(C, generator=g) + 0.5
    beta = (0.25 + 0.75 * torch.rand(C, generator=g)) * torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
    alpha = torch.rand(C, generator=g) * 0.3 if case.with_alpha else None
    gy = torch.randn(N, C, H, W, generator=g)
    residual = None
    if case.with_res:
        var = _chan(z.double(), lambda t, d: t.var(d, unbiased=False))
        yscale = torch.sqrt(gamma.double() ** 2 * var / (var + eps) + beta.double() ** 2).float()
        residual = _bc(yscale) * torch.randn(N, C, H, W, generator=g)
    inp = {'z': z, 'residual': residual, 'gy': gy, 'gamma': gamma, 'beta': beta, 'alpha': alpha, 'classes': shape.classes}
    if alpha is None:
        return inp
    fixed = torch.zeros(N, C, H, W, dtype=torch.bool)                  # z elements that are never drawn again
    fixed[0, outl, 0, 0] = True
    fixed[:, [c for c, cls in enumerate(shape.classes) if cls == 'const' or zeros]] = True
    for _ in range(64):
        u, band = _prelu_band(inp, eps)
        bad = u.abs() < _bc(band)
        if not bool(bad.any()):
            return inp
        ch = bad.nonzero()[:, 1]
        if residual is not None:
            residual[bad] = yscale[ch] * draw_z(int(bad.sum()))
        else:
            assert not bool((bad & fixed).any()), 'a fixed element of z lies in the PReLU band'
            z[bad] = mu[ch] + sd[ch] * draw_z(int(bad.sum()))
    raise AssertionError('PReLU band not cleared: %s' % (case,))


@functools.lru_cache(maxsize=2)
def reference(case, seed=0, eps=EPS, momentum=MOMENTUM):
    """(inputs, float64 result, float32 result, bounds) of one case on fresh running statistics (0 / 1); computed once per case,
    shared, never modified."""
    inp = conditioned_input(case, seed, eps)
    r64, r32 = evaluate(inp, torch.float64, eps, momentum), evaluate(inp, torch.float32, eps, momentum)
    return inp, r64, r32, bounds(inp, r64, r32, eps, momentum)


# ------------------------------------------------------------------ the defect the cases are there to see, restated in numpy float32
def _seq_mean_f32(v):
    """Row means of a float32 matrix, each row added up element after element in float32 (one accumulator, no pairwise tree)."""
    return (np.add.accumulate(v, axis=1, dtype=np.float32)[:, -1] / np.float32(v.shape[1])).astype(np.float32)


def _channel_rows(z):
    N, C = z.shape[:2]
    return np.ascontiguousarray(z.reshape(N, C, -1).transpose(1, 0, 2)).reshape(C, -1)


def y_unshifted_f32(inp, eps=EPS):
    """The forward with the variance taken as E[x^2] - E[x]^2 on the RAW values, float32 throughout (no shift by k): at
    |mean| >> std the two moments cancel."""
    zc = _channel_rows(inp['z'].numpy())
    e1, e2 = _seq_mean_f32(zc), _seq_mean_f32((zc * zc).astype(np.float32))
    var = np.maximum((e2 - (e1 * e1).astype(np.float32)).astype(np.float32), np.float32(0))
    return _fold_f32(inp, e1, var, eps)


def y_shifted_all_f32(inp, eps=EPS):
    """The kernels' shifted formula, E[(x-k)^2] - E[x-k]^2 with k = z[0,c,0], but float32 THROUGHOUT (the kernels keep float32 to a
    thread's few dozen terms and go to double across threads): with k an outlier the two SHIFTED moments cancel like the raw ones do
    at |mean| >> std.  (On a channel with mean 0 the raw moments do not cancel at all: dropping the shift is harmless there.)"""
    zc = _channel_rows(inp['z'].numpy())
    k = zc[:, :1]
    d = (zc - k).astype(np.float32)
    e1, e2 = _seq_mean_f32(d), _seq_mean_f32((d * d).astype(np.float32))
    var = np.maximum((e2 - (e1 * e1).astype(np.float32)).astype(np.float32), np.float32(0))
    return _fold_f32(inp, (k[:, 0] + e1).astype(np.float32), var, eps)


def _fold_f32(inp, mean, var, eps):
    z = inp['z'].numpy()
    invstd = (np.float32(1) / np.sqrt((var + np.float32(eps)).astype(np.float32))).astype(np.float32)
    scale = (inp['gamma'].numpy() * invstd).astype(np.float32)
    shift = (inp['beta'].numpy() - (mean * scale).astype(np.float32)).astype(np.float32)
    u = ((z * scale[None, :, None, None]).astype(np.float32) + shift[None, :, None, None]).astype(np.float32)
    if inp['residual'] is not None:
        u = (u + inp['residual'].numpy()).astype(np.float32)
    if inp['alpha'] is not None:
        u = np.where(u > 0, u, (inp['alpha'].numpy()[None, :, None, None] * u).astype(np.float32))
    return torch.from_numpy(u)
