"""tests/bn_cases.py held to the conditions tests/test_gpu_bn_conditioning.py relies on (no GPU): the oracle is nn.BatchNorm2d +
PReLU, the generator reaches the channel classes and clears the PReLU band, each seam shape sits where its comment says, the float32
oracle meets the bounds on its own, and a float32 forward without the kernels' precautions misses them."""
import pytest
import torch
import torch.nn.functional as F

from tests import bn_cases as bc

CLASSES_CASES = [bc.Case(s.name, True, True, 'classes') for s in bc.SHAPES]
ids = bc.case_id


def _M(shape):
    N, C, H, W = shape.dims
    return N * H * W


@pytest.mark.parametrize('case', [c for c in CLASSES_CASES if _M(bc.SHAPE[c.shape]) > 1], ids=ids)
def test_oracle_equals_batchnorm2d(case):
    """Outputs, every gradient and the running statistics of the oracle against nn.BatchNorm2d(...).double().train() + F.prelu, twice
    on one module (the second call on the first call's statistics)."""
    C = bc.generated_dims(bc.SHAPE[case.shape])[1]
    bn = torch.nn.BatchNorm2d(C).double().train()
    rm, rv = None, None
    for call in range(2):
        inp = bc.conditioned_input(case, call)
        r = bc.evaluate(inp, torch.float64, running_mean=rm, running_var=rv)
        rm, rv = r['running_mean'], r['running_var']
        with torch.no_grad():
            bn.weight.copy_(inp['gamma'])
            bn.bias.copy_(inp['beta'])
        bn.weight.grad = bn.bias.grad = None
        z, res, al = [inp[k].double().requires_grad_() for k in ('z', 'residual', 'alpha')]
        y = F.prelu(bn(z) + res, al)
        y.backward(inp['gy'].double())
        for name, got, want in [('y', r['y'], y.detach()), ('gz', r['gz'], z.grad), ('gres', r['gres'], res.grad),
                                ('dgamma', r['dgamma'], bn.weight.grad), ('dbeta', r['dbeta'], bn.bias.grad),
                                ('dalpha', r['dalpha'], al.grad), ('running_mean', rm, bn.running_mean),
                                ('running_var', rv, bn.running_var)]:
            # two float64 evaluations of one formula: 1e-9 of the largest value (cancellation at R ~ 1e3 costs three of the sixteen digits)
            tol = 1e-9 * max(float(want.abs().max()), 1e-30)
            assert float((got - want).abs().max()) <= tol, (name, call)
    assert int(bn.num_batches_tracked) == 2


def test_oracle_single_value_channels():
    """M = 1, which nn.BatchNorm2d refuses: mean = z, var = 0, invstd = 1 / sqrt(eps), y = PReLU(beta + residual); the running
    variance moves by the BIASED variance (0), the kernels' documented choice."""
    g = torch.Generator().manual_seed(3)
    z, res, gy = [torch.randn(1, 8, 1, 1, generator=g, dtype=torch.float64) for _ in range(3)]
    inp = {'z': z, 'residual': res, 'gy': gy, 'gamma': torch.rand(8, generator=g, dtype=torch.float64) + 0.5,
           'beta': torch.randn(8, generator=g, dtype=torch.float64), 'alpha': torch.full((8,), 0.25, dtype=torch.float64)}
    r = bc.evaluate(inp, torch.float64)
    assert torch.equal(r['mean'], z.flatten()) and torch.equal(r['invstd'], torch.full((8,), bc.EPS, dtype=torch.float64) ** -0.5)
    # (z * scale + (beta - z * scale) is beta to the rounding of z * scale = 316 gamma z: 1e-13)
    assert float((r['y'] - F.prelu(inp['beta'].view(1, 8, 1, 1) + res, inp['alpha'])).abs().max()) <= 1e-12
    assert torch.equal(r['running_var'], torch.full((8,), 1.0 - bc.MOMENTUM, dtype=torch.float64))
    assert torch.equal(r['running_mean'], bc.MOMENTUM * z.flatten())
    assert all(bool(torch.isfinite(r[k]).all()) for k in ('gz', 'gres', 'dgamma', 'dbeta', 'dalpha'))


# ------------------------------------------------------------------ the seams
def test_seam_shapes_sit_where_they_say():
    s = dict((sh.name, sh.dims) for sh in bc.SHAPES)
    hw = lambda n: s[n][2] * s[n][3]                                                     # noqa: E731
    for sh in bc.SHAPES:
        N, C, H, W = sh.dims
        assert bc.small_fits(N, H * W) == sh.small and (sh.form == 'small') <= sh.small and (sh.form == 'two') <= (not sh.small)
        n, c, h, w = bc.generated_dims(sh)
        assert n * c * h * w <= 1.5e6                             # what the CPU side ever holds
        idx = bc.channel_index(sh)
        if idx is not None:                                       # every distinct channel is used, in its own class, in no regular order
            assert sorted(set(idx.tolist())) == list(range(sh.unique)) and torch.equal(idx % 8, torch.arange(C) % 8)
            assert len(set((idx[8:] - idx[:-8]).tolist())) > 1 and idx.shape == (C,)
    # 256 | 1024 threads at 2047 | 2048 units, scalar and quads
    assert bc.units(s['s_2047_scalar'][0], hw('s_2047_scalar')) == (89, 2047) and bc.small_threads(23, 89) == 256
    assert bc.units(s['s_2048_scalar'][0], hw('s_2048_scalar')) == (2, 2048) and bc.small_threads(1024, 2) == 1024
    assert bc.units(s['s_2047_quads'][0], hw('s_2047_quads')) == (89, 2047) and hw('s_2047_quads') % 4 == 0
    assert bc.units(s['s_2048_quads'][0], hw('s_2048_quads')) == (256, 2048) and bc.small_threads(8, 1024) == 1024
    # small | two-launch at 40960 | 40961
    assert s['s_largest'][0] * hw('s_largest') == 40960 and s['t_first'][0] * hw('t_first') == 40961
    # L = 1; L above the workgroup (step_n = NT // L = 0)
    assert bc.units(2, hw('s_L1_scalar'))[0] == 1 and hw('s_L1_scalar') == 1
    assert bc.units(3, hw('s_L1_quads'))[0] == 1 and hw('s_L1_quads') == 4
    L, tot = bc.units(s['s_L300'][0], hw('s_L300'))
    assert L == 300 > bc.small_threads(1, hw('s_L300')) == 256
    L, tot = bc.units(s['s_L1026'][0], hw('s_L1026'))
    assert L == 1026 > bc.small_threads(2, hw('s_L1026')) == 1024
    assert hw('s_odd') % 2 == 1
    # the two-launch ranges: scalar with L > 256; ranges that end inside a plane; an empty trailing range; parts = 1
    N, C = s['t_first'][:2]
    assert hw('t_first') % 4 and bc.fused_parts(N, C, hw('t_first')) == 80 and bc.fused_parts(N, C, hw('t_first'), bc.BWD_BLOCKS) == 48
    N, C = s['t_midplane'][:2]
    L, tot = bc.units(N, hw('t_midplane'))
    rng = bc.fused_ranges(N, C, hw('t_midplane'))
    assert hw('t_midplane') % 4 == 0 and len(rng) == 20 and any(u0 < L < u1 for u0, u1 in rng)
    assert sum(1 for u0, u1 in rng if u1 % L) >= len(rng) - 2
    for blocks in (bc.FWD_BLOCKS, bc.BWD_BLOCKS):
        for name in ('t_first', 't_midplane', 't_empty_range', 't_parts1'):
            r = bc.fused_ranges(s[name][0], s[name][1], hw(name), blocks)
            tot = bc.units(s[name][0], hw(name))[1]
            assert sum(max(0, u1 - u0) for u0, u1 in r) == tot and r[0][0] == 0 and max(u1 for _, u1 in r) == tot
    N, C = s['t_empty_range'][:2]
    rng = bc.fused_ranges(N, C, hw('t_empty_range'))
    assert C == 1 and hw('t_empty_range') % 4 and len(rng) == 600 and rng[-1][0] >= bc.units(N, hw('t_empty_range'))[1]
    assert rng[-2][0] < rng[-2][1]
    N, C = s['t_parts1'][:2]
    assert C >= 768 and bc.fused_parts(N, C, hw('t_parts1')) == 1 == bc.fused_parts(N, C, hw('t_parts1'), bc.BWD_BLOCKS)
    assert 40960 < N * hw('t_parts1') <= 40960 + hw('t_parts1') and bc.units(N, hw('t_parts1'))[0] == 1
    # the plain pair: three slices on the scalar path; two and one on the 16-byte path
    assert bc.pair_chunks(*s['p_scalar3'][:2], hw('p_scalar3')) == (3, False) and hw('p_scalar3') == 8777 and 8777 % 4 == 1
    assert bc.pair_chunks(*s['p_quads2'][:2], hw('p_quads2')) == (2, True) and bc.pair_chunks(*s['p_one'][:2], hw('p_one')) == (1, True)


# ------------------------------------------------------------------ the generator and the bounds
GEN_CASES = bc.CASES + \
            [bc.Case('s_odd', r, True, 'zeros') for r in (True, False)]


@pytest.mark.parametrize('case', GEN_CASES, ids=ids)
def test_generator_reaches_its_conditions(case):
    """Per-channel conditioning in the stated ranges; near_const has var < eps / 100, const var == 0; no pre-activation is left inside
    BAND_c; the float32 oracle alone stays inside every bound taken with MARGIN = 1."""
    shape = bc.SHAPE[case.shape]
    inp, r64, r32, bnd = bc.reference(case)
    z = inp['z'].double()
    C = z.shape[1]
    var = bc._chan(z, lambda t, d: t.var(d, unbiased=False))
    m = r64['mean'].abs() * r64['invstd']
    k = z.reshape(z.shape[0], C, -1)[0, :, 0]
    away = (k - r64['mean']).abs() * r64['invstd']
    assert torch.equal(bc.conditioning(inp['z'], r64), torch.maximum(m, away))
    for c, cls in enumerate(inp['classes']):
        if case.fill == 'zeros':
            assert float(var[c]) == 0.0 and float(r64['mean'][c]) == 0.0 and not bool(inp['z'].any())
            continue
        if cls == 'const':
            assert float(var[c]) == 0.0 and float(r64['mean'][c]) == 3.0
        if _M(shape) < bc.R_MIN_M:
            continue
        if cls == 'near_const':
            assert 0.0 < float(var[c]) < bc.EPS / 100
        lo, hi = bc.MEAN_RANGE[cls]
        assert lo <= float(m[c]) <= hi, (cls, float(m[c]))
        if cls == 'outlier_k':
            assert float(k[c]) == bc.OUTLIER and bc.OUTLIER_RANGE[0] <= float(away[c]) <= bc.OUTLIER_RANGE[1], float(away[c])
        else:
            assert float(away[c]) < 6.0, (cls, float(away[c]))
    assert 0.5 <= float(inp['gamma'].min()) and float(inp['gamma'].max()) <= 1.5
    if case.with_alpha:
        assert 0.0 <= float(inp['alpha'].min()) and float(inp['alpha'].max()) <= 0.3
        band = bc.BAND_FACTOR * bnd['y']
        assert bool((r64['u'].abs() >= band[None, :, None, None]).all())          # ... and so no element is left out anywhere
        # on either side of 0 (the branch the band protects is taken), except where the whole channel is one value without a residual
        if _M(shape) >= bc.R_MIN_M and case.fill == 'classes':
            assert bool((r64['u'] < 0).any()) and bool((r64['u'] > 0).any())
    worst = {}
    for q, b in bnd.items():
        assert bool(torch.isfinite(b).all()) and bool((b >= 0).all()), q
        worst[q] = float(bc.ratios(r32[q], r64[q], b / bc.MARGIN).max())
        assert worst[q] <= 1.0, (q, worst[q])
    print(ids(case), 'err32 / (bound at MARGIN = 1):', ' '.join('%s %.2g' % kv for kv in sorted(worst.items())))


NEGATIVE = [bc.Case(n, r, True, 'classes') for n in ('s_2048_quads', 's_largest', 't_first', 't_midplane', 'p_scalar3') for r in (True, False)]


@pytest.mark.parametrize('case', NEGATIVE, ids=ids)
def test_cases_see_a_forward_without_the_precautions(case):
    """A float32 forward that takes the variance as E[x^2] - E[x]^2 on the raw values misses the y bound on the offset64 channel; one
    that shifts by k = z[0,c,0] like the kernels but stays in float32 across the whole channel misses it on outlier_k.  (The raw
    formula does NOT miss it on outlier_k, and cannot: that channel's mean is 0, its raw moments do not cancel -- measured 0.002 to
    0.2 of the bound, against 15 to 560 on offset64 and 12 to 320 for the float32 shifted form on outlier_k.  The defect an outlying k exposes is cancellation between the SHIFTED moments.)"""
    inp, r64, r32, bnd = bc.reference(case)
    cls = inp['classes']
    raw = bc.ratios(bc.y_unshifted_f32(inp), r64['y'], bnd['y'])
    shifted = bc.ratios(bc.y_shifted_all_f32(inp), r64['y'], bnd['y'])
    print(ids(case), 'raw moments:', ['%s %.2g' % (n, v) for n, v in zip(cls, raw.tolist())])
    print(ids(case), 'shifted, float32 throughout:', ['%s %.2g' % (n, v) for n, v in zip(cls, shifted.tolist())])
    assert float(raw[cls.index('offset64')]) > 1.0
    assert float(shifted[cls.index('outlier_k')]) > 1.0
