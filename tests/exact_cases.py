"""Integer-data cases for the gradient kernels: operands are small integers or dyadic fractions, so every product and every partial
sum of a (piecewise) linear kernel is exactly representable in float32 and ANY summation order -- matrix cores, atomics, LDS trees,
split workspaces -- gives the same bits.  The kernel's result must therefore EQUAL a float64 reference; one term dropped, doubled or
misplaced at a chunk, band, strip or image seam changes an integer.

Shared by tests/test_exact_cases.py (CPU: the exactness precondition, float32 == float64 on the CPU, and the library's own plan
queries proving that a case reaches the kernel form and seam it is here for) and tests/test_gpu_exact_grad.py (the kernels).

Generators (seeded): activations, gradients and weights from {-2, -1, 1, 2} (no zeros: every term counts); BatchNorm scale and
inv from {0.5, 1, 2}; PReLU slopes from {0.25, 0.5}; frozen-BatchNorm mean from multiples of 0.25; shifts from ODD multiples of 0.25.
(Odd multiples of 0.5 would not do: with scale = 0.5 and an odd z, z * scale is itself an odd multiple of 0.5 and u = z * scale + shift
can be 0.  z * scale is always a multiple of 0.5, so an odd multiple of 0.25 keeps u != 0 and the PReLU branch is never in doubt.)

The fused EESP backward with the projection tail draws from subsets of these sets (make_eesp_fused says why).

Every reference is a plain torch statement of the forward operation whose gradients torch.autograd.grad takes; `reference(case, inputs,
dtype)` evaluates it in float64 (the reference) or float32 (the second summation order of the CPU test).

Exactness bound: the same expression on the absolute values of all operands (mean -> -|mean|, so that z - mean cannot cancel; PReLU
with slope 1 on both branches and d alpha summed over all elements), times
2^Q with 2^-Q the finest grid an intermediate of that output lies on (GRIDS below, derived per operation), must stay below 2^24 for
every output element.  It is a precondition on the DATA, asserted on the CPU; it is not a tolerance.
"""
import collections
import functools

import torch
import torch.nn.functional as F

from mspl_amd import _native as nv

VALS = (-2.0, -1.0, 1.0, 2.0)
SCALES = (0.5, 1.0, 2.0)
SLOPES = (0.25, 0.5)
SHIFTS = (-1.25, -0.75, -0.25, 0.25, 0.75, 1.25)
HALVES = (-2.5, -1.5, -0.5, 0.5, 1.5, 2.5)
MEANS = (-0.75, -0.5, -0.25, 0.0, 0.25, 0.5, 0.75)


def draw(shape, seed, vals=VALS):
    g = torch.Generator().manual_seed(seed)
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    return torch.tensor(vals, dtype=torch.float64)[torch.randint(len(vals), shape, generator=g)]


Case = collections.namedtuple('Case', 'op id cfg expect')


def _case(op, cid, expect=None, **cfg):
    return Case(op, '%s-%s' % (op, cid), cfg, expect or {})


def _grad(loss_terms, leaves):
    """d sum(<g, y>) / d leaves."""
    loss = sum((g * y).sum() for g, y in loss_terms)
    return torch.autograd.grad(loss, leaves, allow_unused=True)


def _leaf(t, dtype):
    return t.to(dtype).clone().requires_grad_(True)


def _bn(z, p, pre, dtype):
    """The affine / frozen-BatchNorm pre-activation of channel axis 1 and its differentiable leaves (scale | gamma, shift | beta).
    With mean / inv the folded pair the kernels get is scale = gamma * inv, shift = beta - mean * gamma * inv."""
    v = lambda t: t.to(dtype).view(1, -1, *([1] * (z.dim() - 2)))            # noqa: E731
    scale, shift = p[pre + 'scale'].to(dtype), p[pre + 'shift'].to(dtype)
    if pre + 'mean' in p:
        mean, inv = p[pre + 'mean'].to(dtype), p[pre + 'inv'].to(dtype)
        a, b = (scale / inv).requires_grad_(True), (shift + mean * scale).requires_grad_(True)
        return (z - v(mean)) * v(inv) * v(a) + v(b), a, b
    a, b = scale.clone().requires_grad_(True), shift.clone().requires_grad_(True)
    return z * v(a) + v(b), a, b


def _bn_params(p, pre, C, seed, mean_inv, coarse=False):
    """coarse: the subsets with integer scales (then odd multiples of 0.5 keep u != 0), for cases whose sums are long."""
    p[pre + 'scale'], p[pre + 'shift'] = draw(C, seed, SCALES[1:] if coarse else SCALES), draw(C, seed + 1, HALVES if coarse else SHIFTS)
    p[pre + 'alpha'] = draw(C, seed + 2, SLOPES[1:] if coarse else SLOPES)
    if mean_inv:
        p[pre + 'mean'], p[pre + 'inv'] = draw(C, seed + 3, MEANS[1::2] if coarse else MEANS), draw(C, seed + 4, SCALES[1:] if coarse else SCALES)


def _prelu(u, al, p):
    """PReLU; in the magnitude evaluation (operands >= 0, so u > 0 everywhere) the form that bounds both branches: slope 1 on every
    element and d / d alpha = the sum of g * u over ALL elements."""
    if 'magnitude' in p:
        return u * al.view(1, -1, *([1] * (u.dim() - 2)))
    return F.prelu(u, al)


def conv_out(h, k, s):
    return (h + 2 * (k // 2) - (k - 1) - 1) // s + 1


# ------------------------------------------------------------------------------------------------------------------ operations
# Each: make(cfg) -> inputs (float64), ref(cfg, inputs, dtype) -> outputs, and GRIDS[op]: output -> Q.

def make_conv_wgrad(cfg):
    N, Cin, Cout, G, H, W, K, s = cfg['shape']
    p = {'x': draw((N, Cin, H, W), 1), 'gy': draw((N, Cout, conv_out(H, K, s), conv_out(W, K, s)), 2)}
    if cfg.get('accumulate'):
        p['pre_gw'] = draw((Cout, Cin // G, K, K), 3)
    return p


def ref_conv_wgrad(cfg, p, dtype):
    N, Cin, Cout, G, H, W, K, s = cfg['shape']
    w = torch.zeros(Cout, Cin // G, K, K, dtype=dtype, requires_grad=True)
    gw, = _grad([(p['gy'].to(dtype), F.conv2d(p['x'].to(dtype), w, None, s, K // 2, 1, G))], [w])
    return {'gw': gw + p['pre_gw'].to(dtype) if 'pre_gw' in p else gw}


def make_conv_dgrad(cfg):
    N, Cin, Cout, G, H, W, K, s = cfg['shape']
    p = {'w': draw((Cout, Cin // G, K, K), 4), 'gy': draw((N, Cout, conv_out(H, K, s), conv_out(W, K, s)), 2)}
    if cfg.get('accumulate'):
        p['pre_gx'] = draw((N, Cin, H, W), 5)
    return p


def ref_conv_dgrad(cfg, p, dtype):
    N, Cin, Cout, G, H, W, K, s = cfg['shape']
    x = torch.zeros(N, Cin, H, W, dtype=dtype, requires_grad=True)
    gx, = _grad([(p['gy'].to(dtype), F.conv2d(x, p['w'].to(dtype), None, s, K // 2, 1, G))], [x])
    return {'gx': gx + p['pre_gx'].to(dtype) if 'pre_gx' in p else gx}


def _k2_branches(x, w4, dil, stride):
    n = x.shape[1]
    return [F.conv2d(x, w4[k].unsqueeze(1), None, stride, dil[k], dil[k], n) for k in range(4)]


def _hff(branches):
    """Hierarchical feature fusion: block k of the concatenation is the sum of branches 0..k."""
    outs = []
    for k, o in enumerate(branches):
        outs.append(o if k == 0 else o + outs[-1])
    return torch.cat(outs, 1)


def make_eesp_dw(cfg):
    N, n, H, W = cfg['shape']
    s = cfg['stride']
    p = {'gs': draw((4, N, n, (H - 1) // s + 1, (W - 1) // s + 1), 2), 'x': draw((N, n, H, W), 1), 'w4': draw((4, n, 3, 3), 4)}
    if cfg.get('prefill'):
        p['pre_gw'] = draw((4, n, 3, 3), 3)
    return p


def ref_eesp_dw(cfg, p, dtype):
    """gs[k] is the gradient that reaches branch k (already suffix-summed): the four branches are independent here."""
    x, w4 = _leaf(p['x'], dtype), _leaf(p['w4'], dtype)
    gs = p['gs'].to(dtype)
    gx, gw = _grad(list(zip(gs, _k2_branches(x, w4, cfg['dil'], cfg['stride']))), [x, w4])
    return {'gx': gx, 'gw': gw + p['pre_gw'].to(dtype) if 'pre_gw' in p else gw}


def make_eesp_fused(cfg):
    N, n, H, W = cfg['shape']
    # With the projection tail the data gradient of every pixel (36 taps of four suffix sums) is itself summed over the plane for
    # proj_1x1's parameter gradients: only the unit-magnitude, integer-scale subsets of the generators keep that within the bound
    tail = cfg['tail']
    vals = VALS[1:3] if tail else VALS
    p = {'z': draw((N, 4 * n, H, W), 6), 'gy': draw((N, 4 * n, H, W), 2, vals), 'w4': draw((4, n, 3, 3), 4, vals)}
    _bn_params(p, '', 4 * n, 10, cfg['mean_inv'], tail)
    if tail:
        p['c'] = draw((N, n, H, W), 1, vals)
        _bn_params(p, 'p', n, 20, cfg['mean_inv'], tail)
    else:
        p['x'] = draw((N, n, H, W), 1)
    if cfg.get('prefill'):
        p['pre_gw'] = draw((4, n, 3, 3), 3)
        for k, name in enumerate(('gscale', 'gshift', 'galpha')):
            p['pre_' + name] = draw(4 * n, 30 + k)
            if cfg['tail']:
                p['pre_gp' + name[1:]] = draw(n, 40 + k)
    return p


def fused_x(p, dtype=torch.float64):
    """K2's input as the kernel gets it: given, or PReLU(BN(c)) of the projection tail."""
    if 'c' not in p:
        return p['x'].to(dtype)
    with torch.no_grad():
        u, _, _ = _bn(p['c'].to(dtype), p, 'p', dtype)
        return F.prelu(u, p['palpha'].to(dtype))


def ref_eesp_fused(cfg, p, dtype):
    """[proj BN + PReLU ->] four dilated depthwise branches -> HFF -> br_after_cat's BN + PReLU, cotangent gy.  The kernel is handed
    the saved concatenation z as data, so the reference evaluates the BatchNorm at that z: z + (K2(x) - K2(x).detach()) has z's
    value exactly and K2's derivative."""
    tail = cfg['tail']
    w4 = _leaf(p['w4'], dtype)
    if tail:
        c, pal = _leaf(p['c'], dtype), _leaf(p['palpha'], dtype)
        pu, pa, pb = _bn(c, p, 'p', dtype)
        x, xin = _prelu(pu, pal, p), c
    else:
        x = xin = _leaf(p['x'], dtype)
    k2 = _hff(_k2_branches(x, w4, cfg['dil'], 1))
    z = p['z'].to(dtype) + (k2 - k2.detach())
    al = _leaf(p['alpha'], dtype)
    u, a, b = _bn(z, p, '', dtype)
    leaves = [xin, w4, a, b, al] + ([pa, pb, pal] if tail else [])
    g = dict(zip(['gx', 'gw', 'gscale', 'gshift', 'galpha', 'gpscale', 'gpshift', 'gpalpha'], _grad([(p['gy'].to(dtype), _prelu(u, al, p))], leaves)))
    for name in list(g):
        if 'pre_' + name in p:
            g[name] = g[name] + p['pre_' + name].to(dtype)
    return g


def make_hff_bn(cfg):
    N, n, HW = cfg['shape']
    p = {'z': draw((N, 4 * n, HW), 6), 'gy': draw((N, 4 * n, HW), 2)}
    _bn_params(p, '', 4 * n, 10, cfg['mean_inv'])
    return p


def _hff_leaves(z, dtype):
    """Branch tensors whose hierarchical fusion is z: o_0 = z_0, o_k = z_k - z_{k-1}."""
    zb = z.to(dtype).chunk(4, 1)
    return [(zb[k] if k == 0 else zb[k] - zb[k - 1]).clone().requires_grad_(True) for k in range(4)]


def ref_hff_bn(cfg, p, dtype):
    o = _hff_leaves(p['z'], dtype)
    al = _leaf(p['alpha'], dtype)
    u, a, b = _bn(_hff(o), p, '', dtype)
    g = _grad([(p['gy'].to(dtype), _prelu(u, al, p))], o + [a, b, al])
    return {'out': torch.stack(g[:4]), 'gscale': g[4], 'gshift': g[5], 'galpha': g[6]}


def make_hff_sum(cfg):
    N, n, HW = cfg['shape']
    return {'g': draw((N, 4 * n, HW), 2)}


def ref_hff_sum(cfg, p, dtype):
    o = _hff_leaves(torch.zeros_like(p['g']), dtype)
    return {'out': torch.stack(_grad([(p['g'].to(dtype), _hff(o))], o))}


def make_affine(cfg):
    N, C, HW = cfg['shape']
    p = {'c': draw((N, C, HW), 1), 'gy': draw((N, C, HW), 2)}
    if cfg.get('pre_add'):
        p['pre_add'] = draw((N, C, HW), 7)
    if cfg.get('residual'):
        p['residual'] = draw((N, C, HW), 8)
    _bn_params(p, '', C, 10, cfg['mean_inv'])
    return p


def ref_affine(cfg, p, dtype):
    """y = PReLU((c + pre_add) * scale + shift + residual); gz is the gradient of the pre-activation (= the residual's)."""
    c = _leaf(p['c'], dtype)
    r = _leaf(p['residual'] if 'residual' in p else torch.zeros_like(p['c']), dtype)
    al = _leaf(p['alpha'], dtype)
    u, a, b = _bn(c + p['pre_add'].to(dtype) if 'pre_add' in p else c, p, '', dtype)
    g = _grad([(p['gy'].to(dtype), _prelu(u + r, al, p))], [r, c, a, b, al])
    return dict(zip(['gz', 'gc', 'gscale', 'gshift', 'galpha'], g))


def make_down_tail(cfg):
    N, nin, C, HW = cfg['shape']
    p = {'a': draw((N, nin, HW), 1), 'b': draw((N, C - nin, HW), 7), 'gy': draw((N, C, HW), 2), 'alpha': draw(C, 12, SLOPES)}
    if cfg['reinf']:
        p['reinf'] = draw((N, C, HW), 8, HALVES)         # odd multiples of 0.5: cat[a, b] + reinf is never 0
    return p


def ref_down_tail(cfg, p, dtype):
    a, b, al = _leaf(p['a'], dtype), _leaf(p['b'], dtype), _leaf(p['alpha'], dtype)
    z, leaves = torch.cat([a, b], 1), [a, b, al]
    if 'reinf' in p:
        r = _leaf(p['reinf'], dtype)
        z, leaves = z + r, leaves + [r]
    return dict(zip(['ga', 'gb', 'galpha', 'greinf'], _grad([(p['gy'].to(dtype), _prelu(z, al, p))], leaves)))


def make_wgrad_batch(cfg):
    p = {}
    for i, (N, Cin, Cout, G, HW) in enumerate(cfg['problems']):
        p['x%d' % i], p['gy%d' % i] = draw((N, Cin, HW), 100 + i), draw((N, Cout, HW), 200 + i)
        p['pre_gw%d' % i] = draw((Cout, Cin // G), 300 + i)
        if i in cfg.get('rowscale', ()):
            p['rowscale%d' % i] = draw(Cout, 400 + i, SCALES)
    return p


def ref_wgrad_batch(cfg, p, dtype):
    """Problem i: the weight gradient of y = rowscale * conv1x1(x, w) for the cotangent gy, added to what gw[i] held."""
    out = {}
    for i, (N, Cin, Cout, G, HW) in enumerate(cfg['problems']):
        w = torch.zeros(Cout, Cin // G, 1, dtype=dtype, requires_grad=True)
        y = F.conv1d(p['x%d' % i].to(dtype), w, None, 1, 0, 1, G)
        if 'rowscale%d' % i in p:
            y = y * p['rowscale%d' % i].to(dtype).view(1, -1, 1)
        out['gw%d' % i] = _grad([(p['gy%d' % i].to(dtype), y)], [w])[0][:, :, 0] + p['pre_gw%d' % i].to(dtype)
    return out


def make_dense(cfg):
    N, Cin, Cout, H, W, k, dil = cfg['shape']
    return {'x': draw((N, Cin, H, W), 1), 'w': draw((Cout, Cin, k, k), 4), 'gy': draw((N, Cout, H, W), 2), 'pre_gx': draw((N, Cin, H, W), 5)}


def ref_dense(cfg, p, dtype):
    N, Cin, Cout, H, W, k, dil = cfg['shape']
    x, w = _leaf(p['x'], dtype), _leaf(p['w'], dtype)
    b = torch.zeros(Cout, dtype=dtype, requires_grad=True)
    gx, dw, db = _grad([(p['gy'].to(dtype), F.conv2d(x, w, b, 1, dil * (k // 2), dil))], [x, w, b])
    if Cout % 32:                      # mspl_dense_conv_dgrad takes whole 32-channel tiles of Cout only: the weight gradient alone
        return {'dw': dw, 'db': db}
    return {'gx': gx, 'gx_acc': gx + p['pre_gx'].to(dtype), 'dw': dw, 'db': db}


def make_sums(cfg):
    planes, HW, n = cfg['shape']
    p = {'src%d' % k: draw((planes, HW), 50 + k) for k in range(n)}
    p['pc'], p['v'], p['pre'] = draw(planes, 60), draw(planes, 61), draw((planes, HW), 62)
    return p


def ref_sums(cfg, p, dtype):
    """FanOutFn's backward (n consumers of one tensor, one of them a global average pool), the plane dot product and the broadcast."""
    planes, HW, n = cfg['shape']
    x = torch.zeros(planes, HW, dtype=dtype, requires_grad=True)
    srcs = [p['src%d' % k].to(dtype) for k in range(n)]
    total, = _grad([(s, x) for s in srcs], [x])
    with_pc, = _grad([(s, x) for s in srcs] + [(0.5 * p['pc'].to(dtype), x.sum(1))], [x])
    bc, = _grad([(0.5 * p['v'].to(dtype), x.sum(1))], [x])
    return {'sum_n': total, 'sum_n_planes': with_pc, 'plane_dot': (srcs[0] * srcs[1]).sum(1), 'plane_sum': srcs[0].sum(1),
            'broadcast': bc, 'broadcast_acc': bc + p['pre'].to(dtype)}


def make_pyr_merge(cfg):
    """zcat and gy are drawn; mraw is the reference's own convolution result (exact on these data).  Unit-magnitude data and the
    integer-scale subsets: merge_layer.2's parameter gradients are sums over whole planes of products of a nine-tap-per-branch sum."""
    N, P, h, w, nb = cfg['shape']
    v = VALS[1:3]
    p = {'zcat': draw((N, nb * P, h, w), 6, v), 'gy': draw((N, P, h, w), 2, v), 'merge_w': draw((P, nb, 3, 3), 4, v)}
    _bn_params(p, 'br_', nb * P, 10, cfg['mean_inv'], True)
    _bn_params(p, 'm_', P, 20, cfg['mean_inv'], True)
    if not cfg['m_alpha']:
        del p['m_alpha']
    p['mraw'] = merge_conv(p, cfg['shape'], torch.float64)
    return p


def _merge_forward(p, shape, dtype):
    """merge_layer.0 (BatchNorm + PReLU over the concatenation), Shuffle, merge_layer.2's grouped 3x3 -> (m, leaves)."""
    N, P, h, w, nb = shape
    z, wm, bal = _leaf(p['zcat'], dtype), _leaf(p['merge_w'], dtype), _leaf(p['br_alpha'], dtype)
    u, ba, bb = _bn(z, p, 'br_', dtype)
    y = _prelu(u, bal, p).view(N, nb, P, h, w).transpose(1, 2).reshape(N, P * nb, h, w)
    return F.conv2d(y, wm, None, 1, 1, 1, P), [z, ba, bb, bal, wm]


def merge_conv(p, shape, dtype):
    return _merge_forward(p, shape, dtype)[0].detach()


def ref_pyr_merge(cfg, p, dtype):
    """mspl_pyrpool_merge_bwd: out = [PReLU](BN(m)), m = conv3x3(Shuffle(PReLU(BN(zcat)))), cotangent gy.  The kernel is handed the kept
    convolution result as data: mraw + (m - m.detach()) has mraw's value exactly and the convolution's derivative.  gt is
    branch-major (nb, N, P, h, w)."""
    N, P, h, w, nb = cfg['shape']
    m, leaves = _merge_forward(p, cfg['shape'], dtype)
    u, ma, mb = _bn(p['mraw'].to(dtype) + (m - m.detach()), p, 'm_', dtype)
    leaves += [ma, mb]
    if 'm_alpha' in p:
        mal = _leaf(p['m_alpha'], dtype)
        u = _prelu(u, mal, p)
        leaves.append(mal)
    g = dict(zip(['gt', 'g_br_scale', 'g_br_shift', 'g_br_alpha', 'g_merge_w', 'g_m_scale', 'g_m_shift', 'g_m_alpha'],
                 _grad([(p['gy'].to(dtype), u)], leaves)))
    g['gt'] = g['gt'].view(N, nb, P, h, w).transpose(0, 1).contiguous()
    return g


OPS = {'conv_wgrad': (make_conv_wgrad, ref_conv_wgrad), 'conv_dgrad': (make_conv_dgrad, ref_conv_dgrad),
       'eesp_dw': (make_eesp_dw, ref_eesp_dw), 'eesp_fused': (make_eesp_fused, ref_eesp_fused), 'hff_bn': (make_hff_bn, ref_hff_bn),
       'hff_sum': (make_hff_sum, ref_hff_sum), 'affine': (make_affine, ref_affine), 'down_tail': (make_down_tail, ref_down_tail),
       'wgrad_batch': (make_wgrad_batch, ref_wgrad_batch), 'dense': (make_dense, ref_dense), 'sums': (make_sums, ref_sums),
       'pyr_merge': (make_pyr_merge, ref_pyr_merge)}

# Q per output: 2^-Q is the finest grid an intermediate of that output lies on, in the kernel's or the reference's order.  With g, z,
# c, x, w integers; scale, inv on 2^-1; alpha, mean, shift on 2^-2:
#   u = z * scale + shift: 2^-2.  gz = g * alpha: 2^-2.  gz * scale: 2^-3.  sum gz * z, sum gz, sum g * u: 2^-2.
#   d gamma = (sum gz * z - mean * sum gz) * inv: 2^-(2 + 2 + 1).
GRIDS = {
    'conv_wgrad': {'gw': 0}, 'conv_dgrad': {'gx': 0}, 'eesp_dw': {'gx': 0, 'gw': 0}, 'hff_sum': {'out': 0},
    'hff_bn': {'out': 3, 'gscale': 5, 'gshift': 2, 'galpha': 2},
    'affine': {'gz': 2, 'gc': 3, 'gscale': 5, 'gshift': 2, 'galpha': 2},
    # cat[a, b] + reinf on 2^-1, times g: 2^-1; g * alpha: 2^-2
    'down_tail': {'ga': 2, 'gb': 2, 'greinf': 2, 'galpha': 1},
    'wgrad_batch': {'gw': 1},                                  # rowscale on 2^-1
    'dense': {'gx': 0, 'gx_acc': 0, 'dw': 0, 'db': 0},
    'sums': {'sum_n': 0, 'sum_n_planes': 1, 'plane_dot': 0, 'plane_sum': 0, 'broadcast': 1, 'broadcast_acc': 1},
    # G_k = suffix sums of gz * scale: 2^-3; gx = sum w * G: 2^-3; gw = sum G * x: 2^-3
    'eesp_fused': {'gx': 3, 'gw': 3, 'gscale': 5, 'gshift': 2, 'galpha': 2},
    # with the projection tail (coarse sets: scale, inv integers; alpha, shift, mean on 2^-1): u, gz, G, acc = sum w * G on 2^-1;
    # x = PReLU(u_p): 2^-2, so gw = sum G * x: 2^-3; acc * alpha_p [* c | * scale_p]: 2^-2; d gamma = (. - mean * .) * inv: one bit more
    # than its sums (gscale: 2^-2, gpscale: 2^-3); acc * u_p: 2^-2
    # pyr_merge (coarse sets, unit data): u on 2^-1, y = PReLU(u) on 2^-2, m = sum w * y on 2^-2; g_m = gy [* alpha_m] * scale_m on 2^-1;
    # gyi = sum w * g_m: 2^-1, * alpha_b: 2^-2 (gt, sum gz, sum gz * z); sum y * g_m: 2^-3; sum gyi * u: 2^-2; d gamma: one bit more than
    # its sums; merge_layer.2: gz * m on 2^-3, sum gz on 2^-1, gy * (m * scale + shift) on 2^-2
    'pyr_merge': {'gt': 2, 'g_merge_w': 3, 'g_br_scale': 3, 'g_br_shift': 2, 'g_br_alpha': 2, 'g_m_scale': 3, 'g_m_shift': 1, 'g_m_alpha': 2},
    'eesp_fused_tail': {'gx': 2, 'gw': 3, 'gscale': 2, 'gshift': 1, 'galpha': 1, 'gpscale': 3, 'gpshift': 2, 'gpalpha': 2},
}


def grid_q(case, name):
    key = 'eesp_fused_tail' if case.op == 'eesp_fused' and case.cfg['tail'] else case.op
    return GRIDS[key][name if case.op == 'pyr_merge' else name.rstrip('0123456789')]


@functools.lru_cache(maxsize=None)
def _inputs(cid):
    case = BY_ID[cid]
    return OPS[case.op][0](case.cfg)


def inputs(case):
    """The case's operands (float64, CPU).  Shared: do not modify."""
    return _inputs(case.id)


def reference(case, p=None, dtype=torch.float64):
    return {k: v.detach() for k, v in OPS[case.op][1](case.cfg, inputs(case) if p is None else p, dtype).items() if v is not None}


@functools.lru_cache(maxsize=None)
def reference64(cid):
    """The float64 reference of a case, computed once."""
    return reference(BY_ID[cid])


def magnitude_inputs(case):
    """Absolute values of all operands (mean: -|mean|, so that z - mean adds; PReLU slopes: 1, see _prelu)."""
    p = {k: (-v.abs() if k.endswith('mean') else torch.ones_like(v) if k.endswith('alpha') and not k.startswith('pre_') else v.abs())
         for k, v in inputs(case).items()}
    p['magnitude'] = True
    return p


# ------------------------------------------------------------------------------------------------------------------ plan queries
import ctypes  # noqa: E402


def wgrad_plan(shape, aligned16=True):
    """(form, parts, ngroups) of mspl_conv_bwd_weight for (N, Cin, Cout, groups, H, W, K, stride), from the library."""
    f, parts, ng = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    nv.check(nv.lib.mspl_conv_bwd_weight_plan(*shape, 1, int(aligned16), ctypes.byref(f), ctypes.byref(parts), ctypes.byref(ng)))
    return f.value, parts.value, ng.value


def dw_chunks(shape, stride):
    return nv.lib.mspl_eesp_dw_bwd_weight_chunks(*shape, stride)


def fused_bands(shape, dil):
    rows = ctypes.c_int32()
    bands = nv.lib.mspl_eesp_bwd_fused_bands(*shape, (ctypes.c_int32 * 4)(*dil), ctypes.byref(rows))
    return bands, rows.value


# ------------------------------------------------------------------------------------------------------------------ the table
# conv shapes are (N, Cin, Cout, groups, H, W, K, stride); `expect` is what the plan query must confirm (tests/test_exact_cases.py)
STRIP_GROUPS = {1: (16, 16, 16), 2: (16, 16, 8), 3: (12, 12, 4), 4: (16, 8, 4), 5: (10, 4, 2), 8: (16, 8, 2)}    # cin_g -> (Cin, Cout, groups)

CONV_SHAPES = [
    # 1x1 with 16x16 LDS tiles: an odd plane in chunks; the 3-channel zero-padded tile
    ('lds_odd', (2, 24, 20, 4, 17, 31, 1, 1), dict(form=nv.WGRAD_1X1_LDS, parts_min=2)),
    ('lds_3ch', (2, 3, 12, 1, 20, 30, 1, 1), dict(form=nv.WGRAD_1X1_LDS, parts_min=2)),
    # 1x1 on the matrix cores: fewer waves per tile than 64-pixel groups, not dividing them (a wave's groups lie in several images);
    # more waves than groups (empty slots); partial M and K tiles with a partial last pixel group
    ('mfma_span', (3, 512, 512, 1, 18, 30, 1, 1), dict(form=nv.WGRAD_1X1_MFMA, slots='span')),
    ('mfma_empty', (3, 512, 512, 4, 18, 30, 1, 1), dict(form=nv.WGRAD_1X1_MFMA, slots='empty')),
    ('mfma_partial', (1, 40, 24, 1, 8, 12, 1, 1), dict(form=nv.WGRAD_1X1_MFMA, slots='empty')),
    ('stem_s2', (2, 3, 16, 1, 96, 96, 3, 2), dict(form=nv.WGRAD_STEM_S2_STRIP, parts_min=2, unaligned_form=nv.WGRAD_STEM_COB4)),
    ('stem_cob4', (2, 3, 16, 1, 50, 45, 3, 1), dict(form=nv.WGRAD_STEM_COB4, parts_min=2)),
    ('strip1_two_images', (2, 16, 16, 16, 64, 68, 3, 1), dict(form=nv.WGRAD_STRIP, parts_min=2, cin_g=1)),
    ('generic', (2, 12, 12, 2, 64, 68, 3, 1), dict(form=nv.WGRAD_GENERIC, parts_min=2)),
    # the shapes above have two images in two chunks: the chunk seam is the image seam.  Three images with an odd number of pixels (or
    # strips): ceil(total / chunks) rounds, a chunk ends inside an image and inside a row, the last chunk is shorter
    ('stem_s2_odd', (3, 3, 16, 1, 54, 104, 3, 2), dict(form=nv.WGRAD_STEM_S2_STRIP, parts_min=2, seam_inside_image=True,
                                                       unaligned_form=nv.WGRAD_STEM_COB4)),
    ('stem_cob4_odd', (3, 3, 16, 1, 37, 41, 3, 1), dict(form=nv.WGRAD_STEM_COB4, parts_min=2, seam_inside_image=True)),
    ('generic_odd', (3, 12, 12, 2, 43, 65, 3, 1), dict(form=nv.WGRAD_GENERIC, parts_min=2, seam_inside_image=True)),
] + [
    ('strip%d' % c, (3, ci, co, g, 43, 68, 3, 1), dict(form=nv.WGRAD_STRIP, parts_min=2, cin_g=c, seam_inside_image=True,
                                                       unaligned_form=nv.WGRAD_G3X3))
    for c, (ci, co, g) in sorted(STRIP_GROUPS.items())
] + [
    # three groups in two chunks: six (group, chunk) pairs, so two of the eight slots of an XCD round are padding
    ('strip3_pad', (3, 9, 6, 3, 43, 68, 3, 1), dict(form=nv.WGRAD_STRIP, parts_min=2, cin_g=3, padded_pairs=True, seam_inside_image=True)),
] + [
    ('g3x3_%d' % c, (3, ci, co, g, 43, 67, 3, 1), dict(form=nv.WGRAD_G3X3, parts_min=2, cin_g=c, seam_inside_image=True))
    for c, (ci, co, g) in sorted(STRIP_GROUPS.items())
] + [
    ('g3x3_%d_s2' % c, (3,) + STRIP_GROUPS[c] + (70, 98, 3, 2), dict(form=nv.WGRAD_G3X3, parts_min=2, cin_g=c, seam_inside_image=True))
    for c in (1, 4)
]

CASES = []
for _name, _shape, _expect in CONV_SHAPES:
    for _acc in (0, 1):
        CASES.append(_case('conv_wgrad', '%s-acc%d' % (_name, _acc), _expect, shape=_shape, accumulate=_acc))
        CASES.append(_case('conv_dgrad', '%s-acc%d' % (_name, _acc), shape=_shape, accumulate=_acc))
    if 'unaligned_form' in _expect:
        # x and gy one float into a larger buffer: the launcher's own `& 15` test must pick the fallback form
        CASES.append(_case('conv_wgrad', '%s-unaligned' % _name, dict(form=_expect['unaligned_form'], parts_min=2, aligned16=False),
                           shape=_shape, accumulate=1, misalign=True))

CASES += [
    _case('eesp_dw', 's1', dict(chunks_min=2), shape=(2, 8, 36, 60), stride=1, dil=[1, 2, 3, 4], prefill=True),
    _case('eesp_dw', 's1-d1123', dict(chunks_min=2), shape=(2, 8, 36, 60), stride=1, dil=[1, 1, 2, 3]),
    # stride 2: even plane (a 2 x 2 input quad per thread), the same with gx two floats short of 8-byte alignment (the launcher's
    # `& 7` test: per-pixel form), and an odd plane (per-pixel form)
    _case('eesp_dw', 's2-even', dict(chunks_min=2), shape=(2, 6, 66, 64), stride=2, dil=[1, 2, 3, 4]),
    _case('eesp_dw', 's2-even-d1123', dict(chunks_min=2), shape=(2, 6, 66, 64), stride=2, dil=[1, 1, 2, 3], prefill=True),
    _case('eesp_dw', 's2-even-unaligned', dict(chunks_min=2), shape=(2, 6, 66, 64), stride=2, dil=[1, 2, 3, 4], misalign_gx=True),
    _case('eesp_dw', 's2-odd', dict(chunks_min=2), shape=(2, 5, 65, 63), stride=2, dil=[1, 2, 3, 4], prefill=True),
]
for _shape, _dil, _bands in [((2, 4, 37, 60), [1, 2, 3, 4], dict(bands=2, band_rows=19, last_rows=18)),
                             ((1, 4, 18, 140), [1, 2, 3, 4], dict(bands=4, band_rows=5, last_rows=3)),
                             ((1, 8, 9, 15), [1, 1, 2, 3], dict(bands=1, band_rows=9, last_rows=9))]:
    for _tail in (False, True):
        for _mi in (False, True):
            CASES.append(_case('eesp_fused', '%dx%d-tail%d-mean%d' % (_shape[2], _shape[3], _tail, _mi), _bands, shape=_shape, dil=_dil,
                               tail=_tail, mean_inv=_mi, prefill=_tail != _mi))
CASES += [
    # (N, n, HW): HW % 4 == 0 in two chunks, HW % 4 != 0 in two chunks, one small
    _case('hff_bn', 'quads', shape=(2, 4, 2048), mean_inv=True), _case('hff_bn', 'odd', shape=(2, 3, 2051), mean_inv=False),
    _case('hff_bn', 'small', shape=(3, 5, 35), mean_inv=True),
    _case('hff_sum', 'quads', shape=(2, 4, 2048)), _case('hff_sum', 'odd', shape=(3, 5, 35)),
    # (N, C, HW): N * HW / 4 >= 1024 (two parts per channel; three images, so a part crosses an image), an odd plane, one small
    _case('affine', 'parts', shape=(3, 6, 1400), mean_inv=False, pre_add=True, residual=True),
    _case('affine', 'bn-parts', shape=(3, 6, 1400), mean_inv=True, residual=True),
    _case('affine', 'bn-odd', shape=(2, 5, 1027), mean_inv=True, pre_add=True),
    _case('affine', 'small', shape=(2, 3, 15), mean_inv=False),
    # (N, nin, C, HW): HW / 4 >= 1024 (two chunks), one small
    _case('down_tail', 'chunks', shape=(2, 3, 8, 4100), reinf=True), _case('down_tail', 'chunks-noreinf', shape=(1, 2, 5, 4100), reinf=False),
    _case('down_tail', 'small', shape=(2, 3, 7, 12), reinf=True),
]
_E = [(2, 16, 16, 1, 20), (1, 40, 24, 1, 96), (3, 64, 32, 2, 36), (2, 8, 8, 1, 4), (2, 48, 80, 1, 128), (6, 32, 32, 1, 540)]   # eligible
_SMALL_M, _ODD_HW = (2, 12, 12, 4, 24), (2, 16, 16, 1, 15)                                      # left to mspl_conv_bwd_weight
CASES += [
    # (N, Cin, Cout, groups, HW) x 18: a run of matrix-core problems ends at an ineligible one twice
    _case('wgrad_batch', 'mixed', problems=[_E[0], _E[1], _E[2], _SMALL_M, _E[3], _E[4], _E[5], _ODD_HW] + [_E[i % 6] for i in range(10)],
          rowscale=(1, 4, 9, 17)),
    # ... and a run of the launch's 16-problem capacity between two ineligible ones
    _case('wgrad_batch', 'full', problems=[_SMALL_M] + [_E[i % 5] for i in range(16)] + [_ODD_HW], rowscale=(2, 16)),
]
CASES += [_case('dense', 'x'.join(str(v) for v in s) + '-split%d' % sp, shape=s, split=sp)
          for s, sp in [((3, 64, 48, 7, 9, 3, 2), 0), ((1, 32, 130, 9, 8, 1, 1), 0), ((2, 96, 256, 5, 6, 3, 6), 0),       # dilation >= H
                        ((4, 32, 32, 40, 40, 3, 3), 1), ((4, 32, 32, 40, 40, 3, 3), 2), ((4, 32, 32, 40, 40, 3, 3), 5),
                        ((4, 32, 32, 40, 40, 3, 3), 0)]]
CASES += [_case('sums', 'quads', shape=(6, 1028, 3)), _case('sums', 'small', shape=(3, 8, 8))]      # (planes, HW, tensors)

# (N, P, h, w, nb): one tile; a one-row band and a one-column tile; three bands of three tiles; w % 4 != 0 (the scalar path); every nb
for _shape in [(1, 4, 16, 64, 5), (1, 4, 17, 65, 5), (2, 3, 33, 130, 3), (1, 2, 9, 67, 2), (1, 1, 5, 6, 1), (1, 2, 17, 65, 4)]:
    for _al in (1, 0):
        for _mi in (0, 1):
            CASES.append(_case('pyr_merge', '%dx%dx%dx%d-nb%d-alpha%d-mean%d' % (_shape + (_al, _mi)), shape=_shape, m_alpha=bool(_al),
                               mean_inv=bool(_mi)))

BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
