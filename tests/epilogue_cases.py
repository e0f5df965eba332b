"""The epilogue contract of the forward entry points, as a table, with the float64 reference every check compares against.
Shared by tests/test_epilogue_cases.py (no GPU) and tests/test_gpu_epilogue_contract.py.  Nothing here touches the code under test.

The rule (csrc/common.hpp, epi_apply): an entry point that takes an mspl_epilogue_t either applies a term as
    v = (acc + pre_add) * scale + shift + reinf + residual;  v = PReLU(v, alpha);  v *= gate
does, with every per-channel constant indexed by the ABSOLUTE destination channel coff + c, or it refuses the term on the host with
MSPL_ERR_UNSUPPORTED before anything is launched.

Per op the table holds: the C entry point, the terms it accepts and the terms it refuses (read from its host code; 'slice' is a
destination with more channels than the op writes, 'raw_out' the second, bare output), and its cases: (shape args, the kernel form
the shape is meant to reach, the line of the condition that sends it there).  A form is chosen by the shape AND by the terms present:
several lean forms take only scale/shift/alpha (AFFINE), the DownSampler's pool form exactly AFFINE + reinforcement, so those term
sets are tested next to every single term and next to all terms together.

Data rules: inputs are seeded randn (minus 0.2, so that pooled and resized values are negative more often than not and PReLU shows),
weights scaled by fan-in, scale in [0.5, 1.5), alpha <= 0.3; problem() walks a fixed list of seeds until every term of the set moves
at least half of the float64 outputs by more than VISIBLE x the comparison tolerance -- decided by the reference alone.
"""
import collections
import functools
import math

import torch
import torch.nn.functional as F

ATOL, RTOL = 2e-5, 1e-4          # tests/test_gpu_kernels.py's own tolerance for these kernels against a CPU reference
BARE_BILINEAR_ATOL = 1e-5        # ... and for bilinear without an epilogue
VISIBLE = 100.0                  # a term must move the reference by more than VISIBLE x (ATOL + RTOL |ref|) ...
VISIBLE_SHARE = 0.5              # ... on at least this share of the outputs
SEED_TRIES = 24

TERMS = ('scale', 'shift', 'alpha', 'pre_add', 'residual', 'reinf', 'gate')          # reinf = reinf_r and reinf_w together
ALL = frozenset(TERMS)
AFFINE = frozenset(('scale', 'shift', 'alpha'))
DOWN = AFFINE | {'reinf'}                                                            # the DownSampler's pool call
EVERYTHING = ALL | {'slice', 'raw_out'}

# gap: only where a case needs more room than the standing tolerance -- max |float32 torch-CPU reference - float64 reference| over the
# case's term sets (recomputed and pinned by tests/test_epilogue_cases.py); the comparison then allows 4 x gap.  Both such shapes
# resize with align_corners=True by a ratio float32 cannot hold (39/15; 32/65 and 46/93 inside the pyramid): the source position,
# computed in float32 as ATen does, differs from the float64 one by ~1e-6 of a pixel at the far end of the map.
Case = collections.namedtuple('Case', 'args form where gap', defaults=(None,))

D1234, D1123 = (1, 2, 3, 4), (1, 1, 2, 3)

OPS = {
    # ---- entry points that apply every operand term (epi_apply / epi_apply4 in every form)
    'conv3x3': dict(
        entry='mspl_conv3x3_fwd', accepts=EVERYTHING, refuses=frozenset(),
        # (N, Cin, Cout, G, H, W, stride, shuffle)
        cases=[Case((1, 3, 3, 1, 9, 15, 1, 0), 'LDS-tiled, odd W (element stores)', 'conv3x3.hip:536'),
               Case((1, 3, 32, 1, 31, 45, 2, 0), 'LDS-tiled, stride-2 stem', 'conv3x3.hip:608'),
               Case((2, 16, 6, 2, 41, 124, 1, 0), 'LDS-tiled, lean staging', 'conv3x3.hip:537'),
               Case((2, 6, 6, 6, 37, 64, 1, 0), 'depthwise streaming', 'conv3x3.hip:347'),
               # 8 -> 3 channels per group: the streaming form declines it (conv3x3.hip:504-506), lean staging of the tiled kernel
               Case((2, 128, 48, 16, 24, 120, 1, 0), 'grouped 8->3 per group: LDS-tiled, lean staging', 'conv3x3.hip:506'),
               Case((1, 256, 64, 64, 12, 60, 1, 0), 'grouped streaming <4,1>', 'conv3x3.hip:504'),
               Case((1, 64, 256, 64, 9, 28, 1, 0), 'grouped streaming <1,4>', 'conv3x3.hip:505'),
               Case((1, 80, 16, 16, 16, 30, 1, 5), 'LDS-tiled with Shuffle', 'conv3x3.hip:536')]),
    'conv1x1': dict(
        entry='mspl_conv1x1_fwd', accepts=EVERYTHING, refuses=frozenset(),
        termsets=(),             # operand terms: tests/test_gpu_kernels.py::test_conv1x1_epilogues; here raw_out and the split-K fall-back
        # (N, Cin, Cout, G, H, W); the form is the library's own answer (ops.conv1x1_plan; CONV1X1_PLAN_FORMS below is checked against
        # it by tests/test_conv1x1_cases.py, and tests/conv1x1_cases.py holds the exact-data cases of every form's seams)
        cases=[Case((2, 32, 24, 4, 16, 30), 'small-K vector-unit form (K = 8 per group)', 'conv1x1.hip:pw_decide'),
               Case((2, 512, 128, 4, 18, 30), 'matrix cores, tile-pipelined (grouped: not split-K)', 'conv1x1.hip:pw_decide'),
               Case((2, 128, 20, 1, 7, 11), 'split-K', 'conv1x1_splitk.hip:conv1x1_splitk_plan'),
               Case((12, 32, 16, 1, 144, 240), 'streaming vector-unit form', 'conv1x1.hip:plan_thin')]),
    'bilinear': dict(
        entry='mspl_bilinear_fwd', accepts=ALL | {'slice'}, refuses=frozenset({'raw_out'}),
        # ((N, C, Hi, Wi), (Ho, Wo), align_corners)
        cases=[Case((s, o, a), f, w, g if a else None) for a in (True, False) for s, o, f, w, g in [
            ((2, 3, 40, 64), (16, 32), 'streaming, down-scaling', 'resample.hip:557', 1.2e-5),
            ((1, 5, 9, 16), (27, 16), 'streaming, rows repeat', 'resample.hip:557', None),
            ((1, 2, 8, 15), (24, 45), 'strip kernel, Wo % 4 != 0', 'resample.hip:557', None),
            ((1, 2, 3, 8), (6, 8), 'strip kernel, Ho < 8', 'resample.hip:557', None)]]),
    'avgpool3x3s2': dict(
        entry='mspl_avgpool3x3s2_fwd', accepts=ALL | {'slice'}, refuses=frozenset({'raw_out'}),
        # (N, C, H, W)
        cases=[Case((2, 5, 16, 30), 'strip kernel, element stores (Wo = 15)', 'resample.hip:49'),
               Case((1, 3, 15, 24), 'strip kernel, 16-byte stores (Wo = 12)', 'resample.hip:49'),
               Case((2, 6, 36, 60), 'strip kernel (the lean form is the plane-sum entry point\'s)', 'resample.hip:493'),
               Case((2, 4, 8, 24), 'strip kernel (the lean form is the plane-sum entry point\'s)', 'resample.hip:493')]),
    'avgpool3x3s2_psum': dict(
        entry='mspl_avgpool3x3s2_psum_fwd', accepts=ALL | {'slice'}, refuses=frozenset({'raw_out'}),
        termsets=('singles', AFFINE, DOWN, ALL),
        cases=[Case((2, 5, 16, 30), 'strip kernel, element stores (Wo = 15)', 'resample.hip:513'),
               Case((1, 3, 15, 24), 'strip kernel, 16-byte stores (Wo = 12)', 'resample.hip:513'),
               Case((2, 6, 36, 60), 'DownSampler lean form, rows end in a half strip (with exactly AFFINE + reinf)', 'resample.hip:512'),
               Case((2, 4, 8, 24), 'DownSampler lean form, whole strips (with exactly AFFINE + reinf)', 'resample.hip:512')]),
    'adaptive_avgpool': dict(
        entry='mspl_adaptive_avgpool_fwd', accepts=ALL | {'slice'}, refuses=frozenset({'raw_out'}),
        # ((N, C, Hi, Wi), (Ho, Wo))
        cases=[Case(((1, 2, 6, 9), (5, 5)), 'strip form, overlapping windows', 'resample.hip:588'),
               Case(((2, 4, 32, 60), (16, 30)), 'strip form, exact 2x2 windows', 'resample.hip:588'),
               Case(((1, 3, 32, 60), (5, 5)), 'wave per output (Hi*Wi >= 32*Ho*Wo)', 'resample.hip:588')]),
    'pointwise': dict(
        entry='mspl_pointwise_fwd', accepts=ALL | {'slice'}, refuses=frozenset({'raw_out'}),
        cases=[Case((1, 5, 7, 9), 'element path (hw % 4 != 0)', 'resample.hip:416'),
               Case((2, 6, 16, 32), '16-byte path', 'resample.hip:416')]),
    'pyrpool_fused': dict(
        entry='mspl_pyrpool_fused_fwd', accepts=ALL | {'slice'}, refuses=frozenset({'raw_out'}),
        termsets=('singles', AFFINE, ALL),
        # (N, P, h, w) of the projected map; branch sizes by EfficientPyrPool.branch_sizes
        cases=[Case((1, 4, 6, 9), 'separable LDS form with AFFINE, table form otherwise', 'pyrpool_sep.hip:457'),
               Case((2, 8, 14, 22), 'separable LDS form with AFFINE, table form otherwise', 'pyrpool_sep.hip:457'),
               Case((2, 16, 33, 47), 'streaming form with AFFINE, table form otherwise', 'pyrpool_stream.hip:635', 5.5e-6)]),
    'pyrpool_fused_train': dict(
        entry='mspl_pyrpool_fused_train_fwd', accepts=EVERYTHING, refuses=frozenset(),
        termsets=(AFFINE, ALL),
        cases=[Case((1, 4, 6, 9), 'table form (narrower than the streaming form takes)', 'pyrpool_stream.hip:495'),
               Case((2, 16, 33, 47), 'streaming form with AFFINE + raw_out, table form otherwise', 'pyrpool_stream.hip:639')]),
    # ---- entry points that implement scale / shift / alpha and refuse the rest
    'eesp_dw_hff': dict(
        entry='mspl_eesp_dw_hff_fwd', accepts=AFFINE | {'slice', 'raw_out'}, refuses=ALL - AFFINE,
        termsets=('singles', AFFINE),
        # (N, n, H, W, dilations, stride, streaming form forced)
        cases=[Case((2, 8, 16, 30, D1234, 1, None), 'LDS-tiled / direct form, stride 1', 'eesp_dw.hip:847'),
               Case((5, 2, 37, 120, D1123, 2, True), 'stride-2 streaming form (left when raw_out is asked for)', 'eesp_dw.hip:848')]),
    'eesp_proj_dw_hff': dict(
        entry='mspl_eesp_proj_dw_hff_fwd', accepts=AFFINE | {'slice'}, refuses=(ALL - AFFINE) | {'raw_out'},
        termsets=(AFFINE,), atol=2e-4, rtol=2e-4,           # test_eesp_proj_dw_hff's tolerance (projection on the matrix cores)
        # (N, Cin, n, G, H, W, dilations)
        cases=[Case((1, 256, 64, 4, 8, 12, D1234), 'fused projection + depthwise', 'eesp_dw.hip:1251')]),
    'eesp_dw_exp': dict(
        entry='mspl_eesp_dw_exp_fwd', accepts=AFFINE | {'residual'}, refuses=frozenset({'pre_add', 'reinf', 'gate', 'slice', 'raw_out'}),
        termsets=(AFFINE | {'residual'},),                  # all four are required
        # (N, n, H, W, dilations)
        cases=[Case((1, 64, 1, 60, D1234), 'fused depthwise + expansion, 60 columns', 'eesp_exp.hip:527')]),
    'eesp_dw_exp_next': dict(
        entry='mspl_eesp_dw_exp_next_fwd', accepts=AFFINE | {'residual'}, refuses=frozenset({'pre_add', 'reinf', 'gate', 'slice', 'raw_out'}),
        termsets=(AFFINE | {'residual'},),
        cases=[Case((1, 64, 1, 60, D1234), 'fused depthwise + expansion + next projection', 'eesp_exp.hip:527')]),
    'down_head': dict(
        entry='mspl_down_head_fwd', accepts=DOWN | {'slice'}, refuses=frozenset({'pre_add', 'residual', 'gate', 'raw_out'}),
        termsets=(DOWN,),                                   # scale, shift, alpha are required; the slice is always [0, nin) of nout
        # (N, nin, n, G, H, W)
        cases=[Case((2, 32, 24, 4, 6, 24), 'projection + pool in one launch', 'down_head.hip:206')]),
    'dense_conv': dict(
        entry='mspl_dense_conv_fwd', accepts=AFFINE | {'slice'}, refuses=(ALL - AFFINE) | {'raw_out'},
        termsets=(AFFINE,), atol=2e-4, rtol=1e-4,           # test_dense_conv_shapes' tolerance
        # (N, Cin, Cout, H, W, k, dilation)
        cases=[Case((1, 64, 40, 7, 9, 3, 2), 'matrix cores, 64-pixel tiles', 'dense_conv.hip:349')]),
    'dense_conv_split': dict(
        entry='mspl_dense_conv_split_fwd', accepts=AFFINE | {'slice'}, refuses=(ALL - AFFINE) | {'raw_out'},
        termsets=(),                                        # arithmetic and epilogue: tests/test_gpu_dense_conv_split.py
        # (index into tests/split_cases.SHAPES, planes)
        cases=[Case((0, 2), 'bf16x3', 'dense_conv_split.hip:220')]),
}

# Entry points whose accepted terms are checked against float64 term by term (the others: refusals, then one valid call)
CONTRACT_OPS = ('conv3x3', 'bilinear', 'avgpool3x3s2', 'avgpool3x3s2_psum', 'adaptive_avgpool', 'pointwise', 'pyrpool_fused',
                'pyrpool_fused_train', 'eesp_dw_hff')
REFUSING_OPS = tuple(op for op, d in OPS.items() if d['refuses'])
RAW_OPS = ('conv3x3', 'conv1x1', 'eesp_dw_hff', 'pyrpool_fused_train')
# (op, case index, the term set of the lean form): a neutral further operand moves the call off the form
FALLBACKS = [('conv1x1', 2, AFFINE), ('pyrpool_fused', 0, AFFINE), ('pyrpool_fused', 2, AFFINE),
             ('avgpool3x3s2_psum', 2, DOWN), ('avgpool3x3s2_psum', 3, DOWN)]
# what mspl_conv1x1_fwd_plan answers for the conv1x1 cases above, in their order (ops.CONV1X1_FORMS names)
CONV1X1_PLAN_FORMS = ('small_k', 'pipe', 'split_k', 'thin')
PYR_SCALES = (2.0, 1.5, 1.0, 0.5, 0.1)


def termsets(op):
    """The term sets a contract op is tested with: every accepted operand term alone, then the sets its forms are keyed on."""
    d = OPS[op]
    acc = [t for t in TERMS if t in d['accepts']]
    out = []
    for ts in d.get('termsets', ('singles', AFFINE, frozenset(acc))):
        if ts == 'singles':
            out += [frozenset((t,)) for t in acc]
        elif ts not in out:
            out.append(frozenset(ts))
    return out


def tolerance(op, ci=None, bare=False):
    """(atol, rtol) of a comparison against float64: the standing tolerance of the op, 4 x the recorded gap where a case has one."""
    d = OPS[op]
    atol = BARE_BILINEAR_ATOL if bare and op == 'bilinear' else d.get('atol', ATOL)
    if ci is not None and d['cases'][ci].gap is not None:
        atol = max(atol, 4.0 * d['cases'][ci].gap)
    return atol, d.get('rtol', RTOL)


def term_id(ts):
    return '+'.join(t for t in TERMS if t in ts) or 'bare'


# ------------------------------------------------------------------ inputs and the float64 operations
def _rn(g, *shape):
    return torch.randn(*shape, generator=g)


def pyr_sizes(h, w):
    """EfficientPyrPool.branch_sizes (efficient_pyramid_pool.py:41-44)."""
    return [(max(int(math.ceil(h * s)), 5), max(int(math.ceil(w * s)), 5)) for s in PYR_SCALES]


def _hff(x, w4, dil, stride, dtype):
    n = x.shape[1]
    outs = []
    for k in range(4):
        o = F.conv2d(x.to(dtype), w4[k].unsqueeze(1).to(dtype), None, stride, dil[k], dil[k], n)
        outs.append(o if k == 0 else o + outs[-1])
    return torch.cat(outs, 1)


def _affine_prelu(v, s, b, a):
    v = v * s.to(v.dtype).view(1, -1, 1, 1) + b.to(v.dtype).view(1, -1, 1, 1)
    return torch.where(v > 0, v, v * a.to(v.dtype).view(1, -1, 1, 1))


def _pyr_down_map(x, size, w, P):
    """The low-resolution map a scale < 1 branch hands to the fused kernel (computed by other launches: an INPUT here, float32)."""
    return F.conv2d(F.adaptive_avg_pool2d(x.double(), size), w.double(), None, 1, 1, 1, P).float()


def make_inputs(op, args, seed):
    """The op's own float32 inputs (everything but the epilogue operands)."""
    g = torch.Generator().manual_seed(seed)
    if op == 'conv3x3':
        N, Cin, Cout, G, H, W, stride, sg = args
        return {'x': _rn(g, N, Cin, H, W) - 0.2, 'w': _rn(g, Cout, Cin // G, 3, 3) * (9 * Cin // G) ** -0.5}
    if op == 'conv1x1':
        N, Cin, Cout, G, H, W = args
        return {'x': _rn(g, N, Cin, H, W) - 0.2, 'w': _rn(g, Cout, Cin // G, 1, 1) * (Cin // G) ** -0.5}
    if op in ('bilinear', 'adaptive_avgpool'):
        return {'x': _rn(g, *args[0]) - 0.2}
    if op in ('avgpool3x3s2', 'avgpool3x3s2_psum', 'pointwise'):
        return {'x': _rn(g, *args) - 0.2}
    if op in ('pyrpool_fused', 'pyrpool_fused_train'):
        N, P, h, w = args
        sizes = pyr_sizes(h, w)
        nb = len(sizes)
        inp = {'x': _rn(g, N, P, h, w) - 0.2, 'stage_w': [_rn(g, P, 1, 3, 3) / 3.0 for _ in sizes],
               'br_scale': torch.rand(nb * P, generator=g) + 0.5, 'br_shift': _rn(g, nb * P) * 0.1,
               'br_alpha': torch.rand(nb * P, generator=g) * 0.3, 'merge_w': _rn(g, P, nb, 3, 3) * (9 * nb) ** -0.5}
        inp['down_e'] = {i: _pyr_down_map(inp['x'], s, inp['stage_w'][i], P) for i, s in enumerate(sizes) if s[0] < h or s[1] < w}
        return inp
    if op == 'eesp_dw_hff':
        N, n, H, W, dil, stride, stream = args
        return {'x': _rn(g, N, n, H, W) - 0.2, 'w': _rn(g, 4, n, 3, 3) / 3.0}
    if op == 'eesp_proj_dw_hff':
        N, Cin, n, G, H, W, dil = args
        return {'x': _rn(g, N, Cin, H, W), 'wp': _rn(g, n, Cin // G, 1, 1) * (Cin // G) ** -0.5, 'ps': torch.rand(n, generator=g) + 0.5,
                'pb': _rn(g, n) * 0.1, 'pa': torch.rand(n, generator=g) * 0.3, 'w': _rn(g, 4, n, 3, 3) / 3.0}
    if op in ('eesp_dw_exp', 'eesp_dw_exp_next'):
        N, n, H, W, dil = args
        return {'r': _rn(g, N, n, H, W), 'w': _rn(g, 4, n, 3, 3) / 3.0, 'bs': torch.rand(4 * n, generator=g) + 0.5, 'bb': _rn(g, 4 * n) * 0.1,
                'ba': torch.rand(4 * n, generator=g) * 0.3, 'wexp': _rn(g, 4 * n, n, 1, 1) * n ** -0.5,
                'w1': _rn(g, n, n, 1, 1) * n ** -0.5, 'ns': torch.rand(n, generator=g) + 0.5, 'nb': _rn(g, n) * 0.1,
                'na': torch.rand(n, generator=g) * 0.3}
    if op == 'down_head':
        N, nin, n, G, H, W = args
        return {'x': _rn(g, N, nin, H, W) - 0.2, 'wp': _rn(g, n, nin // G) * (nin // G) ** -0.5, 'ps': torch.rand(n, generator=g) + 0.5,
                'pb': _rn(g, n) * 0.1, 'pa': torch.rand(n, generator=g) * 0.3}
    if op == 'dense_conv':
        N, Cin, Cout, H, W, k, d = args
        return {'x': _rn(g, N, Cin, H, W), 'w': _rn(g, Cout, Cin, k, k) * (Cin * k * k) ** -0.5}
    raise KeyError(op)


def op_ref(op, args, inp, dtype=torch.float64):
    """The operation before its epilogue, in `dtype`, from the float32 inputs cast up: (N, C, Ho, Wo).  A dict for the ops with
    further outputs: 'acc' is what the epilogue applies to."""
    c = lambda t: t.to(dtype)                                                   # noqa: E731
    if op == 'conv3x3':
        N, Cin, Cout, G, H, W, stride, sg = args
        x = c(inp['x'])
        if sg:                                                                   # Shuffle(groups=sg) in front of the convolution
            x = x.view(N, sg, Cin // sg, H, W).transpose(1, 2).reshape(N, Cin, H, W)
        return F.conv2d(x, c(inp['w']), None, stride, 1, 1, G)
    if op == 'conv1x1':
        return F.conv2d(c(inp['x']), c(inp['w']), None, 1, 0, 1, args[3])
    if op == 'bilinear':
        return F.interpolate(c(inp['x']), args[1], mode='bilinear', align_corners=args[2])
    if op in ('avgpool3x3s2', 'avgpool3x3s2_psum'):
        return F.avg_pool2d(c(inp['x']), 3, 2, 1)
    if op == 'adaptive_avgpool':
        return F.adaptive_avg_pool2d(c(inp['x']), args[1])
    if op == 'pointwise':
        return c(inp['x'])
    if op in ('pyrpool_fused', 'pyrpool_fused_train'):
        N, P, h, w = args
        x = c(inp['x'])
        outs = []
        for i, size in enumerate(pyr_sizes(h, w)):
            if size == (h, w):
                t = F.conv2d(x, c(inp['stage_w'][i]), None, 1, 1, 1, P)
            elif i in inp['down_e']:
                t = F.interpolate(c(inp['down_e'][i]), (h, w), mode='bilinear', align_corners=True)
            else:
                t = F.interpolate(x, size, mode='bilinear', align_corners=True)
                t = F.adaptive_avg_pool2d(F.conv2d(t, c(inp['stage_w'][i]), None, 1, 1, 1, P), (h, w))
            outs.append(t)
        zcat = torch.cat(outs, 1)
        nb = len(outs)
        a = _affine_prelu(zcat, inp['br_scale'], inp['br_shift'], inp['br_alpha'])
        a = a.view(N, nb, P, h, w).transpose(1, 2).reshape(N, nb * P, h, w)      # Shuffle(groups=nb)
        return {'acc': F.conv2d(a, c(inp['merge_w']), None, 1, 1, 1, P), 'zcat': zcat}
    if op == 'eesp_dw_hff':
        N, n, H, W, dil, stride, stream = args
        return _hff(inp['x'], inp['w'], dil, stride, dtype)
    if op == 'eesp_proj_dw_hff':
        N, Cin, n, G, H, W, dil = args
        o1 = _affine_prelu(F.conv2d(c(inp['x']), c(inp['wp']), None, 1, 0, 1, G), inp['ps'], inp['pb'], inp['pa'])
        return _hff(o1, inp['w'], dil, 1, dtype)
    if op in ('eesp_dw_exp', 'eesp_dw_exp_next'):
        N, n, H, W, dil = args
        cat = _affine_prelu(_hff(inp['r'], inp['w'], dil, 1, dtype), inp['bs'], inp['bb'], inp['ba'])
        return F.conv2d(cat, c(inp['wexp']), None, 1, 0, 1, 4)
    if op == 'down_head':
        N, nin, n, G, H, W = args
        r = F.conv2d(c(inp['x']), c(inp['wp']).view(n, nin // G, 1, 1), None, 1, 0, 1, G)
        return {'acc': F.avg_pool2d(c(inp['x']), 3, 2, 1), 'r': _affine_prelu(r, inp['ps'], inp['pb'], inp['pa']),
                'sums': c(inp['x']).sum((2, 3))}
    if op == 'dense_conv':
        N, Cin, Cout, H, W, k, d = args
        return F.conv2d(c(inp['x']), c(inp['w']), None, 1, d * (k // 2), d)
    raise KeyError(op)


def _acc(r):
    return r['acc'] if isinstance(r, dict) else r


# ------------------------------------------------------------------ the epilogue operands and THE reference epilogue
def make_operands(N, C, H, W, terms, seed):
    """Float32 operands of an un-sliced destination (N, C, H, W) for the terms asked for."""
    g = torch.Generator().manual_seed(seed + 77)
    full = {'scale': torch.rand(C, generator=g) + 0.5, 'shift': _rn(g, C) * 0.5 - 0.3, 'alpha': torch.rand(C, generator=g) * 0.3,
            'pre_add': _rn(g, N, C, H, W), 'residual': _rn(g, N, C, H, W), 'reinf_r': _rn(g, N, 3, H, W), 'reinf_w': _rn(g, C, 3) * 0.5,
            'gate': torch.sigmoid(_rn(g, N, C))}
    keep = set(terms) - {'reinf'}
    if 'reinf' in terms:
        keep |= {'reinf_r', 'reinf_w'}
    return {k: v for k, v in full.items() if k in keep}


def embed(t, C, ctot, coff, seed=5):
    """The same operands in the geometry of a destination with ctot channels, the op's at [coff, coff + C): every per-channel and
    per-element value sits at the same ABSOLUTE channel, the rest is filled with other random values (never read by a correct kernel
    for its outputs, but valid memory)."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, v in t.items():
        if k == 'reinf_r':
            out[k] = v
            continue
        dim = 0 if k in ('scale', 'shift', 'alpha', 'reinf_w') else 1
        shape = list(v.shape)
        shape[dim] = ctot
        big = torch.randn(*shape, generator=g)
        if k in ('scale', 'alpha', 'gate'):
            big = big.abs() * 0.3 + 0.1
        big.narrow(dim, coff, C).copy_(v)
        out[k] = big
    return out


def ref_epilogue(acc, t, coff=0):
    """epi_apply in the dtype of `acc`: (acc + pre_add) * scale + shift + reinf + residual, PReLU, gate; operands in the geometry of
    the destination, channel c of acc is absolute channel coff + c."""
    dt = acc.dtype
    C = acc.shape[1]
    s = slice(coff, coff + C)
    ch = lambda v: v[s].to(dt).view(1, -1, 1, 1)                                # noqa: E731
    v = acc
    if 'pre_add' in t:
        v = v + t['pre_add'][:, s].to(dt)
    if 'scale' in t:
        v = v * ch(t['scale'])
    if 'shift' in t:
        v = v + ch(t['shift'])
    if 'reinf_r' in t:
        v = v + torch.einsum('cj,njhw->nchw', t['reinf_w'][s].to(dt), t['reinf_r'].to(dt))
    if 'residual' in t:
        v = v + t['residual'][:, s].to(dt)
    if 'alpha' in t:
        v = torch.where(v > 0, v, ch(t['alpha']) * v)
    if 'gate' in t:
        v = v * t['gate'][:, s].to(dt)[:, :, None, None]
    return v


def drop(t, term):
    gone = ('reinf_r', 'reinf_w') if term == 'reinf' else (term,)
    return {k: v for k, v in t.items() if k not in gone}


def visible_share(acc, t, term, atol=ATOL, rtol=RTOL):
    """Share of the outputs that `term` moves by more than VISIBLE x the comparison tolerance (float64 reference with / without)."""
    with_, without = ref_epilogue(acc, t), ref_epilogue(acc, drop(t, term))
    return float(((with_ - without).abs() > VISIBLE * (atol + rtol * with_.abs())).double().mean())


Problem = collections.namedtuple('Problem', 'op args terms seed inp full t ref shares')


@functools.lru_cache(maxsize=None)
def problem(op, ci, terms):
    """Inputs, operands and float64 reference of OPS[op].cases[ci] with the term set `terms` (a frozenset), built once per process
    and never modified: the first seed of a fixed list at which every term of the set is visible."""
    args = OPS[op]['cases'][ci].args
    atol, rtol = tolerance(op, ci)
    base = 1000 * (sorted(OPS).index(op) + 1) + 10 * ci
    tried = []
    for k in range(SEED_TRIES):
        seed = base + 100000 * k
        inp = make_inputs(op, args, seed)
        full = op_ref(op, args, inp)
        acc = _acc(full)
        N, C, H, W = acc.shape
        t = make_operands(N, C, H, W, terms, seed)
        shares = {term: visible_share(acc, t, term, atol, rtol) for term in TERMS if term in terms}
        tried.append(shares)
        if all(v >= VISIBLE_SHARE for v in shares.values()):
            return Problem(op, args, terms, seed, inp, full, t, ref_epilogue(acc, t), shares)
    raise AssertionError('%s case %d %s: no seed of %d shows every term: %s' % (op, ci, term_id(terms), SEED_TRIES, tried[-3:]))


def f32_gap(p):
    """max |float32 torch-CPU reference - float64 reference| of a problem: the yardstick of the "more room" rule (4 x this)."""
    acc32 = _acc(op_ref(p.op, p.args, p.inp, torch.float32))
    return float((ref_epilogue(acc32, p.t).double() - p.ref).abs().max())
