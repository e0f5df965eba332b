"""Every forward kernel form against float64 on every epilogue term (the table: tests/epilogue_cases.py).

An entry point either applies a term exactly as epi_apply does or refuses it on the host.  Per op x form x accepted term set: the
result against the float64 reference built from the same float32 inputs; into a channel slice of a sentinel-filled destination
(nothing outside the slice changes, the slice is bit-identical to the un-sliced call with the constants at the same absolute
channels); raw_out where accepted (bit-identical to the call without an epilogue, the activated output bit-identical to the call
without raw_out); a neutral further operand where a term moves the call off a lean form; and for every refused term: RuntimeError,
the destination untouched, the next valid call on the stream still right.

Every operand is a whole, freshly allocated tensor of exactly the size the kernel indexes."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests import epilogue_cases as ec

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENT = -7.25                     # sentinel of a destination (exact in float32; no reference value is exactly this)
EXTRA, COFF = 5, 3               # a sliced destination has EXTRA more channels, the op's start at COFF

BARE = frozenset()
CONTRACT = [(op, ci, ts) for op in ec.CONTRACT_OPS for ci in range(len(ec.OPS[op]['cases'])) for ts in [BARE] + ec.termsets(op)]
SLICES = [(op, ci, ts) for op in ec.CONTRACT_OPS for ci in range(len(ec.OPS[op]['cases']))
          for ts in dict.fromkeys([ec.AFFINE & ec.OPS[op]['accepts'], ec.termsets(op)[-1]])]
RAWS = [(op, ci, ts) for op in ec.RAW_OPS for ci in range(len(ec.OPS[op]['cases']))
        for ts in dict.fromkeys([ec.AFFINE, frozenset(t for t in ec.TERMS if t in ec.OPS[op]['accepts'])])]
REFUSALS = [(op, term) for op in ec.REFUSING_OPS for term in sorted(ec.OPS[op]['refuses'])]


def _id(v):
    return '%s-%d-%s' % (v[0], v[1], ec.term_id(v[2]))


def dv(v):
    if isinstance(v, torch.Tensor):
        return v.to(DEV)
    if isinstance(v, dict):
        return {k: dv(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [dv(x) for x in v]
    return v


def epi(t, raw_out=None):
    from mspl_amd.ops import Epi
    return Epi(t.get('scale'), t.get('shift'), t.get('alpha'), t.get('pre_add'), t.get('residual'), t.get('reinf_r'), t.get('reinf_w'),
               t.get('gate'), raw_out)


def sentinel(*shape):
    return torch.full(shape, SENT, device=DEV)


def untouched(t):
    torch.cuda.synchronize()
    return bool((t == SENT).all())


def check64(got, ref, tol, what):
    """|got - ref| <= atol + rtol |ref| everywhere; prints the worst fraction of the allowance first."""
    atol, rtol = tol
    assert tuple(got.shape) == tuple(ref.shape), (what, tuple(got.shape), tuple(ref.shape))
    g = got.double().cpu()
    assert torch.isfinite(g).all(), what
    err = (g - ref).abs()
    frac = float((err / (atol + rtol * ref.abs())).max())
    print('%s: max |kernel - float64| %.3e, worst fraction of the allowance %.3f' % (what, float(err.max()), frac))
    assert frac <= 1.0, what


# ------------------------------------------------------------------ one call of each entry point
def _pointwise(x, ep, out):
    """mspl_pointwise_fwd reads its input in the destination's geometry: for a slice, x sits at the same channels of a tensor as wide."""
    from mspl_amd import ops
    if out is None:
        return ops.pointwise(x, ep)
    dst, coff = out
    N, C = x.shape[:2]
    hw = x[0, 0].numel()
    xin = torch.full_like(dst, 0.5)
    xin[:, coff:coff + C] = x
    s, keep = ops._build(ep, dst, coff, N, C, hw)
    ops.check(ops.lib.mspl_pointwise_fwd(ops._p(xin), N, C, hw, ctypes.byref(s), ops._p(dst), ops._stream()))
    return dst


def _pyrpool(train, args, I, ep, out, aux):
    from mspl_amd import ops
    N, P, h, w = args
    sizes = ec.pyr_sizes(h, w)
    nb = len(sizes)
    hs = (ctypes.c_int32 * nb)(*[s[0] for s in sizes])
    ws = (ctypes.c_int32 * nb)(*[s[1] for s in sizes])
    sw, de = (ctypes.c_void_p * nb)(), (ctypes.c_void_p * nb)()
    for i in range(nb):
        if i in I['down_e']:
            assert tuple(I['down_e'][i].shape) == (N, P) + sizes[i]
            de[i] = I['down_e'][i].data_ptr()
        else:
            sw[i] = I['stage_w'][i].data_ptr()
    dst, coff = out if out is not None else (torch.empty((N, P, h, w), device=DEV), 0)
    s, keep = ops._build(ep, dst, coff, N, P, h * w)
    common = (ops._p(I['x']), N, P, h, w, nb, hs, ws, sw, de, ops._p(I['br_scale']), ops._p(I['br_shift']), ops._p(I['br_alpha']),
              ops._p(I['merge_w']), ctypes.byref(s), ops._p(dst))
    if train:
        aux['zcat'] = sentinel(N, nb * P, h, w)
        ops.check(ops.lib.mspl_pyrpool_fused_train_fwd(*common, ops._p(aux['zcat']), ops._stream()))
    else:
        ops.check(ops.lib.mspl_pyrpool_fused_fwd(*common, ops._stream()))
    return dst


def _eesp_dw_exp(op, args, I, ep, out, aux):
    """The C entry points directly (ops.eesp_dw_exp allocates its own destination): a destination and a slice of the caller's."""
    from mspl_amd import ops
    N, n, H, W, dil = args
    packed = ops.eesp_dw_exp_pack(I['w'], I['bs'], I['bb'], I['ba'], I['wexp'], H, W, dil)
    dst, coff = out if out is not None else (torch.empty((N, 4 * n, H, W), device=DEV), 0)
    s, keep = ops._build(ep, dst, coff, N, 4 * n, H * W)
    d = (ctypes.c_int32 * 4)(*dil)
    if op == 'eesp_dw_exp':
        ops.check(ops.lib.mspl_eesp_dw_exp_fwd(ops._p(I['r']), ops._p(packed), d, N, n, H, W, ctypes.byref(s), ops._p(dst), ops._stream()))
    else:
        npk = ops.eesp_dw_exp_next_pack(I['w1'])
        aux['rnext'] = sentinel(N, n, H, W)
        ops.check(ops.lib.mspl_eesp_dw_exp_next_fwd(ops._p(I['r']), ops._p(packed), d, N, n, H, W, ctypes.byref(s), ops._p(dst), ops._p(npk),
                                                    ops._p(I['ns']), ops._p(I['nb']), ops._p(I['na']), ops._p(aux['rnext']), ops._stream()))
    return dst


def run(op, args, I, ep=None, out=None):
    """One call of the op's entry point with inputs I (on the device), an ops.Epi or None, out = (destination, channel offset) or None.
    Returns (destination, further outputs)."""
    from mspl_amd import ops
    aux = {}
    if op == 'conv3x3':
        N, Cin, Cout, G, H, W, stride, sg = args
        y = ops.conv3x3(I['x'], I['w'], G, stride, sg, ep, out)
    elif op == 'conv1x1':
        y = ops.conv1x1(I['x'], I['w'], args[3], ep, out)
    elif op == 'bilinear':
        y = ops.bilinear(I['x'], args[1], ep, out, align_corners=args[2])
    elif op == 'avgpool3x3s2':
        y = ops.avgpool3x3s2(I['x'], ep, out)
    elif op == 'avgpool3x3s2_psum':
        y, aux['sums'] = ops.avgpool3x3s2(I['x'], ep, out, plane_sums=True)
    elif op == 'adaptive_avgpool':
        y = ops.adaptive_avgpool(I['x'], args[1], ep, out)
    elif op == 'pointwise':
        y = _pointwise(I['x'], ep, out)
    elif op in ('pyrpool_fused', 'pyrpool_fused_train'):
        y = _pyrpool(op == 'pyrpool_fused_train', args, I, ep, out, aux)
    elif op == 'eesp_dw_hff':
        N, n, H, W, dil, stride, stream = args
        with ops.launch_flags(k2_stream=stream):
            y = ops.eesp_dw_hff(I['x'], I['w'], dil, stride, ep, out)
    elif op == 'eesp_proj_dw_hff':
        N, Cin, n, G, H, W, dil = args
        y = ops.eesp_proj_dw_hff(I['x'], I['wp'], I['ps'], I['pb'], I['pa'], I['w'], dil, G, ep, out)
    elif op in ('eesp_dw_exp', 'eesp_dw_exp_next'):
        y = _eesp_dw_exp(op, args, I, ep, out, aux)
    elif op == 'down_head':
        N, nin, n, G, H, W = args
        y = out[0]
        aux['r'], aux['sums'] = ops.down_head(I['x'], I['wp'], I['ps'], I['pb'], I['pa'], G, ep, y)
    elif op == 'dense_conv':
        N, Cin, Cout, H, W, k, d = args
        y = ops.dense_conv(I['x'], ops.pack_dense_weight(I['w']), k, d, ep, out)
    elif op == 'dense_conv_split':
        x, pack, k, d = I
        y = ops.dense_conv_split(x, pack, k, d, ep, out)
    else:
        raise KeyError(op)
    return y, aux


def check_aux(p, ci, aux):
    """The further outputs of a call: the input's plane sums, the kept branch values of the training pyramid."""
    if 'sums' in aux and p.op == 'avgpool3x3s2_psum':
        x = p.inp['x']
        torch.testing.assert_close(aux['sums'].sum(1).cpu().view(x.shape[0], x.shape[1]), x.double().sum((2, 3)).float(), rtol=1e-5, atol=1e-3)
    if 'zcat' in aux:
        check64(aux['zcat'], p.full['zcat'], ec.tolerance(p.op, ci), 'kept branch values')


# ------------------------------------------------------------------ accepted terms
@pytest.mark.parametrize('case', CONTRACT, ids=_id)
def test_terms_against_float64(case):
    """The op with one term set (nothing, each accepted term alone, the sets the forms are keyed on, all terms) against float64."""
    op, ci, ts = case
    p = ec.problem(op, ci, ts)
    y, aux = run(op, p.args, dv(p.inp), epi(dv(p.t)) if ts else None)
    check64(y, p.ref, ec.tolerance(op, ci, bare=not ts), _id(case))
    check_aux(p, ci, aux)


@pytest.mark.parametrize('case', SLICES, ids=_id)
def test_channel_slice(case):
    """Into channels [COFF, COFF + C) of a sentinel-filled destination with EXTRA more channels, every operand in that geometry with
    its values at the same ABSOLUTE channels: nothing outside the slice changes, the slice is bit-identical to the un-sliced call."""
    op, ci, ts = case
    p = ec.problem(op, ci, ts)
    I = dv(p.inp)
    N, C, H, W = p.ref.shape
    plain, _ = run(op, p.args, I, epi(dv(p.t)))
    dst = sentinel(N, C + EXTRA, H, W)
    run(op, p.args, I, epi(dv(ec.embed(p.t, C, C + EXTRA, COFF))), out=(dst, COFF))
    assert untouched(dst[:, :COFF]) and untouched(dst[:, COFF + C:]), 'wrote outside the channel slice'
    check64(dst[:, COFF:COFF + C], p.ref, ec.tolerance(op, ci), _id(case))
    assert torch.equal(dst[:, COFF:COFF + C], plain), 'the slice differs from the un-sliced call'


def _raw_pairs_share_a_form(op, ci, ts):
    """(raw_out vs the call without an epilogue, activated output vs the call without raw_out): whether the two calls of the pair
    take the same kernel form.  Two forms are keyed on the terms themselves: split-K conv1x1 takes AFFINE at most (the bare call is
    split-K, the call with further terms is not), the training pyramid's streaming form AFFINE at most AND raw_out."""
    form = ec.OPS[op]['cases'][ci].form
    if op == 'pyrpool_fused_train' and 'streaming' in form:
        return ts == ec.AFFINE, ts != ec.AFFINE
    if op == 'conv1x1' and form == 'split-K':
        return ts == ec.AFFINE, True
    return True, True


@pytest.mark.parametrize('case', RAWS, ids=_id)
def test_raw_out(case):
    """raw_out receives the bare result: bit-identical to the call without an epilogue; the activated output is bit-identical to the
    call without raw_out; all of them against float64.  For the training pyramid the call that keeps only the bare result is the
    'call without an epilogue' (as the training step issues it).  A pair of calls that spans two kernel forms
    (_raw_pairs_share_a_form) is held to the float64 bound alone."""
    op, ci, ts = case
    p = ec.problem(op, ci, ts)
    I = dv(p.inp)
    t = dv(p.t)
    acc = p.full['acc'] if isinstance(p.full, dict) else p.full
    tol, tol_bare = ec.tolerance(op, ci), ec.tolerance(op, ci, bare=True)
    same_raw, same_act = _raw_pairs_share_a_form(op, ci, ts)
    raw = sentinel(*acc.shape)
    both, aux = run(op, p.args, I, epi(t, raw_out=raw))
    act, _ = run(op, p.args, I, epi(t))
    if op == 'pyrpool_fused_train':
        raw0 = sentinel(*acc.shape)
        bare, _ = run(op, p.args, I, epi({}, raw_out=raw0))
        assert torch.equal(raw0, bare)
    else:
        bare, _ = run(op, p.args, I, None)
    check64(raw, acc, tol_bare, _id(case) + ' raw')
    check64(bare, acc, tol_bare, _id(case) + ' bare')
    check64(both, p.ref, tol, _id(case) + ' activated')
    check64(act, p.ref, tol, _id(case) + ' without raw_out')
    check_aux(p, ci, aux)
    if same_raw:
        assert torch.equal(raw, bare), 'raw_out differs from the call without an epilogue'
    if same_act:
        assert torch.equal(both, act), 'raw_out changed the activated output'


# ------------------------------------------------------------------ a term that moves the call off a lean form
@pytest.mark.parametrize('case', ec.FALLBACKS, ids=_id)
def test_neutral_operand_leaves_the_lean_form(case):
    """Split-K conv1x1, the streaming / separable pyramid and the DownSampler's lean pool exist for one term set only.  With a zero
    pre_add, a zero residual or an all-ones gate added the call takes the general form: same float64 bound as the lean result."""
    op, ci, ts = case
    p = ec.problem(op, ci, ts)
    I = dv(p.inp)
    t = dv(p.t)
    N, C, H, W = p.ref.shape
    lean, aux = run(op, p.args, I, epi(t))
    check64(lean, p.ref, ec.tolerance(op, ci), _id(case) + ' lean')
    check_aux(p, ci, aux)
    neutral = {'pre_add': torch.zeros(N, C, H, W, device=DEV), 'residual': torch.zeros(N, C, H, W, device=DEV),
               'gate': torch.ones(N, C, device=DEV)}
    for name, v in neutral.items():
        y, aux = run(op, p.args, I, epi(dict(t, **{name: v})))
        check64(y, p.ref, ec.tolerance(op, ci), _id(case) + ' + neutral ' + name)
        check_aux(p, ci, aux)


# ------------------------------------------------------------------ refused terms
def _refusal_problem(op):
    """(args, device inputs, valid operands in the destination's geometry, destination channels, float64 references, tolerance)."""
    if op == 'dense_conv_split':
        from mspl_amd import ops
        from tests.split_cases import C_SPLIT, reference
        index, planes = ec.OPS[op]['cases'][0].args
        ref = reference(index)
        N, Cin, Cout, H, W, k, d = ref['shape']
        I = (ref['x'].to(DEV), ops.pack_dense_weight_split(ref['w'], planes).to(DEV), k, d)
        return None, I, {}, Cout, {'y': ref['true'], 'allow': C_SPLIT[planes] * ref['mag'] + 4.0 * ref['e32']}, None
    p = ec.problem(op, 0, ec.termsets(op)[-1])
    N, C, H, W = p.ref.shape
    ctot, t = C, p.t
    if op == 'down_head':                               # the pool fills channels [0, nin) of the block's nout = nin + 4 n
        ctot = p.args[1] + 4 * p.args[2]
        t = ec.embed(p.t, C, ctot, 0)
    return p.args, dv(p.inp), t, ctot, {'y': p.ref, 'p': p}, ec.tolerance(op, 0)


@pytest.mark.parametrize('op,term', REFUSALS, ids=['%s-%s' % v for v in REFUSALS])
def test_refused_term_is_refused(op, term):
    """A term the entry point does not implement is refused on the host (MSPL_ERR_UNSUPPORTED -> RuntimeError) before anything is
    launched: the sentinel-filled destination is unchanged, and the next valid call on the same stream still matches float64."""
    args, I, t, ctot, refs, tol = _refusal_problem(op)
    N, C, H, W = refs['y'].shape
    bad_ctot, coff, raw = ctot, 0, None
    bad = dict(t)
    if term == 'slice':
        bad_ctot, coff = C + EXTRA, COFF
        bad = ec.embed(t, C, bad_ctot, coff)
    elif term == 'raw_out':
        raw = sentinel(N, C, H, W)
    else:
        more = ec.make_operands(N, C, H, W, frozenset((term,)), 3)
        bad.update(more if ctot == C else ec.embed(more, C, ctot, 0))
    dst = sentinel(N, bad_ctot, H, W)
    with pytest.raises(RuntimeError) as err:
        run(op, args, I, epi(dv(bad), raw_out=raw), out=(dst, coff))
    assert '(-2)' in str(err.value) or (term == 'raw_out' and 'raw_out must be' in str(err.value)), str(err.value)
    assert untouched(dst) and (raw is None or untouched(raw)), 'a refused call wrote to its destination'
    # the next valid call
    good = sentinel(N, ctot, H, W)
    y, aux = run(op, args, I, epi(dv(t)) if t else None, out=(good, 0))
    if op == 'dense_conv_split':
        errs = (y.double().cpu() - refs['y']).abs()
        assert torch.all(errs <= refs['allow'])
        return
    check64(y[:, :C], refs['y'], tol, '%s after a refused %s' % (op, term))
    assert untouched(good[:, C:])
    p = refs['p']
    if op == 'down_head':
        check64(aux['r'], p.full['r'], tol, 'down_head reduced tensor')
        torch.testing.assert_close(aux['sums'].sum(1).cpu().view(N, C), p.full['sums'].float(), rtol=1e-5, atol=1e-3)
    if op == 'eesp_dw_exp_next':
        n = p.args[1]
        rn = F.conv2d(p.ref, p.inp['w1'].double(), None, 1, 0, 1, 4)
        rn = rn * p.inp['ns'].double().view(1, -1, 1, 1) + p.inp['nb'].double().view(1, -1, 1, 1)
        rn = torch.where(rn > 0, rn, rn * p.inp['na'].double().view(1, -1, 1, 1))
        check64(aux['rnext'], rn, tol, 'next projection (n = %d)' % n)
