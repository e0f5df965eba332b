"""The batch-statistics BatchNorm kernels (every BatchNorm of the supervised loop in train() mode) at ill-conditioned channels and at
the seams between and inside their three forms, against float64 (tests/bn_cases.py: the oracle, the channel classes, the shapes and
the bounds; tests/test_bn_cases.py holds those to their conditions on the host).

Every comparison is per channel:  |kernel - float64| <= MARGIN * max(err32, 2**-23 * magnitude)  with err32 the float32 oracle's own
error on the CPU and the magnitude taken from float64 (bn_cases.bounds says which).  Nothing is left out of a comparison: the generator
keeps every pre-activation out of a band around 0 in which a float32 result inside the bound could take the other PReLU slope.  Each
test prints the worst error / bound per quantity; eager launches only (no graph capture, no side streams)."""
import collections
import math

import numpy as np
import pytest
import torch

from tests import bn_cases as bc

pytestmark = pytest.mark.gpu
DEV = 'cuda'
WORST = collections.defaultdict(dict)           # form -> quantity -> worst error / bound seen in this run


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    for form in sorted(WORST):
        print('\nBN conditioning, worst error / bound, %s form: %s'
              % (form, '  '.join('%s %.3f' % kv for kv in sorted(WORST[form].items()))))


def _ws_is_zero(bn):
    """Every byte of the module's persistent workspace(s) is 0: what both fused kernels promise to hand back."""
    tab = bn.__dict__.get('_mspl_bn_ws')
    assert tab, 'the module has no workspace'
    for ws in tab.values():
        assert int(torch.count_nonzero(ws.view(torch.uint8))) == 0, 'workspace not handed back zeroed'


def _saved(fn, i):
    return fn.saved_tensors[i].detach().clone()


def _call(bn, inp, shape, backward=True, sinks=False, check_ws=False):
    """One call of the node (or of the plain pair) on the module: {quantity: result on the device}."""
    from mspl_amd import autograd as ag
    from mspl_amd._native import lib
    N, C, H, W = shape.dims
    assert ag._SMALL_BN and bool(lib.mspl_bn_train_small_fits(N, C, H * W)) == shape.small
    idx = bc.channel_index(shape)
    dev = lambda t: None if t is None else bc.expand(t.to(DEV), idx).contiguous()      # noqa: E731
    z, res, gy, al = [dev(inp[k]) for k in ('z', 'residual', 'gy', 'alpha')]
    with torch.no_grad():
        bn.weight.copy_(dev(inp['gamma']))
        bn.bias.copy_(dev(inp['beta']))
    params = [bn.weight, bn.bias] + ([al] if al is not None else [])
    for t in [z, res, al] if backward else []:
        if t is not None:
            t.requires_grad_()
    for p in params:
        p.grad = torch.full_like(p, 0.5) if sinks else None
    got = {}
    with torch.set_grad_enabled(backward), ag.grad_sinks(enabled=sinks):
        if shape.form == 'pair':
            scale, shift = ag.bn_batch_stats(z, bn)
            y = ag.affine_prelu(z, scale, shift, al, residual=res)
            got.update(scale=scale.detach().clone(), shift=shift.detach().clone())
            if backward:
                got.update(mean=_saved(scale.grad_fn, 2), invstd=_saved(scale.grad_fn, 3))
        else:
            y = ag.bn_train_prelu(z, bn, al, res)
            if backward:
                st = _saved(y.grad_fn, 4)                   # the node's (mean, invstd, scale, shift) rows
                got.update(mean=st[0], invstd=st[1], scale=st[2], shift=st[3])
            if check_ws:
                _ws_is_zero(bn)
        if backward:
            y.backward(gy)
            if check_ws and shape.form != 'pair':
                _ws_is_zero(bn)
    got.update(y=y.detach(), running_mean=bn.running_mean.detach().clone(), running_var=bn.running_var.detach().clone())
    if backward:
        off = 0.5 if sinks else 0.0
        got.update(gz=z.grad, dgamma=bn.weight.grad - off, dbeta=bn.bias.grad - off)
        if res is not None:
            got['gres'] = res.grad
        if al is not None:
            got['dalpha'] = al.grad - off
    return got


def _check(tag, form, got, r64, bnd, idx, exclude=()):
    """Every quantity of `got` against float64 under its per-channel bound; prints the worst ratio of each, then asserts them all."""
    worst, missed = {}, []
    for q in sorted(got):
        if q in exclude:
            continue
        assert bool(torch.isfinite(got[q]).all()), (tag, q)
        r = bc.ratios(got[q], r64[q], bnd[q], idx)
        worst[q] = float(r.max())
        WORST[form][q] = max(WORST[form].get(q, 0.0), worst[q])
        if not worst[q] <= 1.0:
            missed.append((q, worst[q], int(r.argmax())))
    print('%s [%s]: error / bound  %s' % (tag, form, '  '.join('%s %.3f' % kv for kv in sorted(worst.items()))))
    assert not missed, '%s: (quantity, error / bound, channel) %s' % (tag, missed)


def _chain(cases, eps=bc.EPS, momentum=bc.MOMENTUM, backward=None, sinks=False, check_ws=False, exclude=()):
    """The cases one after the other on ONE module (its running statistics, counter and workspace carry over), each call against the
    oracle on the statistics the float64 oracle left before it.  -> [(inputs, float64 result, bounds, kernel results)]"""
    shapes = [bc.SHAPE[c.shape] for c in cases]
    C = shapes[0].dims[1]
    assert all(s.dims[1] == C for s in shapes)
    bn = torch.nn.BatchNorm2d(C, eps=eps, momentum=momentum).to(DEV).train()
    stats = {torch.float64: (None, None), torch.float32: (None, None)}
    out = []
    for i, (case, shape) in enumerate(zip(cases, shapes)):
        inp, r64, r32, bnd = bc.reference(case, i, eps, momentum)
        if i:
            r64 = bc.evaluate(inp, torch.float64, eps, momentum, *stats[torch.float64])
            r32 = bc.evaluate(inp, torch.float32, eps, momentum, *stats[torch.float32])
            bnd = bc.bounds(inp, r64, r32, eps, momentum, *stats[torch.float64])
        stats = {torch.float64: (r64['running_mean'], r64['running_var']), torch.float32: (r32['running_mean'], r32['running_var'])}
        bwd = True if backward is None else backward[i]
        got = _call(bn, inp, shape, bwd, sinks, check_ws)
        assert int(bn.num_batches_tracked) == i + 1
        _check('%s (call %d%s)' % (bc.case_id(case), i + 1, '' if bwd else ', forward only'), shape.form, got, r64, bnd,
               bc.channel_index(shape), exclude)
        out.append((inp, r64, bnd, got))
    return out


def _constant_channels(inp, r64, got):
    """A channel whose every element is one value v: mean == v exactly (the shifted sums are exactly 0), invstd == 1 / sqrt(eps)."""
    for c, cls in enumerate(inp['classes']):
        if cls == 'const' and 'mean' in got:
            assert float(got['mean'][c]) == 3.0
            assert float(got['invstd'][c]) == float(np.float32(1.0 / math.sqrt(float(np.float32(bc.EPS)))))


@pytest.mark.parametrize('case', bc.CASES, ids=bc.case_id)
def test_bn_node_at_conditioned_channels_and_seams(case):
    """Every seam shape of every form, with and without residual and alpha: y, gz, gres, d gamma, d beta, d alpha, the statistics and
    their fold, the running statistics and the counter.

    s_L1_scalar (two values per channel) is the shape that found the backward's double form: there xhat is +-1 whatever z is and
    gz = scale * (g' - mean g' - xhat mean(g' xhat)) cancels to eps / (var + eps) of its terms (float64: 6.3e-12 of terms of 9.5e-3 on
    the `huge` channel).  The float32 kernel was off by 0.3 * 2**-24 of a term there -- 7.1 x this bound, the float32 oracle happening
    to be exact -- and by 6.8 x on the offset64 channel, where its uncentred differences round at 2**-24 |mean| / std.  Channels of one
    or two values now take bn_train_few_bwd_kernel (moments taken again, statistics path centred and in double): 0.001 x."""
    (inp, r64, bnd, got), = _chain([case], check_ws=bc.SHAPE[case.shape].form != 'pair')
    if bc.SHAPE[case.shape].unique is None:
        _constant_channels(inp, r64, got)


@pytest.mark.parametrize('shape', ['s_odd', 's_2048_quads', 't_midplane', 'p_scalar3'])
@pytest.mark.parametrize('with_res', [True, False])
def test_all_zero_input(shape, with_res):
    """Every element 0.0 (a bias-free convolution of a blank input): scale = gamma / sqrt(eps) and shift = beta EXACTLY, mean 0."""
    case = bc.Case(shape, with_res, True, 'zeros')
    (inp, r64, bnd, got), = _chain([case])
    isf = torch.tensor(1.0 / math.sqrt(float(np.float32(bc.EPS))), dtype=torch.float64).float()
    assert torch.equal(got['scale'].cpu(), inp['gamma'] * isf) and torch.equal(got['shift'].cpu(), inp['beta'])
    assert not bool(got['mean'].any()) and not bool(got['running_mean'].any())
    if not with_res:
        assert torch.equal(got['y'].cpu(), torch.where(inp['beta'] > 0, inp['beta'], inp['alpha'] * inp['beta'])[None, :, None, None]
                           .expand_as(got['y']))


A, B = bc.Case('t_first', True, True, 'classes'), bc.Case('t_midplane', False, True, 'classes')


@pytest.mark.parametrize('order', [(A, B), (B, A)], ids=['scalar-then-quads', 'quads-then-scalar'])
def test_second_call_on_one_module_two_launch_form(order):
    """Two shapes on one module: another N, another number of ranges (80 and 20 forward, 48 and 20 backward), scalar units and quads,
    with and without the residual's backward (gc + pointwise | apply).  Both calls inside the bounds, the running statistics those of
    two updates, the counter 2, and the workspace all zero after each forward and each backward."""
    _chain(list(order), check_ws=True)


def test_forward_only_call_then_training_call():
    """A no_grad forward in train() mode between two training steps (validation that leaves the module in train()): the next forward
    and backward find the workspace zeroed and the statistics advanced."""
    _chain([A, B, A], backward=[False, True, True], check_ws=True)


def test_small_then_two_launch_then_small_on_one_module():
    _chain([bc.Case('s_largest', True, True, 'classes'), B, bc.Case('s_odd', True, True, 'classes')], check_ws=True)


@pytest.mark.parametrize('shape', ['s_odd', 't_midplane', 'p_scalar3'])
def test_eps_and_momentum_are_the_modules(shape):
    """eps = 1e-3, momentum = 0.01, two calls (the second update weighs the first by 0.99)."""
    _chain([bc.Case(shape, True, True, 'classes'), bc.Case(shape, False, True, 'classes')], eps=1e-3, momentum=0.01)


@pytest.mark.parametrize('shape', ['s_2048_quads', 's_odd', 't_midplane', 't_first'])
@pytest.mark.parametrize('with_res', [True, False])
def test_gradient_sinks_accumulate(shape, with_res):
    """Inside grad_sinks() d gamma, d beta and d alpha are ADDED to the .grad buffers (0.5 everywhere beforehand; accumulate = 1 of
    the kernels): what was added is inside the same bounds (compare test_fused_pyramid_training_with_gradient_sinks).  The sum
    0.5 + d rounds once more: half an ulp of it, which the bound's unit (sum of |summands| >= |d|) covers from a few elements on."""
    _chain([bc.Case(shape, with_res, True, 'classes')], sinks=True)


@pytest.mark.parametrize('with_res', [True, False])
def test_one_value_per_channel(with_res):
    """M = 1 (torch refuses the shape; the kernels take var = 0 and update the running variance with the biased variance): finite
    outputs, mean == z, invstd == 1 / sqrt(eps), y == PReLU(beta + residual) and every other quantity inside its bound.  gz is exactly 0
    in float64 (a zero bound); the kernel's is held to the rounding of its summands scale * g'."""
    case = bc.Case('s_M1', with_res, True, 'classes')
    (inp, r64, bnd, got), = _chain([case], exclude=('gz',))
    assert torch.equal(got['mean'].cpu(), inp['z'].flatten())
    assert torch.equal(got['invstd'].cpu(), torch.full((8,), float(np.float32(1.0 / math.sqrt(float(np.float32(bc.EPS)))))))
    assert torch.equal(got['running_var'].cpu(), torch.full((8,), float(np.float32(1.0 - float(np.float32(bc.MOMENTUM))))))
    want = inp['beta'].double() + (inp['residual'].double().flatten() if with_res else 0.0)
    want = torch.where(want > 0, want, inp['alpha'].double() * want)
    assert float(((got['y'].cpu().double().flatten() - want).abs() / bnd['y']).max()) <= 1.0
    assert not bool(r64['gz'].any()) and bool(torch.isfinite(got['gz']).all())
    unit = bc.MARGIN * bc.FLOOR * (1.0 + bc.conditioning(inp['z'], r64)) * (r64['scale'] * r64['gu'].flatten()).abs()
    ratio = float((got['gz'].cpu().double().flatten().abs() / unit).max())
    print('M = 1: |gz| / (MARGIN * 2**-23 * (1 + R) * |scale g\'|) = %.3f' % ratio)
    assert ratio <= 1.0
