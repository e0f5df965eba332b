"""The optimizer kernels themselves against the float64 statements of tests/optim_shadow.py: FlatAdam and FlatSGD over several
steps with every step audited, and mspl_adam_step through its C ABI on raw buffers with sentinels around them."""
import ctypes

import numpy as np
import pytest
import torch

from tests import optim_shadow as S

pytestmark = pytest.mark.gpu
DEV = 'cuda'
EPS = 1e-8


def _parameters(arrays, nograd_at):
    """[(name, Parameter)] on the device with one gradient-less parameter in front of position `nograd_at`."""
    named = [('p%d' % i, torch.nn.Parameter(torch.from_numpy(a.copy()).to(DEV))) for i, a in enumerate(arrays)]
    g = torch.Generator().manual_seed(77)
    named.insert(nograd_at, ('nograd', torch.nn.Parameter(torch.randn(S.NOGRAD_SIZE, generator=g).to(DEV))))
    return named


def _load_grads(named, grads, first):
    it = iter(grads)
    for n, p in named:
        if n == 'nograd':
            continue
        g = torch.from_numpy(next(it)).to(DEV)
        if first:
            p.grad = g.clone()
        else:
            p.grad.copy_(g)          # (a view of the optimizer's flat gradient buffer by now)


@pytest.mark.parametrize('wd', [0.0, 5e-4])
@pytest.mark.parametrize('betas', [(0.9, 0.999), (0.8, 0.99)])
def test_flat_adam_six_steps_against_float64(betas, wd):
    from mspl_amd.training import FlatAdam
    params, grads = S.input_set()
    named = _parameters(params, S.NOGRAD_AT)
    by = dict(named)
    frozen = by['nograd'].detach().clone()
    with S.StepAudit() as audit:
        audit.watch(by)
        _load_grads(named, grads[0], True)
        opt = FlatAdam([p for _, p in named], lr=S.LRS[0], betas=betas, eps=EPS, weight_decay=wd)
        assert len(opt.params) == len(S.SIZES) and opt.bucket.numel_params == sum(S.SIZES) <= opt.flat_p.numel()
        assert all(p.data_ptr() % 16 == 0 and p.grad.data_ptr() % 16 == 0 for p in opt.params)
        for s in range(S.STEPS):
            if s:
                _load_grads(named, grads[s], False)
            opt.param_groups[0]['lr'] = S.LRS[s]          # as adjust_learning_rate writes it (changes before steps 3 and 4)
            if s == S.STEPS - 1:                           # GraphedTrainStep.reset_optimizer: a fresh Adam from here on
                opt.m.zero_()
                opt.v.zero_()
                opt.step_count = 0
            opt.step()
            audit.check(by, label='FlatAdam betas=%s wd=%g' % (betas, wd))
    assert audit.steps == [(s + 1, [S.LRS[s]]) for s in range(S.STEPS - 1)] + [(1, [S.LRS[-1]])]
    last = audit.records[-1]
    assert not last.pre[2].any() and not last.pre[3].any()
    nograd = by['nograd']
    assert nograd.grad is None and torch.equal(nograd.detach().view(torch.int32), frozen.view(torch.int32))


SENTINEL = 12345.678
PAD = 32


def _raw_case(n, seed):
    rng = np.random.default_rng(seed)
    p = rng.standard_normal(n).astype(np.float32)
    g = (rng.standard_normal(n) * np.asarray(S.GRAD_SCALES)[rng.integers(0, len(S.GRAD_SCALES), n)]).astype(np.float32)
    m = (rng.standard_normal(n) * 0.1 * np.abs(g)).astype(np.float32)
    v = (rng.random(n) * g.astype(np.float64) ** 2).astype(np.float32)
    if n >= 3:
        g[n // 2] = 0.0
    return p, g, m, v


def _raw_adam(arrays, n, off, step, lr, betas, wd):
    """mspl_adam_step on buffers 64 floats longer than n, the data starting `off` floats in; returns the four buffers whole."""
    from mspl_amd._native import check, lib
    bufs = []
    for a in arrays:
        t = torch.full((n + 2 * PAD,), SENTINEL, dtype=torch.float32, device=DEV)
        t[off:off + n] = torch.from_numpy(a).to(DEV)
        bufs.append(t)
    ptr = [ctypes.c_void_p(t.data_ptr() + 4 * off) for t in bufs]
    check(lib.mspl_adam_step(ptr[0], ptr[1], ptr[2], ptr[3], n, lr, betas[0], betas[1], EPS, wd, step,
                             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in bufs]


@pytest.mark.parametrize('step', [1, 2, 10, 1000, 100000])
def test_adam_kernel_through_the_c_abi(step):
    """Every n around the 256-thread block, the bias corrections at small and very large step counts, nothing written outside
    [0, n), and a start that is only 4-byte aligned gives bit-identical numbers."""
    lr, betas, wd = 1e-2, (0.9, 0.999), 5e-4
    worst = [0.0, 0.0, 0.0]
    for n in (0, 1, 255, 256, 257, 4097):
        arrays = _raw_case(n, 100 + n)
        out = {}
        for off in (PAD, PAD + 1):
            res = _raw_adam(arrays, n, off, step, lr, betas, wd)
            for t in res:
                outside = np.concatenate([t[:off], t[off + n:]])
                assert np.array_equal(outside, np.full(outside.shape, SENTINEL, dtype=np.float32)), (n, off)
            assert np.array_equal(res[1][off:off + n], arrays[1])                   # the gradient is read-only
            out[off] = [t[off:off + n] for t in res]
        for a, b in zip(out[PAD], out[PAD + 1]):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (n, 'aligned and unaligned starts differ')
        if n == 0:
            continue
        p1, m1, v1, tol_p, tol_m, tol_v = S.adam_bounds(*arrays, lr=lr, betas=betas, eps=EPS, wd=wd, step=step)
        got = out[PAD]
        for k, (what, a, want, tol) in enumerate((('p', got[0], p1, tol_p), ('m', got[2], m1, tol_m), ('v', got[3], v1, tol_v))):
            err = np.abs(a.astype(np.float64) - want)
            i = int(np.argmax(err / tol))
            worst[k] = max(worst[k], float(err[i] / tol[i]))
            assert (err <= tol).all(), ('%s n=%d step=%d: element %d is %.9g, float64 says %.9g, error %.3g > bound %.3g'
                                        % (what, n, step, i, a[i], want[i], err[i], tol[i]))
    print('mspl_adam_step step=%d: worst error/bound p %.3f m %.3f v %.3f' % ((step,) + tuple(worst)))


def test_adam_kernel_refuses_step_zero_and_null_pointers():
    from mspl_amd._native import check, lib
    t = [torch.zeros(8, device=DEV) for _ in range(4)]
    ptr = [ctypes.c_void_p(x.data_ptr()) for x in t]
    with pytest.raises(RuntimeError, match='step=0'):
        check(lib.mspl_adam_step(ptr[0], ptr[1], ptr[2], ptr[3], 8, 1e-3, 0.9, 0.999, EPS, 0.0, 0, None))
    for k in range(4):
        args = list(ptr)
        args[k] = None
        with pytest.raises(RuntimeError, match='null pointer'):
            check(lib.mspl_adam_step(args[0], args[1], args[2], args[3], 8, 1e-3, 0.9, 0.999, EPS, 0.0, 1, None))
    torch.cuda.synchronize()
    assert all(not x.any() for x in t)


def test_flat_sgd_groups_across_blocks_against_float64():
    """Three groups whose spans straddle 256-element boundaries; group two without momentum, group three without weight decay, a
    gradient-less parameter inside group one, leftovers in the buffer when the first step arrives, one lr changed before step 3."""
    from mspl_amd.supervised import FlatSGD
    shapes = [(257,), (3,), (1000,), (255,), (1,), (4097,)]
    scales = [10.0, 1.0, 1e-5, 1e-3, 1.0, 1.0]
    rng = np.random.default_rng(4321)
    named = _parameters([rng.standard_normal(s).astype(np.float32) for s in shapes], 2)      # nograd between (3,) and (1000,)
    by = dict(named)
    frozen = by['nograd'].detach().clone()

    def grads():
        out = []
        for s, sc in zip(shapes, scales):
            g = (rng.standard_normal(s) * sc).astype(np.float32)
            if s[0] >= 3:
                g[-1] = 0.0
            out.append(g)
        return out

    with S.StepAudit() as audit:
        audit.watch(by)
        _load_grads(named, grads(), True)
        opt = FlatSGD([{'params': [by['p0'], by['p1'], by['nograd'], by['p2']], 'lr': 0.05},
                       {'params': [by['p3'], by['p4']], 'lr': 0.5, 'momentum': 0.0},
                       {'params': [by['p5']], 'lr': 0.1, 'weight_decay': 0.0}], lr=0.5, momentum=0.9, weight_decay=5e-4)
        assert len(opt.params) == 6 and [len(g['params']) for g in opt.param_groups] == [3, 2, 1]
        assert all(p.data_ptr() % 16 == 0 and p.grad.data_ptr() % 16 == 0 for p in opt.params)
        spans = [(g['_lo'], g['_hi']) for g in opt.param_groups]
        assert spans == [(0, 260 + 4 + 1000), (1264, 1264 + 256 + 4), (1524, 1524 + 4100)] and opt.flat_p.numel() == 5624
        junk = torch.from_numpy(rng.standard_normal(opt.buf.numel()).astype(np.float32)).to(DEV)
        for o, p in zip(opt.bucket.offsets, opt.params):      # (the alignment padding stays zero)
            opt.buf[o:o + p.numel()] = junk[o:o + p.numel()]
        for s in range(4):
            if s:
                _load_grads(named, grads(), False)
            if s == 2:
                opt.param_groups[0]['lr'] = 0.02                # an epoch boundary: set_epoch_learning_rates
            opt.step()
            audit.check(by, label='FlatSGD')
    assert audit.steps == [(1, [0.05, 0.5, 0.1]), (2, [0.05, 0.5, 0.1]), (3, [0.02, 0.5, 0.1]), (4, [0.02, 0.5, 0.1])]
    assert by['nograd'].grad is None and torch.equal(by['nograd'].detach().view(torch.int32), frozen.view(torch.int32))
