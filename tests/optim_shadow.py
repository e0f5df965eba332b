"""Float64 statements of ONE optimizer step, derived elementwise error bounds, and an audit of the steps a test takes.

Two runs of the same Adam steps cannot be compared tightly (float atomics land in another order, Adam turns rounding-noise
gradients into +-lr moves: tests.synth.assert_weights_close_after_adam).  One step can: its inputs -- parameter, final gradient,
moments, hyper-parameters, step count -- are known exactly, so the kernel's result is compared with the float64 value of the same
formula AT THOSE INPUTS and rounding has no room to grow.  `StepAudit` records those inputs and results around every
`FlatAdam.step` / `FlatSGD.step` of a test; `check()` compares every element of every tensor, by name.

Plain numpy / torch: nothing of the product or of the oracle is imported at module level.
"""
import os

import numpy as np

EPS32 = 2.0 ** -24          # unit round-off of float32
MARGIN_ADAM = 16.0          # over first-order rounding of the dozen float32 operations of the Adam kernel
MARGIN_SGD = 8.0

# Worst error / bound over every audited step of the GPU suite on an MI355X (the direct kernel tests and the model-level tests that
# carry the audit), with the tensor and step it came from:
#   Adam p   0.488  base_net.level4.4.conv_1x1_exp.bn.weight[492], step 3 of the train loop (loop_32x48)
#   Adam m   0.148  the 4097-element tensor of the input set below, element 1912, step 2 (betas (0.9, 0.999), wd 0)
#   Adam v   0.159  base_net.level4.5.conv_1x1_exp.conv.weight[51128], step 2 (gradient sinks, 32x48)
#   SGD p    0.500  the 1000-element tensor of test_gpu_optim's FlatSGD case, element 688, step 3
#   SGD buf  0.294  base_net.level4.3.conv_1x1_exp.conv.weight[45905], iteration 4 of the graphed supervised step
# and mspl_adam_step on raw buffers, steps 1 to 100000: p 0.377, m 0.110, v 0.137.
#
# Worst error / bound measured for torch's own float32 CPU optimizers on the input set below (tests/test_optim_shadow.py prints
# them): Adam p 0.469, m 0.087, v 0.113; SGD p 0.500, buf 0.261.  p sits at one half because tol_p starts with a whole ulp32(p')
# and a correctly rounded result is within half of one.
#
# Before this file existed the Adam kernel formed 1 - beta2 and 1 - beta2^step from the float32 beta: a float32 evaluation of that
# arithmetic on the same inputs is 4.5x over tol_v at every step and 1.4x over tol_p (betas (0.9, 0.999); (float)0.999 is 1.3e-8
# too large and 1.f - beta2 makes 1.3e-5 of v out of it).  The entry point now takes the betas as doubles and forms both on the
# host in double, as torch.optim.Adam does.


def ulp32(x):
    """Spacing of float32 at |x| (float64 array in, float64 out)."""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def _f64(*arrays):
    return [np.asarray(a, dtype=np.float64) for a in arrays]


def _cond(g, wdp, gi):
    """Conditioning of gi = g + wd*p: (|g| + |wd*p|) / |gi|, 0 where gi == 0."""
    num = np.abs(g) + np.abs(wdp)
    return np.divide(num, np.abs(gi), out=np.zeros_like(num), where=gi != 0)


def adam_step64(p, g, m, v, lr, betas, eps, wd, step):
    """torch.optim.Adam (L2 weight decay, no amsgrad) in float64 on float32 inputs.  Returns (p', m', v', u, cond, gi)."""
    p, g, m, v = _f64(p, g, m, v)
    b1, b2 = float(betas[0]), float(betas[1])
    wdp = float(wd) * p
    gi = g + wdp
    m1 = b1 * m + (1.0 - b1) * gi
    v1 = b2 * v + (1.0 - b2) * gi * gi
    u = (m1 / (1.0 - b1 ** step)) / (np.sqrt(v1) / np.sqrt(1.0 - b2 ** step) + float(eps))
    return p - float(lr) * u, m1, v1, u, _cond(g, wdp, gi), gi


def adam_bounds(p, g, m, v, lr, betas, eps, wd, step):
    """(p', m', v', tol_p, tol_m, tol_v): the float64 step and the forward-error bounds of a float32 evaluation of it.
    The 4 in tol_p covers (1-b1)/sqrt(1-b2) ~ 3.2, the largest |du/dgi * gi| when gi dwarfs the history."""
    p1, m1, v1, u, cond, gi = adam_step64(p, g, m, v, lr, betas, eps, wd, step)
    b1 = float(betas[0])
    tol_p = ulp32(p1) + MARGIN_ADAM * EPS32 * float(lr) * (4.0 + np.abs(u)) * (1.0 + cond)
    tol_m = MARGIN_ADAM * EPS32 * (np.abs(b1 * np.asarray(m, dtype=np.float64)) + (1.0 - b1) * np.abs(gi) * (1.0 + cond))
    tol_v = MARGIN_ADAM * EPS32 * v1 * (1.0 + 2.0 * cond)
    return p1, m1, v1, tol_p, tol_m, tol_v


def sgd_step64(p, g, buf, lr, momentum, wd, first):
    """torch.optim.SGD (dampening 0, no Nesterov; the buffer equals gi on the first step) in float64 on float32 inputs.
    Returns (p', buf', gi, cond).  With momentum == 0 torch keeps no buffer: buf' is the gi the update used."""
    p, g, buf = _f64(p, g, buf)
    wdp = float(wd) * p
    gi = g + wdp
    b = gi if (first or float(momentum) == 0.0) else float(momentum) * buf + gi
    return p - float(lr) * b, b, gi, _cond(g, wdp, gi)


def sgd_bounds(p, g, buf, lr, momentum, wd, first):
    """(p', buf', tol_p, tol_buf)."""
    p1, b1, gi, cond = sgd_step64(p, g, buf, lr, momentum, wd, first)
    carried = 0.0 if (first or float(momentum) == 0.0) else np.abs(float(momentum) * np.asarray(buf, dtype=np.float64))
    tol_buf = MARGIN_SGD * EPS32 * (carried + np.abs(gi) * (1.0 + cond))
    return p1, b1, ulp32(p1) + float(lr) * tol_buf, tol_buf


# ---- the input set shared by tests/test_optim_shadow.py (CPU) and tests/test_gpu_optim.py (GPU)

SIZES = (1, 3, 255, 256, 257, 1000, 4097)
GRAD_SCALES = (1e-3, 1.0, 1e-8, 1e-5, 10.0, 1e-8, 1.0)     # the 1e-8 tensors are where the place of eps decides the result
STEPS = 6
LRS = (1e-2, 1e-2, 5e-3, 2e-3, 2e-3, 2e-3)                  # changed before steps 3 and 4, as adjust_learning_rate does
NOGRAD_AT = 3                                               # a gradient-less parameter sits in front of SIZES[3]
NOGRAD_SIZE = 37


def input_set(seed=6):
    """(params, grads): params = float32 arrays of SIZES, N(0,1); grads[s][i] = the fresh gradient of parameter i at step s (0-based),
    N(0,1) * GRAD_SCALES[i] with a few exact zeros (tensors of three elements and more; the positions move with the step, and the
    last element is zero at every step so that one element's gradient is the weight decay alone).  The seed is one at which the
    weakest mutation of tests/test_optim_shadow.py ('eps before the bias division' at beta2 = 0.99, which moves the one-element
    tensor by lr * 9e-8 / |g| against a bound of lr * 9.5e-6) clears 10x on every tensor: that needs |g| < 1e-3 there, and the
    draw of about every tenth seed has it."""
    rng = np.random.default_rng(1234 + seed)
    params = [rng.standard_normal(n).astype(np.float32) for n in SIZES]
    grads = []
    for s in range(STEPS):
        gs = []
        for n, sc in zip(SIZES, GRAD_SCALES):
            g = (rng.standard_normal(n) * sc).astype(np.float32)
            if n >= 3:
                g[(s * 7) % (n - 1)] = 0.0
                g[n - 1] = 0.0
            gs.append(g)
        grads.append(gs)
    return params, grads


# ---- the audit

def _named(model):
    """[(name, parameter)] of a module, a dict or a list of pairs."""
    if hasattr(model, 'named_parameters'):
        return list(model.named_parameters())
    return list(model.items()) if isinstance(model, dict) else list(model)


class _Record(object):
    __slots__ = ('opt', 'kind', 'step', 'lrs', 'hyper', 'pre', 'post', 'tag')


class StepAudit(object):
    """with StepAudit(model, ...) as audit: ...steps...; audit.check(model).

    Wraps `training.FlatAdam.step` and `supervised.FlatSGD.step` class-wide (through a pytest.MonkeyPatch it owns).  Around every
    step it keeps device clones of the flat buffers and the host hyper-parameters the kernel is about to receive; clones only -- no
    copy to the host and no synchronisation inside the wrapper.  Models given to the constructor have their parameters and
    floating-point buffers cloned on entry: `check` needs them for the tensors no optimizer owns."""

    def __init__(self, *models):
        self.models = list(models)
        self.records = []
        self.worst = {}          # quantity -> (error / bound, step, tensor name, flat index)
        self.tag = None          # copied into every record made while it is set (a test marks phases with it)
        self._entry = {}

    def watch(self, model):
        """Clone the parameters and floating-point buffers of a module (or the tensors of a {name: parameter} dict) now -- what
        __enter__ does for the constructor's models.  `check` takes the same object."""
        import torch
        snap = {}
        for n, t in _named(model) + (list(model.named_buffers()) if hasattr(model, 'named_buffers') else []):
            if torch.is_floating_point(t):
                snap[n] = t.detach().clone()
        self._entry[id(model)] = snap
        return model

    def __enter__(self):
        import pytest
        from mspl_amd import supervised, training
        self._mp = pytest.MonkeyPatch()
        audit = self
        adam_step, sgd_step = training.FlatAdam.step, supervised.FlatSGD.step

        def adam(opt):
            r = audit._open(opt, 'adam', opt.step_count + 1, [float(opt.lr)],
                            (tuple(float(b) for b in opt.betas), float(opt.eps), float(opt.weight_decay)),
                            (opt.flat_p, opt.flat_g, opt.m, opt.v))
            out = adam_step(opt)
            r.post = tuple(t.clone() for t in (opt.flat_p, opt.m, opt.v))
            return out

        def sgd(opt):
            r = audit._open(opt, 'sgd', opt.step_count + 1, [float(g['lr']) for g in opt.param_groups],
                            [(g['_lo'], g['_hi'], float(g['momentum']), float(g['weight_decay'])) for g in opt.param_groups],
                            (opt.flat_p, opt.flat_g, opt.buf))
            out = sgd_step(opt)
            r.post = tuple(t.clone() for t in (opt.flat_p, opt.buf))
            return out

        self._mp.setattr(training.FlatAdam, 'step', adam)
        self._mp.setattr(supervised.FlatSGD, 'step', sgd)
        for m in self.models:
            self.watch(m)
        return self

    def __exit__(self, *exc):
        self._mp.undo()
        return False

    def _open(self, opt, kind, step, lrs, hyper, tensors):
        r = _Record()
        r.opt, r.kind, r.step, r.lrs, r.hyper, r.tag = opt, kind, step, lrs, hyper, self.tag
        r.pre = tuple(t.clone() for t in tensors)
        r.post = None
        self.records.append(r)
        return r

    @property
    def steps(self):
        """[(step count the kernel received, [lr per group])] in the order the steps ran."""
        return [(r.step, list(r.lrs)) for r in self.records]

    def records_of(self, model):
        ids = set(id(p) for _, p in _named(model))
        return [r for r in self.records if id(r.opt.params[0]) in ids]

    # -- host side

    def _note(self, what, ratio, step, layout, label):
        i = int(np.argmax(ratio))
        val = float(ratio[i])
        k = int(np.searchsorted(layout['offsets'], i, side='right')) - 1
        name = layout['names'][k]
        if val > self.worst.get(what, (-1.0,))[0]:
            self.worst[what] = (val, step, name, i - int(layout['offsets'][k]))
        return val, name, i, i - int(layout['offsets'][k])

    def _compare(self, what, got, want, tol, step, layout, label):
        err = np.abs(got.astype(np.float64) - want)
        bad = ~(err <= tol)                               # (catches NaN too)
        ratio = np.divide(err, tol, out=np.where(err > 0, np.inf, 0.0), where=tol > 0)
        ratio = np.where(np.isnan(ratio), np.inf, ratio)
        val, name, i, j = self._note(what, ratio, step, layout, label)
        assert not bad.any(), ('%s: %s of %s at step %d: element %d is %.9g, float64 says %.9g: error %.3g > bound %.3g (%.3g x), '
                               '%d elements out of bound' % (label, what, name, step, j, got[i], want[i], err[i], tol[i], val,
                                                             int(bad.sum())))

    def check(self, model, frozen_buffers=True, label=''):
        """Every recorded step of the optimizers that own parameters of `model` (a module, or {name: parameter}), every element.
        frozen_buffers=False for a model in train() mode (its BatchNorm statistics move)."""
        import torch
        named = _named(model)
        names = dict((id(p), n) for n, p in named)
        recs = self.records_of(model)
        assert recs, '%s: no optimizer step of this model was recorded' % label
        in_bucket = set()
        for r in recs:
            opt = r.opt
            assert r.post is not None, 'the step raised'
            offsets = np.asarray(opt.bucket.offsets, dtype=np.int64)
            sizes = np.asarray([p.numel() for p in opt.params], dtype=np.int64)
            layout = {'offsets': offsets, 'names': [names[id(p)] for p in opt.params]}
            in_bucket.update(id(p) for p in opt.params)
            pad = np.ones(opt.flat_p.numel(), dtype=bool)
            for o, k in zip(offsets, sizes):
                pad[o:o + k] = False
            pre = [t.cpu().numpy() for t in r.pre]
            post = [t.cpu().numpy() for t in r.post]
            tag = '%s step %d' % (label, r.step)
            for what, a in zip(('p', 'g') + (('m', 'v') if r.kind == 'adam' else ('buf',)), pre):
                assert not a[pad].any(), '%s: alignment padding of flat %s is not zero before the step' % (tag, what)
            for what, a in zip(('p', 'm', 'v') if r.kind == 'adam' else ('p', 'buf'), post):
                assert not a[pad].any(), '%s: alignment padding of flat %s is not zero after the step' % (tag, what)
            if r.kind == 'adam':
                betas, eps, wd = r.hyper
                p1, m1, v1, tol_p, tol_m, tol_v = adam_bounds(pre[0], pre[1], pre[2], pre[3], r.lrs[0], betas, eps, wd, r.step)
                self._compare('adam p', post[0], p1, tol_p, r.step, layout, label)
                self._compare('adam m', post[1], m1, tol_m, r.step, layout, label)
                self._compare('adam v', post[2], v1, tol_v, r.step, layout, label)
            else:
                covered = np.zeros(opt.flat_p.numel(), dtype=bool)
                for lr, (lo, hi, mu, wd) in zip(r.lrs, r.hyper):
                    if hi <= lo:
                        continue
                    assert not covered[lo:hi].any(), '%s: two groups share flat elements' % tag
                    covered[lo:hi] = True
                    k0 = int(np.searchsorted(offsets, lo, side='left'))
                    k1 = int(np.searchsorted(offsets, hi, side='left'))
                    assert offsets[k0] == lo and k1 > k0, '%s: a group span does not start at a parameter' % tag
                    sub = {'offsets': offsets[k0:k1] - lo, 'names': layout['names'][k0:k1]}
                    p1, b1, tol_p, tol_b = sgd_bounds(pre[0][lo:hi], pre[1][lo:hi], pre[2][lo:hi], lr, mu, wd, r.step == 1)
                    self._compare('sgd p', post[0][lo:hi], p1, tol_p, r.step, sub, label)
                    if mu == 0.0:      # torch keeps no buffer without momentum; the kernel leaves its slice alone
                        assert np.array_equal(post[1][lo:hi].view(np.uint32), pre[2][lo:hi].view(np.uint32)), \
                            '%s: momentum 0 and the buffer of a group changed' % tag
                    else:
                        self._compare('sgd buf', post[1][lo:hi], b1, tol_b, r.step, sub, label)
                assert covered[~pad].all(), '%s: a parameter of the bucket belongs to no group' % tag
        snap = self._entry.get(id(model))
        assert snap is not None, 'StepAudit: give the model to the constructor (or watch() it) before its first step'
        for n, p in named:
            if id(p) not in in_bucket and n in snap:
                assert torch.equal(p.detach().view(torch.int32), snap[n].view(torch.int32)), \
                    '%s: %s is in no optimizer bucket and changed' % (label, n)
        if frozen_buffers and hasattr(model, 'named_buffers'):
            for n, b in model.named_buffers():
                if torch.is_floating_point(b):
                    assert torch.equal(b.view(torch.int32), snap[n].view(torch.int32)), '%s: buffer %s of a frozen model changed' % (label, n)
        self._log(label, len(recs))
        return self.worst

    def _log(self, label, n):
        line = '%s: %d steps; worst error/bound ' % (label or 'audit', n) + ', '.join(
            '%s %.3f (%s[%d], step %d)' % (k, v[0], v[2], v[3], v[1]) for k, v in sorted(self.worst.items()))
        print(line)
        path = os.environ.get('MSPL_AUDIT_LOG')
        if path:
            with open(path, 'a') as f:
                f.write(line + '\n')
