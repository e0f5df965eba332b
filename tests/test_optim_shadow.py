"""The yardstick of tests/optim_shadow.py pinned on the CPU: its float64 statements equal torch's optimizers in float64, torch's own
float32 optimizers pass its bounds on every element, and every mutation of the statement a kernel could plausibly carry exceeds
the bound ten times over on every tensor of the input set -- power shown without mutating a kernel."""
import numpy as np
import pytest
import torch

from tests import optim_shadow as S

EPS, WD = 1e-8, 5e-4
BETAS = [(0.9, 0.999), (0.8, 0.99)]
SGD_GROUP = (0, 0, 0, 1, 1, 2, 2)               # parameter -> learning-rate group
SGD_LRS = [(0.05, 0.5, 0.1)] * 2 + [(0.02, 0.5, 0.1)] * 4       # per step, per group
SGD_MU, SGD_WD = 0.9, 5e-4


def _torch_run(opt_cls, dtype, params, grads, lrs, **kw):
    """States before and after each of the STEPS steps of a torch optimizer in `dtype`: [(p, state tensors...)] per parameter."""
    ps = [torch.nn.Parameter(torch.from_numpy(p.copy()).to(dtype)) for p in params]
    opt = opt_cls(ps, lr=lrs[0], **kw)
    out = []
    for s in range(S.STEPS):
        opt.param_groups[0]['lr'] = lrs[s]
        for p, g in zip(ps, grads[s]):
            p.grad = torch.from_numpy(g.copy()).to(dtype)
        opt.step()
        out.append([(p.detach().clone().numpy(), dict((k, v.clone().numpy()) for k, v in opt.state[p].items() if torch.is_tensor(v) and v.dim()))
                    for p in ps])
    return out


def _rel(a, b):
    """Relative to the tensor's largest element: torch forms m' as lerp(m, gi, 1-b1), the statement as b1*m + (1-b1)*gi, and where the
    two terms cancel the float64 results differ by 1e-16 of the TERMS, not of the (small) sum."""
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-300))


@pytest.mark.parametrize('wd', [0.0, WD])
@pytest.mark.parametrize('betas', BETAS)
def test_adam_statement_equals_torch_float64(betas, wd):
    params, grads = S.input_set()
    ref = _torch_run(torch.optim.Adam, torch.float64, params, grads, S.LRS, betas=betas, eps=EPS, weight_decay=wd)
    for i in range(len(params)):
        p, m, v = [a.astype(np.float64) for a in (params[i], np.zeros_like(params[i]), np.zeros_like(params[i]))]
        for s in range(S.STEPS):
            p, m, v = S.adam_step64(p, grads[s][i], m, v, S.LRS[s], betas, EPS, wd, s + 1)[:3]
            want = ref[s][i]
            assert _rel(p, want[0]) <= 1e-14 and _rel(m, want[1]['exp_avg']) <= 1e-14 and _rel(v, want[1]['exp_avg_sq']) <= 1e-14, (i, s)


@pytest.mark.parametrize('wd', [0.0, SGD_WD])
def test_sgd_statement_equals_torch_float64(wd):
    params, grads = S.input_set()
    lrs = [l[0] for l in SGD_LRS]
    ref = _torch_run(torch.optim.SGD, torch.float64, params, grads, lrs, momentum=SGD_MU, weight_decay=wd)
    for i in range(len(params)):
        p, buf = params[i].astype(np.float64), np.full(params[i].shape, 7.0)      # (a first step ignores what the buffer holds)
        for s in range(S.STEPS):
            p, buf = S.sgd_step64(p, grads[s][i], buf, lrs[s], SGD_MU, wd, s == 0)[:2]
            assert _rel(p, ref[s][i][0]) <= 1e-14 and _rel(buf, ref[s][i][1]['momentum_buffer']) <= 1e-14, (i, s)


def _ratio(got, want, tol):
    err = np.abs(got.astype(np.float64) - want)
    return float(np.max(np.divide(err, tol, out=np.where(err > 0, np.inf, 0.0), where=tol > 0)))


def test_float32_torch_optimizers_pass_the_bounds(capsys):
    """torch's float32 CPU Adam and SGD, stepped ONCE from each float32 pre-step state of a six-step run, against the float64
    statement at that state: every element within the derived bound.  (The coupled six-step float32-against-float64 comparison the
    per-step form replaces drifts to 1.5e-3 * lr.)"""
    params, grads = S.input_set()
    worst = {'adam p': 0.0, 'adam m': 0.0, 'adam v': 0.0, 'sgd p': 0.0, 'sgd buf': 0.0}
    for betas in BETAS:
        for wd in (0.0, WD):
            run = _torch_run(torch.optim.Adam, torch.float32, params, grads, S.LRS, betas=betas, eps=EPS, weight_decay=wd)
            for i, p0 in enumerate(params):
                pre = (p0, np.zeros_like(p0), np.zeros_like(p0))
                for s in range(S.STEPS):
                    p1, m1, v1, tp, tm, tv = S.adam_bounds(pre[0], grads[s][i], pre[1], pre[2], S.LRS[s], betas, EPS, wd, s + 1)
                    got = run[s][i]
                    for k, r in (('adam p', _ratio(got[0], p1, tp)), ('adam m', _ratio(got[1]['exp_avg'], m1, tm)),
                                 ('adam v', _ratio(got[1]['exp_avg_sq'], v1, tv))):
                        worst[k] = max(worst[k], r)
                        assert r <= 1.0, (k, betas, wd, i, s, r)
                    pre = (got[0], got[1]['exp_avg'], got[1]['exp_avg_sq'])
    lrs = [l[0] for l in SGD_LRS]
    for wd in (0.0, SGD_WD):
        run = _torch_run(torch.optim.SGD, torch.float32, params, grads, lrs, momentum=SGD_MU, weight_decay=wd)
        for i, p0 in enumerate(params):
            pre = (p0, np.zeros_like(p0))
            for s in range(S.STEPS):
                p1, b1, tp, tb = S.sgd_bounds(pre[0], grads[s][i], pre[1], lrs[s], SGD_MU, wd, s == 0)
                got = run[s][i]
                for k, r in (('sgd p', _ratio(got[0], p1, tp)), ('sgd buf', _ratio(got[1]['momentum_buffer'], b1, tb))):
                    worst[k] = max(worst[k], r)
                    assert r <= 1.0, (k, wd, i, s, r)
                pre = (got[0], got[1]['momentum_buffer'])
    with capsys.disabled():
        print('\nfloat32 torch optimizers, worst error / bound: ' + ', '.join('%s %.3f' % kv for kv in sorted(worst.items())))


# ---- power: mutations of the float64 statement

def _adam_mutant(name):
    def step(p, g, m, v, lr, prev_lr, betas, eps, wd, t):
        b1, b2 = betas
        if name == 'betas swapped':
            b1, b2 = b2, b1
        if name == 'm not carried over':
            m = np.zeros_like(m)
        if name == 'v not carried over':
            v = np.zeros_like(v)
        gi = g if name == 'wd*p dropped' else g + wd * p
        m1 = b1 * m + (1 - b1) * gi
        v1 = b2 * v + (1 - b2) * gi * gi
        tb = t - 1 if name == 'bias correction t-1' else t
        with np.errstate(divide='ignore', invalid='ignore'):
            if name == 'eps inside the square root':
                den = np.sqrt(v1 / (1 - b2 ** tb) + eps)
            elif name == 'eps before the bias division':
                den = (np.sqrt(v1) + eps) / np.sqrt(1 - b2 ** tb)
            else:
                den = np.sqrt(v1) / np.sqrt(1 - b2 ** tb) + eps
            u = (m1 / (1 - b1 ** tb)) / den
        return p - (prev_lr if name == 'lr of the previous step' else lr) * u
    return step


ADAM_MUTANTS = ['betas swapped', 'bias correction t-1', 'eps inside the square root', 'eps before the bias division', 'wd*p dropped',
                'm not carried over', 'v not carried over', 'lr of the previous step']
SGD_MUTANTS = ['first ignored', 'wd after the momentum', "the other group's lr"]


def _excess(mutant_p, p1, tol):
    """Largest |mutant - statement| / bound over a tensor; a non-finite mutant counts as infinitely wrong."""
    d = np.abs(mutant_p - p1)
    d = np.where(np.isfinite(d), d, np.inf)
    return float(np.max(d / tol))


@pytest.mark.parametrize('betas', BETAS)
def test_every_adam_mutation_exceeds_the_bound_on_every_tensor(betas, capsys):
    """Each wrong Adam, run on the true trajectory's pre-step state, is at least 10x over tol_p on some element of EVERY tensor by
    step 3 (weight decay 5e-4: the setting of the product, and the one where a lost wd*p can show)."""
    params, grads = S.input_set()
    table = {}
    for i, p0 in enumerate(params):
        p, m, v = [a.astype(np.float64) for a in (p0, np.zeros_like(p0), np.zeros_like(p0))]
        for s in range(3):
            g = grads[s][i].astype(np.float64)
            p1, m1, v1, tol_p = S.adam_bounds(p, g, m, v, S.LRS[s], betas, EPS, WD, s + 1)[:4]
            for name in ADAM_MUTANTS:
                q = _adam_mutant(name)(p, g, m, v, S.LRS[s], S.LRS[s - 1] if s else S.LRS[0], betas, EPS, WD, s + 1)
                table[name, i] = max(table.get((name, i), 0.0), _excess(q, p1, tol_p))
            # (the next state is the float32 one a kernel would hold)
            p, m, v = [a.astype(np.float32).astype(np.float64) for a in (p1, m1, v1)]
    _report(capsys, 'Adam betas=%s' % (betas,), ADAM_MUTANTS, table)


def test_every_sgd_mutation_exceeds_the_bound_on_every_tensor(capsys):
    """Three learning-rate groups, momentum 0.9; the buffer holds leftovers when the first step arrives (a first step must not read
    it).  Each wrong SGD runs its OWN trajectory: 'wd after the momentum' gives the right p from a right buffer and only stores a
    wrong one, so it shows in p one step later."""
    params, grads = S.input_set()
    rng = np.random.default_rng(5)
    table = {}

    def mutant(name, p, g, buf, s, gr):
        lr = SGD_LRS[s][gr]
        if name == 'first ignored':
            b = SGD_MU * buf + g + SGD_WD * p
        elif name == 'wd after the momentum':
            b = g if s == 0 else SGD_MU * buf + g
            return p - lr * (b + SGD_WD * p), b
        else:
            b = (g + SGD_WD * p) if s == 0 else SGD_MU * buf + g + SGD_WD * p
            lr = SGD_LRS[s][(gr + 1) % 3]
        return p - lr * b, b

    for i, p0 in enumerate(params):
        junk = rng.standard_normal(p0.shape)
        p, buf = p0.astype(np.float64), junk
        state = dict((name, (p, junk)) for name in SGD_MUTANTS)
        gr = SGD_GROUP[i]
        for s in range(3):
            g = grads[s][i].astype(np.float64)
            p1, b1, tol_p, _ = S.sgd_bounds(p, g, buf, SGD_LRS[s][gr], SGD_MU, SGD_WD, s == 0)
            for name in SGD_MUTANTS:
                state[name] = mutant(name, state[name][0], g, state[name][1], s, gr)
                table[name, i] = max(table.get((name, i), 0.0), _excess(state[name][0], p1, tol_p))
            p, buf = p1, b1
    _report(capsys, 'SGD', SGD_MUTANTS, table)


def _report(capsys, title, mutants, table):
    with capsys.disabled():
        print('\n%s: largest |mutant - statement| / tol_p per tensor (sizes %s), steps 1-3' % (title, list(S.SIZES)))
        for name in mutants:
            print('  %-30s %s' % (name, ' '.join('%9.3g' % table[name, i] for i in range(len(S.SIZES)))))
    weak = [(name, S.SIZES[i], r) for (name, i), r in sorted(table.items()) if not r >= 10.0]
    assert not weak, 'mutations under 10x the bound: %s' % weak


def test_wd_after_momentum_mutant_is_not_the_statement():
    """(guards the mutant table itself: at step 1 'wd after the momentum' IS the statement, from step 2 on it is not)"""
    p, g, buf = np.float32([1.0]), np.float32([0.5]), np.float32([0.25])
    p1, b1 = S.sgd_step64(p, g, buf, 0.1, 0.9, 0.01, False)[:2]
    assert abs(b1[0] - (0.9 * 0.25 + 0.5 + 0.01)) < 1e-15 and abs(p1[0] - (1.0 - 0.1 * b1[0])) < 1e-15
    first = S.sgd_step64(p, g, buf, 0.1, 0.9, 0.01, True)[1]
    assert abs(first[0] - 0.51) < 1e-15
