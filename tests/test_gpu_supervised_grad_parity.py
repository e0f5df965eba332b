"""Every gradient of the supervised iteration (supervised.train_seg_ue_step / GraphedSupervisedStep: batch-statistics BatchNorm,
CrossEntropy on main + 0.5 * aux, flooding, SGD groups), tensor by tensor, against the float64 oracle (oracle.train.supervised_step)
evaluated at the path's OWN pre-step state -- parameters AND running statistics -- together with the loss, the BatchNorm buffers
after the step and, after a first step, the parameters SGD wrote.  tests/test_gpu_grad_parity.py does the same for the uest step.

The cases cover what the norm-only golden check and the GPU-vs-GPU comparisons of tests/test_supervised.py cannot see: both
BatchNorm forms (one launch per node on small planes, statistics + apply launches above 40 960 values per channel), the fused
EESP / pyramid nodes on large planes, graph replays one by one, the benchmark's configuration (C=13, ignore_idx=255, class weights),
the flooding branch loss < b, and the RGB-D path with its third SGD group.

Batch duplication: a batch of k permuted copies of four images has the loss and the gradients of the four alone (a weighted
mean over pixels; batch statistics of a multiset and of its k-fold copy agree), so one batch-4 oracle run serves a batch-16 or
batch-64 GPU case; only running_var differs, by the unbiased factor n / (n - 1), which the test restates for the larger count.

Conditioning: as in tests/test_gpu_grad_parity.py -- the oracle at each case's seeded state asserts that no activation input of a
map of <= 256 pixels per plane lies within KINK_REL * rms(tensor) of zero; the seeds below were chosen on the CPU to pass, and so
that the float32 oracle itself stays within 6e-5 of the float64 one (a seed can pass the first and miss the second by 1e-2).

Parameters in no SGD group (auxiliary decoder, fusion gates, ...) are never zeroed by the loop, here as in the reference: their
.grad accumulates over iterations.  The tests zero those in place before every step after the first to read one step's gradient."""
import argparse

import pytest
import torch

from oracle import train as otrain
from tests.gradcheck import (ActivationRecorder, BatchNormRecorder, assert_grads_match, running_var_for_copies,
                             supervised_groups)
from tests.synth import synth_input, synth_labels, synth_state_dict

pytestmark = pytest.mark.gpu
DEV = 'cuda'
KINK_REL = 1e-6
LR, LR_MULT, MOMENTUM, WEIGHT_DECAY, FLOOD = 0.009, 10.0, 0.9, 4e-5, 0.015        # train_seg_ue_step's defaults
# Tolerances: per-tensor errors against the float64 oracle, (relative norm error, largest element error / largest element of the
# tensor), at most 4x the worst observed on the MI355X over every case, form and step below and over two runs (the float atomics
# land in a different order each run).  For scale: the float32 ORACLE against float64 gives 0.7e-5 .. 5.9e-5 on the small cases.
# small cases -- observed worst: rel 5.2e-5, element 6.7e-5 (both base_net.level2_0.inp_reinf.0.bn.weight, 2x48x80 eager, where the
# float32 oracle has 5.9e-5 / 7.6e-5 on the same tensor); the smallest case in every form: 2.7e-5 / 3.4e-5
SUP_TAU_REL, SUP_TAU_EL = 2e-4, 2.5e-4
# the small cases at a state a GPU step wrote (steps after the first, graph replays), which nobody chose for its conditioning --
# observed worst over three runs: rel 1.3e-2 (base_net.level4_0.inp_reinf.0.act.weight, 4x32x48 third step, near-kinks on a 2 x 3
# and an 8 x 12 map), element 6.8e-2 (base_net.level4_0.inp_reinf.1.bn.bias, 4x32x48 second replay, near-kink on a 2 x 3 map);
# also 1.1e-2 / 1.9e-2 on bu_dec_l4.projection_layer.cbr.1.bias with no near-kink on a map of <= 256 pixels (an input of that
# block's 16 x 24 map took the other slope).  In other runs the very same steps stay within 2.7e-5 / 4.2e-5: the outcome is
# bimodal, a PReLU sign on a small map or none (tests/test_supervised.py describes the same for two GPU runs), and with 24 values
# per channel at level 4 one sign is per cent of a channel's sums.  The constant is for the first mode.
STEPPED_TAU_REL, STEPPED_TAU_EL = 5e-2, 0.25
# the batch-16 / batch-64 cases -- observed worst: rel 2.5e-2 (base_net.level2_0.inp_reinf.0.bn.bias, 192x256 second replay), element
# 8.4e-2 (base_net.level4.6.conv_1x1_exp.bn.bias, benchmark configuration).  These are NOT rounding of the longer sums: level 4 holds
# 4 x 512 x 192 (540) activation inputs per block there, a handful of them within float32 rounding of zero whatever the seed (the
# near-kinks each message lists), and the float32 oracle itself is off by 2e-3 .. 2e-2 / 1.3e-2 .. 1.9e-2 at these states; batch 16
# and batch 64 land on the same figures (8.25e-3 / 5.92e-2, the same PReLU signs).  So these cases see a missing, doubled or
# misplaced term, not a small one; the small cases and the op / block tests hold the large-plane kernels to rounding.
FULL_TAU_REL, FULL_TAU_EL = 0.1, 0.3
# the RGB-D case -- observed: rel 4.4e-4, element 7.2e-4 (both bu_dec_l4.merge_layer.0.br.0.bias), 12x the float32 oracle's 3.6e-5 /
# 4.1e-5 and chased down: with the depth encoder the step has twice the activation inputs, and the closest one to zero lies at
# 1.7e-6 rms (of 31 seeds tried on the CPU the best has 3.9e-6) -- here at 3.6e-6 rms on the 16 x 24 input of that very
# bu_dec_l4.merge_layer.0, a map the conditioning rule (<= 256 pixels) does not look at, and within the float32 forward's error.
# Every other tensor of the case is inside the small-case constants' scale.
RGBD_TAU_REL, RGBD_TAU_EL = 1.8e-3, 2.9e-3
# running_mean / running_var after the step, per buffer -- observed worst: rel 6.2e-7 (depth_base_net.level4.6.br_after_cat.bn
# .running_mean), element 1.4e-6 (depth_base_net.level4.6.proj_1x1.bn.running_var), both RGB-D, where these BatchNorms run twice;
# elsewhere 2.6e-7 / 3.9e-7
BUF_TAU_REL, BUF_TAU_EL = 2.5e-6, 5e-6
# the loss, relative -- observed worst 1.3e-6 (192x256 at batch 64; small cases 3.4e-7)
LOSS_TAU = 5e-6
PERM16 = [0, 1, 2, 3, 3, 2, 1, 0, 1, 3, 0, 2, 2, 0, 3, 1]                         # (tests/test_gpu_grad_parity.py)
PERMS = {16: PERM16, 64: [(p + r) % 4 for r in range(4) for p in PERM16]}


class Case:
    def __init__(self, shape, seed, classes=5, dataset='greenhouse', ignore_idx=4, weights=False, void_band=None, depth=False):
        self.shape, self.seed, self.classes, self.dataset, self.ignore_idx = shape, seed, classes, dataset, ignore_idx
        self.weights, self.void_band, self.depth = weights, void_band, depth

    def model(self):
        from mspl_amd import models
        a = argparse.Namespace(s=2.0, channels=3, num_classes=1000)
        m = models.ESPDNetwithUncertaintyEstimation(a, classes=self.classes, dataset=self.dataset, trainable_fusion=True,
                                                    fix_pyr_plane_proj=True)
        m.load_state_dict(synth_state_dict(m.state_dict(), self.seed))
        return m

    def class_weights(self):
        return torch.linspace(0.5, 2.0, self.classes) if self.weights else None

    def data(self):
        """(images, labels, depth or None) on the CPU."""
        n, _, h, w = self.shape
        x, y = synth_input(self.shape, self.seed), synth_labels((n, h, w), self.classes, self.seed)
        if self.void_band is not None:
            y[:, self.void_band[0]:self.void_band[1], :] = self.ignore_idx
        return x, y, (synth_input((n, 1, h, w), self.seed + 100) if self.depth else None)

    def criterion(self):
        from mspl_amd import losses
        return losses.SegmentationLoss(n_classes=self.classes, device=DEV, ignore_idx=self.ignore_idx, class_weights=self.class_weights())


# seeds of weights and inputs: chosen for their conditioning in train() mode (the uest file's seeds do not carry over)
CASES = {'4x32x48': Case((4, 3, 32, 48), 8),           # the smallest: level 4 at 2x3 pixels
         '2x64x96': Case((2, 3, 64, 96), 10),          # streaming pyramid kernels, matrix-core weight gradients
         '2x48x80': Case((2, 3, 48, 80), 1),           # odd level-4 sides (3x5)
         '4x64x64': Case((4, 3, 64, 64), 51),          # the shape of the golden step
         'rgbd': Case((2, 3, 32, 48), 2, depth=True),
         # levels 1 and 2 above 40 960 values per channel at batch 16, levels 3 and 4 below; at batch 64 level 3 (the stride-1 EESP
         # blocks, the only BatchNorm nodes with a residual) is above it too
         '192x256': Case((4, 3, 192, 256), 2),
         # bench.py's supervised_step: 16 x 3 x 288 x 480, C=13, camvid, ignore_idx=255; here with void labels and class weights
         'bench': Case((4, 3, 288, 480), 1, classes=13, dataset='camvid', ignore_idx=255, weights=True, void_band=(100, 124))}
SMALLEST = '4x32x48'


def _snapshot(m):
    return {k: (v.detach().to('cpu', torch.float64).clone() if v.is_floating_point() else v.detach().cpu().clone())
            for k, v in m.state_dict().items()}


def _names(m):
    return [n for n, _ in m.named_parameters()]


def _oracle(case, sd64, names, b=FLOOD):
    """The float64 oracle at the state sd64: dict(loss, grads, new, after, kinks, count = (values per channel, calls) of every BatchNorm
    that ran, lr = learning rate by parameter name)."""
    x, y, xd = case.data()
    cw = case.class_weights()
    groups = supervised_groups(names, LR, LR_MULT, case.depth)
    with pytest.MonkeyPatch.context() as mp:
        rec, bnrec = ActivationRecorder(mp), BatchNormRecorder(mp)
        loss, g, new, after = otrain.supervised_step(sd64, groups, x.double(), y, None if cw is None else cw.double(), case.ignore_idx,
                                                     MOMENTUM, WEIGHT_DECAY, b, None if xd is None else xd.double(),
                                                     dense_fuse=False, trainable_fusion=True)
    return {'loss': float(loss), 'grads': g, 'new': new, 'after': after, 'kinks': rec.near_kinks(rel=KINK_REL),
            'count': bnrec.per_channel(after), 'lr': {n: lr for ns, lr in groups for n in ns}}


def _compare(m, loss, ref, before, what, conditioned, tau, batch=None, n_expected=340, check_new=False):
    """conditioned: the state is the seeded one, whose conditioning the case asserts; a state written by a GPU step is not ours to
    choose, so there the near-kinks are only named in a failure message."""
    what = '%s (near-kinks %s)' % (what, ref['kinks'][:4])
    if conditioned:
        assert not ref['kinks'], '%s: activation inputs within %g rms of zero on small maps' % (what, KINK_REL)
    params = dict(m.named_parameters())
    (rel, rn), (el, en) = assert_grads_match({n: p.grad for n, p in params.items()}, ref['grads'], tau[0], tau[1],
                                             n_expected=n_expected, what=what)
    # the buffers: running statistics of every BatchNorm (those the step did not run keep their values), num_batches_tracked exactly
    sd = m.state_dict()
    got_buf, ref_buf = {}, {}
    for k, v in ref['after'].items():
        if k.endswith('num_batches_tracked'):
            ran = ref['count'].get(k[:-len('num_batches_tracked')] + 'running_var', (0, 0))[1]
            assert int(sd[k]) == int(before[k]) + ran, (what, k, int(sd[k]), int(before[k]), ran)
        elif k.endswith(('running_mean', 'running_var')):
            if batch is not None and k in ref['count']:
                n, calls = ref['count'][k]
                assert calls == 1
                v = running_var_for_copies(before[k], v, n, batch // 4)          # (batch / 4 copies of each of the four images)
            got_buf[k], ref_buf[k] = sd[k], v
    assert len(ref['count']) >= 70 and all(not torch.equal(ref['after'][k], before[k]) for k in ref['count'])
    (brel, brn), (bel, ben) = assert_grads_match(got_buf, ref_buf, BUF_TAU_REL, BUF_TAU_EL, what=what + ' buffers')
    lerr = abs(float(loss) - ref['loss']) / abs(ref['loss'])
    print('\n%s: loss %.8g oracle %.8g (rel %.2g) | gradients: worst rel %.3g (%s) worst el %.3g (%s) | buffers: worst rel %.3g (%s) '
          'worst el %.3g (%s)' % (what, float(loss), ref['loss'], lerr, rel, rn, el, en, brel, brn, bel, ben))
    assert lerr <= LOSS_TAU, (what, float(loss), ref['loss'])
    if check_new:
        # SGD's first step, p - lr * (g + wd * p): the gradient's share of the error is bounded by the gradient tolerance, the rest is
        # float32 rounding of the stored value and of the two operations that form it (2^-22 relative)
        for n, want in ref['new'].items():
            g = ref['grads'][n]
            bound = (0.0 if g is None else ref['lr'][n] * tau[1] * float(g.abs().max())) + 2.0 ** -22 * want.abs()
            d = (params[n].detach().to('cpu', torch.float64) - want).abs()
            assert bool((d <= bound).all()), '%s: %s after SGD off by %.3g' % (what, n, float(d.max()))
            if ref['lr'][n] == 0.0 or g is None:
                assert torch.equal(params[n].detach().to('cpu', torch.float64), before[n]), '%s: %s is in no group and moved' % (what, n)
    return rel, el


def _zero_ungrouped(m, opt):
    """See the module docstring: the parameters outside the optimizer keep accumulating, as in the reference."""
    inside = {id(p) for p in opt.params}
    for p in m.parameters():
        if p.grad is not None and id(p) not in inside:
            p.grad.zero_()


def _gpu_batch(case, batch):
    x, y, xd = case.data()
    perm = PERMS[batch] if batch is not None else list(range(x.shape[0]))
    return (x[perm].contiguous().to(DEV), y[perm].contiguous().to(DEV), None if xd is None else xd[perm].contiguous().to(DEV))


@pytest.fixture(scope='module')
def step1_refs():
    """Oracle at the seeded state, keyed by (case, flooding level): shared by every path's first eager step."""
    cache = {}

    def get(name, b=FLOOD):
        if (name, b) not in cache:
            m = CASES[name].model()
            cache[(name, b)] = _oracle(CASES[name], _snapshot(m), _names(m), b)
        return cache[(name, b)]
    return get


def _eager(name, refs, steps=1, batch=None, tau=None, b=FLOOD, n_expected=340, conditioned=True):
    """`steps` eager iterations: each against the oracle at the state it starts from.  Returns the model."""
    from mspl_amd import supervised
    case = CASES[name]
    tau = tau or (SUP_TAU_REL, SUP_TAU_EL)
    m = case.model().to(DEV).train()
    names = _names(m)
    x, y, xd = _gpu_batch(case, batch)
    crit, opt = case.criterion(), None
    for step in range(steps):
        before = _snapshot(m)
        if opt is not None:
            _zero_ungrouped(m, opt)
        loss, _, opt = supervised.train_seg_ue_step(m, x, y, crit, opt, depth=xd, b=b)
        torch.cuda.synchronize()
        ref = refs(name, b) if step == 0 else _oracle(case, before, names, b)
        what = '%s batch %s b=%g eager step %d' % (name, batch or case.shape[0], b, step + 1)
        stepped = step > 0 and batch is None
        _compare(m, loss, ref, before, what, conditioned=conditioned and step == 0,
                 tau=(STEPPED_TAU_REL, STEPPED_TAU_EL) if stepped else tau, batch=batch, n_expected=n_expected,
                 check_new=step == 0)
    return m


def _graphed(name, replays, batch=None, tau=None):
    """GraphedSupervisedStep as bench.py builds it (construction runs one eager iteration and the first replay): every further replay
    against the oracle at the state it starts from -- the workspaces' "handed back zeroed" contract and the running statistics
    advancing inside the graph, replay by replay."""
    from mspl_amd import supervised
    case = CASES[name]
    tau = tau or (STEPPED_TAU_REL, STEPPED_TAU_EL)
    m = case.model().to(DEV).train()
    names = _names(m)
    x, y, xd = _gpu_batch(case, batch)
    gs = supervised.GraphedSupervisedStep(m, x, y, case.criterion(), depth=xd)
    for r in range(replays):
        torch.cuda.synchronize()
        before = _snapshot(m)
        _zero_ungrouped(m, gs.optimizer)
        loss, _ = gs(x, y) if xd is None else gs(x, y, xd)
        torch.cuda.synchronize()
        what = '%s batch %s graph replay %d' % (name, batch or case.shape[0], r + 1)
        _compare(m, loss, _oracle(case, before, names), before, what, conditioned=False, tau=tau, batch=batch)
        assert int(m.state_dict()['base_net.level1.bn.num_batches_tracked']) == r + 3
    return m


class Spy:
    """Which forms ran: every BatchNorm node's forward as (small, with residual), and the fused EESP / pyramid nodes as (large plane,
    stride) / (large plane,) -- large: above the one-launch rule of the library, mspl_bn_train_small_fits."""

    def __init__(self, monkeypatch):
        from mspl_amd import autograd as ag
        from mspl_amd._native import lib
        self.bn, self.eesp, self.pyr = [], [], []
        bn_forward, eesp_apply, pyr_apply = ag._bn_train_forward, ag.EespDwBNFn.apply, ag.PyrBodyBNFn.apply

        def large(n, c, hw):
            return not lib.mspl_bn_train_small_fits(int(n), int(c), int(hw))

        def bn(z, residual, *a):
            out = bn_forward(z, residual, *a)
            assert bool(out[2]) == (ag._SMALL_BN and not large(z.shape[0], z.shape[1], z.shape[2] * z.shape[3]))
            self.bn.append((bool(out[2]), residual is not None))
            return out

        def eesp(x, w0, w1, w2, w3, dil, stride, *a):
            ho, wo = (x.shape[2] - 1) // stride + 1, (x.shape[3] - 1) // stride + 1
            self.eesp.append((large(x.shape[0], 4 * x.shape[1], ho * wo), stride))
            return eesp_apply(x, w0, w1, w2, w3, dil, stride, *a)

        def pyr(x, *a):
            self.pyr.append((large(x.shape[0], x.shape[1], x.shape[2] * x.shape[3]),))
            return pyr_apply(x, *a)
        monkeypatch.setattr(ag, '_bn_train_forward', bn)
        monkeypatch.setattr(ag.EespDwBNFn, 'apply', eesp)
        monkeypatch.setattr(ag.PyrBodyBNFn, 'apply', pyr)


# ------------------------------------------------------------------ small shapes
@pytest.mark.parametrize('name', ['4x32x48', '2x64x96', '2x48x80', '4x64x64'])
def test_eager_supervised_step_vs_float64_oracle(name, step1_refs):
    """train_seg_ue_step: loss, every gradient, the buffers and the parameters after SGD; three steps on the smallest case."""
    _eager(name, step1_refs, steps=3 if name == SMALLEST else 1)


VARIANTS = {'small_bn_off': ('autograd', '_SMALL_BN', False),            # every BatchNorm node through the two-launch kernels
            'fused_bn_train_off': ('layers', '_FUSED_BN_TRAIN', False),
            'eesp_dw_bn_off': ('layers', '_EESP_DW_BN', False),
            'conv_skip_off': ('layers', '_CONV_SKIP', False),
            'fused_pyr_train_off': ('layers', '_FUSED_PYR_TRAIN', False),
            'two_head_sum_off': ('supervised', '_TWO_HEAD_SUM', False),
            'grad_sinks_off': None}                                     # MSPL_GRAD_SINKS=0: autograd's AccumulateGrad


@pytest.mark.parametrize('variant', sorted(VARIANTS))
def test_other_forms_meet_the_same_oracle(variant, step1_refs, monkeypatch):
    """The same step in the library's other forms, one switch at a time: the same reference, the same tolerances."""
    import importlib
    if VARIANTS[variant] is None:
        monkeypatch.setenv('MSPL_GRAD_SINKS', '0')
    else:
        mod, attr, value = VARIANTS[variant]
        mod = importlib.import_module('mspl_amd.' + mod)
        assert getattr(mod, attr) is (not value)
        monkeypatch.setattr(mod, attr, value)
    spy = Spy(monkeypatch)
    _eager(SMALLEST, step1_refs)
    if variant == 'small_bn_off':
        # the two-launch kernels (statistics + apply; backward sums + apply) ran every node, with and without a residual
        assert spy.bn and not any(small for small, _ in spy.bn) and any(res for _, res in spy.bn)
    elif variant == 'fused_bn_train_off':
        assert not spy.bn or all(not res for _, res in spy.bn)          # (the fused EESP / pyramid nodes keep their own BatchNorms)
    elif variant == 'eesp_dw_bn_off':
        assert not spy.eesp
    elif variant == 'fused_pyr_train_off':
        assert not spy.pyr
    else:
        assert spy.bn and spy.eesp and spy.pyr and all(small for small, _ in spy.bn)


def test_flooding_below_the_level_flips_every_gradient(step1_refs):
    """b above the loss: the flooded loss is 2b - ce and every gradient changes sign (utilities/train_eval_seg.py:221)."""
    b = 5.0
    plain, flooded = step1_refs(SMALLEST), step1_refs(SMALLEST, b)
    assert plain['loss'] < b and abs(flooded['loss'] - (2 * b - plain['loss'])) <= 1e-12 * b
    for n, g in plain['grads'].items():
        f = flooded['grads'][n]
        assert (g is None and f is None) or float((f + g).abs().max()) <= 1e-12 * float(g.abs().max()), n
    _eager(SMALLEST, step1_refs, b=b)


def test_rgbd_supervised_step_vs_float64_oracle(step1_refs):
    """With a depth image: depth encoder and trainable fusion gates, three SGD groups through train_seg_ue_step(..., depth=...)."""
    ref = step1_refs('rgbd')
    n = sum(1 for g in ref['grads'].values() if g is not None)
    depth = [k for k, g in ref['grads'].items() if g is not None and k.startswith('depth_base_net.')]
    gates = [k for k, g in ref['grads'].items() if g is not None and k.startswith('fusion_gate_level')]
    assert n > 340 and len(gates) == 4 and len(depth) > 100, (n, len(gates), len(depth))
    m = _eager('rgbd', step1_refs, n_expected=n, tau=(RGBD_TAU_REL, RGBD_TAU_EL))
    # the depth encoder is the third group and moved; the gates are in no group
    assert any(ref['lr'][k] == LR * LR_MULT for k in depth) and all(ref['lr'][k] == 0.0 for k in gates)
    del m


@pytest.mark.parametrize('name', [SMALLEST, '2x64x96'])
def test_graph_replays_vs_float64_oracle(name):
    _graphed(name, replays=3)


# ------------------------------------------------------------------ large planes
@pytest.mark.parametrize('batch', [16, 64])
def test_large_planes_eager_vs_float64_oracle(batch, step1_refs, monkeypatch):
    """(16 | 64) x 3 x 192 x 256 made of four distinct images: both BatchNorm forms inside one model, the fused EESP and pyramid nodes
    on large planes; at batch 64 also a two-launch BatchNorm node WITH a residual and a stride-1 EESP node on a large plane (the
    residual-bearing nodes sit at level 3 and below: 16 x 24 x 32 values per channel at batch 16 is still a small plane)."""
    spy = Spy(monkeypatch)
    _eager('192x256', step1_refs, batch=batch, tau=(FULL_TAU_REL, FULL_TAU_EL), conditioned=False)
    _assert_large_forms(spy, batch)


def _assert_large_forms(spy, batch):
    print('BatchNorm nodes (small, residual): %s; EESP nodes (large, stride): %s; pyramid nodes (large,): %s'
          % tuple({k: f.count(k) for k in sorted(set(f))} for f in (spy.bn, spy.eesp, spy.pyr)))
    assert any(small for small, _ in spy.bn) and any(not small for small, _ in spy.bn)
    assert any(small and res for small, res in spy.bn)
    assert (True, 2) in spy.eesp and (False, 1) in spy.eesp
    assert (True,) in spy.pyr and (False,) in spy.pyr
    if batch == 64:
        assert any(not small and res for small, res in spy.bn)
        assert (True, 1) in spy.eesp


def test_large_planes_graph_replays_vs_float64_oracle(monkeypatch):
    spy = Spy(monkeypatch)                       # (sees the eager iteration and the capture of the construction)
    _graphed('192x256', replays=2, batch=16, tau=(FULL_TAU_REL, FULL_TAU_EL))
    _assert_large_forms(spy, 16)


def test_bench_configuration_vs_float64_oracle(monkeypatch):
    """bench.py's supervised_step: 16 x 3 x 288 x 480, C=13, camvid, ignore_idx=255 through GraphedSupervisedStep; a band of void
    labels and non-uniform class weights on top, four distinct images under PERM16, one batch-4 oracle run."""
    spy = Spy(monkeypatch)
    _graphed('bench', replays=1, batch=16, tau=(FULL_TAU_REL, FULL_TAU_EL))
    _assert_large_forms(spy, 16)
