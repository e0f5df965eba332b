"""mspl_amd.script.train_seg and mspl_amd.evaluation.val_seg -- the drop-ins for the reference's single-head loops
(utilities/train_eval_seg.py:16-162) -- against the FLOAT64 golden written by the reference's own train_seg / val_seg
(tests/golden/make_train_seg_golden.py).

Bounds: those of tests/supervised_loop_cases.py, imported (loss average per epoch, areas per epoch within 2 x the near-margin pixels,
a sample of every parameter per tensor within max(5e-5, 4 x the recorded float32-against-float64 gap), running statistics 1e-3);
tests/test_gpu_train_seg_ue_loop.py explains them.  val_seg after the last epoch: the loss within the same loss bound on its own
recorded gap, the areas within 2 x the held-out batches' near-margin pixels, the scalar miou the reference's formula on the areas."""
import gc
import json
import os

import numpy as np
import pytest
import torch

from tests.conftest import GOLDEN
from tests.optim_shadow import StepAudit
from tests.single_head_loop_cases import SINGLE_HEAD_LOOP_CASES, build_model, loop_batches, val_batches
from tests.supervised_loop_cases import (CLASS_WEIGHTS, IGNORE_IDX, LR_MULT, MOMENTUM, NUM_CLASSES, WEIGHT_DECAY, loss_bound, param_bounds,
                                         per_tensor_max)
from tests.synth import grad_sample_index

pytestmark = pytest.mark.gpu
DEV = 'cuda'
K = NUM_CLASSES - 1
META = json.load(open(os.path.join(GOLDEN, 'train_seg_loop.json')))
BUFFER_TAU = 1e-3                # tests/test_gpu_train_seg_ue_loop.py
LOSS_TAU, GRAD_TAU_EL = 5e-6, 2.5e-4        # the project's bounds for a loss and for a gradient element (tests/test_gpu_supervised_grad_parity.py)


class Loader(object):
    """The seeded batches, device-resident; tells the spies when the loop is inside steps 2..K."""

    def __init__(self, batches, spy):
        self.batches, self.spy = batches, spy

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        for i, b in enumerate(self.batches):
            self.spy['inside'] = i >= 1
            yield b
        self.spy['inside'] = False


def _sample(tensors):
    flat = torch.cat([t.detach().reshape(-1)[grad_sample_index(t.numel()).to(DEV)].double() for t in tensors])
    return flat.cpu().numpy()


def _run(name, epochs=None, restated=False, with_val=True):
    from mspl_amd import evaluation, losses, models, script, supervised
    case = SINGLE_HEAD_LOOP_CASES[name]
    spy = {'inside': False, 'inside_calls': [], 'graph_built': 0, 'graph_calls': 0, 'eager_steps': 0, 'reads': [], 'entry_kept': []}
    mp = pytest.MonkeyPatch()
    audit = StepAudit()
    m = ep = None
    try:
        def counted(owner, attr):
            orig = getattr(owner, attr)

            def wrapper(*a, **k):
                if spy['inside']:
                    spy['inside_calls'].append(attr)
                return orig(*a, **k)
            mp.setattr(owner, attr, wrapper)
        counted(torch.cuda, 'synchronize')
        counted(torch.Tensor, 'item')
        counted(torch.Tensor, 'cpu')
        g_init, g_call, t_step, m_read = (supervised.GraphedSupervisedStep.__init__, supervised.GraphedSupervisedStep.__call__,
                                          supervised.train_seg_step, supervised.SupervisedMeters.read)

        def init(self, model, *a, **k):
            spy['graph_built'] += 1
            spy['building'] = True
            spy['heads'] = k.get('heads')
            audit.tag = 'capture'          # the two steps the constructor takes on the batch that only shapes the capture
            before = dict((n, t.detach().clone()) for n, t in list(model.named_parameters()) + list(model.named_buffers()))
            try:
                g_init(self, model, *a, **k)
            finally:
                spy['building'] = False
                audit.tag = None
            after = dict(list(model.named_parameters()) + list(model.named_buffers()))
            spy['entry_kept'].append(torch.stack([(after[n] == t).all() for n, t in before.items()]).all())
            spy['momentum_zero_after_capture'] = ~self.optimizer.buf.any()
            spy['step_count_after_capture'] = self.optimizer.step_count

        def call(self, *a, **k):
            spy['graph_calls'] += 1
            return g_call(self, *a, **k)

        def step(*a, **k):
            if not spy.get('building'):
                spy['eager_steps'] += 1
            return t_step(*a, **k)

        def read(self):
            r = m_read(self)
            spy['reads'].append(r)
            return r
        mp.setattr(supervised.GraphedSupervisedStep, '__init__', init)
        mp.setattr(supervised.GraphedSupervisedStep, '__call__', call)
        mp.setattr(supervised, 'train_seg_step', step)
        mp.setattr(supervised.SupervisedMeters, 'read', read)
        mp.setattr(script, '_FORCE_RESTATED', bool(restated))

        m = build_model(case, models.ESPNetv2Segmentation, models.ESPDNetSegmentation).to(DEV)
        assert [n for n, _ in m.named_parameters()] == META['cases'][name]['names']
        assert [n for n, b in m.named_buffers() if b.is_floating_point()] == META['cases'][name]['buffer_names']
        crit = losses.SegmentationLoss(n_classes=NUM_CLASSES, device=DEV, ignore_idx=IGNORE_IDX, class_weights=torch.tensor(CLASS_WEIGHTS))
        add = losses.NIDLoss() if case['nid'] is not None else None
        loader = Loader([(x.to(DEV), y.to(DEV)) for x, y in loop_batches(case)], spy)
        out = {'miou': [], 'loss_avg': [], 'params': [], 'buffers': [], 'tracked': [], 'optimizers': []}
        epoch = 0
        with audit:
            audit.watch(m)
            for n_epochs in case['phases']:
                lr0 = case['lrs'][epoch] if epoch < len(case['lrs']) else case['lrs'][-1]
                opt = torch.optim.SGD([{'params': m.get_basenet_params(), 'lr': lr0}, {'params': m.get_segment_params(), 'lr': lr0 * LR_MULT}],
                                      lr0, momentum=MOMENTUM, weight_decay=WEIGHT_DECAY)
                out['optimizers'].append(opt)
                for _ in range(n_epochs):
                    if epochs is not None and epoch >= epochs:
                        break
                    lr = case['lrs'][epoch]
                    opt.param_groups[0]['lr'] = lr                  # train_segmentation.py:356-358
                    opt.param_groups[1]['lr'] = lr * LR_MULT
                    miou, avg = script.train_seg(m, loader, opt, crit, NUM_CLASSES, epoch, device=DEV, add_criterion=add,
                                                 weight=case['nid'] if case['nid'] is not None else 1.0)
                    out['miou'].append(miou)
                    out['loss_avg'].append(avg)
                    out['params'].append(_sample(list(m.parameters())))
                    out['buffers'].append(_sample([b for b in m.buffers() if b.is_floating_point()]))
                    out['tracked'].append(sorted(set(int(b) for b in m.buffers() if not b.is_floating_point())))
                    epoch += 1
        if with_val:
            held = [(x.to(DEV), y.to(DEV)) for x, y in val_batches(case)]
            ep = evaluation.EvalPass(m, NUM_CLASSES, class_weights=crit.class_wts, ignore_idx=IGNORE_IDX, aux_weight=0.0, device=DEV)
            for x, y in held:
                ep(x, y)
            out['val_areas'] = ep.areas.cpu().numpy().astype(np.float64)
            out['val'] = evaluation.val_seg(m, held, criterion=crit, num_classes=NUM_CLASSES, device=DEV)
            m.train()
        spy['entry_kept'] = [bool(v) for v in spy['entry_kept']]
        if 'momentum_zero_after_capture' in spy:
            spy['momentum_zero_after_capture'] = bool(spy['momentum_zero_after_capture'])
        out.update(spy=spy, epochs=epoch, audit=_audit_summary(audit, m, name))
        return out
    finally:
        mp.undo()
        # the model holds its graphed step and the step the model: only the cyclic collector frees that graph, and it must not do so
        # inside a later capture (HIP refuses to destroy a graph while a stream captures).  Free it here.
        if m is not None:
            script.release_supervised_loop(m)
        m = ep = None
        audit._entry.clear()
        gc.collect()
        torch.cuda.synchronize()


def _audit_summary(audit, model, label):
    """tests/test_gpu_train_seg_ue_loop.py, _audit_summary."""
    if not audit.records:
        return {'steps': []}
    audit.check(model, frozen_buffers=False, label='single-head loop ' + label)
    loop = [r for r in audit.records if r.tag is None]
    entry = audit._entry[id(model)]
    names = dict((id(p), n) for n, p in model.named_parameters())
    opt = loop[0].opt
    same = all(torch.equal(loop[0].pre[0][o:o + p.numel()].view(torch.int32), entry[names[id(p)]].reshape(-1).view(torch.int32))
               for o, p in zip(opt.bucket.offsets, opt.params))
    out = {'steps': [(r.tag, r.step, tuple(r.lrs)) for r in audit.records],
           'hyper': sorted(set((mu, wd) for r in loop for (_, _, mu, wd) in r.hyper)),
           'fresh_momentum_zero': [not bool(r.pre[2].any()) for r in audit.records if r.step == 1],
           'first_step_from_entry_weights': same, 'groups': [len(g['params']) for g in opt.param_groups]}
    audit.records = []
    return out


_RUNS = {}


def _cached(name):
    if name not in _RUNS:
        _RUNS[name] = _run(name)
    return _RUNS[name]


def _check_epochs(name, g, got, want_loss, want_areas, epochs):
    for e in range(epochs):
        r = got['spy']['reads'][e]
        ref, bound = want_loss[e], loss_bound(want_loss[e], float(g[name + '.loss_gap'][e]))
        dev = abs(got['loss_avg'][e] - ref)
        print('%s epoch %d: loss average %.9g against %.9g (deviation %.2e, allowed %.2e)' % (name, e, got['loss_avg'][e], ref, dev, bound))
        assert dev <= bound
        cap = 2 * int(g[name + '.near'][e].sum())
        l1 = np.abs(r['areas'] - want_areas[e]).sum(1)
        print('    areas L1 per histogram', l1.tolist(), 'allowed', cap)
        assert (l1 <= cap).all()


def _check_params(name, g, sample, want, gaps, what):
    names = META['cases'][name]['names']
    off = g[name + '.params_off']
    err, bound = per_tensor_max(sample - want, off), param_bounds(gaps)
    i = int(np.argmax(err / bound))
    print('%s %s: worst parameter error / bound %.3f (%s: %.3g against %.3g)' % (name, what, err[i] / bound[i], names[i], err[i], bound[i]))
    assert (err <= bound).all(), [(names[j], float(err[j]), float(bound[j])) for j in np.nonzero(err > bound)[0][:8]]


def _against_golden(name, golden):
    case, g, got = SINGLE_HEAD_LOOP_CASES[name], golden('train_seg_loop'), _cached(name)
    steps, epochs = len(case['batches']), sum(case['phases'])
    assert got['epochs'] == epochs and len(got['spy']['reads']) == epochs          # one read per epoch
    for e in range(epochs):
        r, miou = got['spy']['reads'][e], got['miou'][e]
        assert r['steps'] == steps
        a = r['areas']
        iou = a[0] / (a[1] + a[2] - a[0] + steps * 1e-6 + 1e-10)
        assert np.ndim(miou) == 0 and abs(miou - iou[[1, 2, 3]].mean() * 100) <= 1e-9          # :84-89 on the adapter's own areas
        assert isinstance(got['loss_avg'][e], float)
        assert got['tracked'][e] in ([(e + 1) * steps], [0, (e + 1) * steps])
    _check_epochs(name, g, got, g[name + '.loss_avg'], g[name + '.areas'].sum(1), epochs)
    e = 0
    for p, n_epochs in enumerate(case['phases']):
        e += n_epochs
        _check_params(name, g, got['params'][e - 1], g[name + '.params_%d' % p].astype(np.float64), g[name + '.params_gap_%d' % p],
                      'after phase %d' % p)
        boff = g[name + '.buffers_off']
        want = g[name + '.buffers_%d' % p].astype(np.float64)
        rel = [np.linalg.norm(got['buffers'][e - 1][boff[i]:boff[i + 1]] - want[boff[i]:boff[i + 1]]) / np.linalg.norm(want[boff[i]:boff[i + 1]])
               for i in range(len(boff) - 1)]
        print('    running statistics: worst relative norm error %.2e (%s)' % (max(rel), META['cases'][name]['buffer_names'][int(np.argmax(rel))]))
        assert max(rel) <= BUFFER_TAU
    # val_seg after the last epoch on the held-out batches
    vm, vl = got['val']
    ref_m, ref_l = g[name + '.val']
    bound = loss_bound(ref_l, float(g[name + '.val_gap'][1]))
    l1 = np.abs(got['val_areas'] - g[name + '.val_areas']).sum(1)
    print('%s val_seg: miou %.6g against %.6g, loss %.9g against %.9g (allowed %.2e), areas L1 %s allowed %d'
          % (name, vm, ref_m, vl, ref_l, bound, l1.tolist(), 2 * int(g[name + '.val_near'])))
    assert np.ndim(vm) == 0 and abs(vl - ref_l) <= bound
    assert (l1 <= 2 * int(g[name + '.val_near'])).all()
    va = got['val_areas']
    viou = va[0] / (va[1] + va[2] - va[0] + 2 * 1e-6 + 1e-10)
    assert abs(vm - viou[[1, 2, 3]].mean() * 100) <= 1e-9
    return case, got


@pytest.mark.parametrize('name', ['v2_s05_32x48', 'espdnet_32x48'])
def test_loop_against_the_reference_loop(name, golden):
    """The graphed path: what the loop returns, the meters per epoch, every parameter and running statistic after each phase, val_seg
    after the last epoch, and the audited sequence of FlatSGD steps (tests/test_gpu_train_seg_ue_loop.py)."""
    case, got = _against_golden(name, golden)
    steps = len(case['batches'])
    audited, spy = got['audit'], got['spy']
    lr0 = case['lrs'][0]
    want = [('capture', 1, (lr0, lr0 * LR_MULT)), ('capture', 2, (lr0, lr0 * LR_MULT))]
    e = 0
    for n_epochs in case['phases']:
        for k in range(n_epochs):
            lr = case['lrs'][e]
            want += [(None, k * steps + i + 1, (lr, lr * LR_MULT)) for i in range(steps)]
            e += 1
    assert audited['steps'] == want
    assert audited['hyper'] == [(MOMENTUM, WEIGHT_DECAY)]
    assert audited['fresh_momentum_zero'] == [True] * (1 + len(case['phases']))
    assert audited['first_step_from_entry_weights'] is True
    assert spy['entry_kept'] == [True] and spy['momentum_zero_after_capture'] is True and spy['step_count_after_capture'] == 0
    assert len(audited['groups']) == 2 and all(n > 0 for n in audited['groups'])


@pytest.mark.parametrize('name', ['v2_s05_32x48', 'espdnet_32x48'])
def test_fast_path_runs_on_one_graphed_step_without_host_sync(name):
    """One graph (heads=1), K - 1 replays per epoch plus the eager partial batch, no host read inside the loop, one meter read per
    epoch, and the caller's SGD left with empty state."""
    case, got = SINGLE_HEAD_LOOP_CASES[name], _cached(name)
    spy, epochs = got['spy'], sum(case['phases'])
    full = sum(1 for b in case['batches'] if b == case['batches'][0])
    assert spy['graph_built'] == 1 and spy['heads'] == 1
    assert spy['graph_calls'] == full * epochs and spy['eager_steps'] == (len(case['batches']) - full) * epochs
    assert spy['inside_calls'] == []
    assert len(spy['reads']) == epochs
    assert all(len(o.state) == 0 for o in got['optimizers'])


def test_nid_case_takes_the_restated_body_and_meets_its_golden(golden):
    """The loop around the additional criterion: restated body, the caller's optimizer, the extra meter.  Its parameter bound is 4 x the
    reference's own float32 gap at this case (3e-4: tests/single_head_loop_cases.py), about 1.2e-3 per tensor after two steps, which
    still sees a batch applied twice or dropped (asserted by the generator) but NOT a `weight` wrong by a factor of order 1;
    test_additional_criterion_enters_the_step_with_its_weight checks that directly."""
    case, got = _against_golden('v2_nid_32x48', golden)
    assert got['spy']['graph_built'] == 0 and got['spy']['graph_calls'] == 0 and got['audit']['steps'] == []
    assert all(len(o.state) > 0 for o in got['optimizers'])                   # the caller's own optimizer stepped
    assert got['spy']['reads'][0]['extra_sum'] != 0.0                         # the additional loss went into its meter


def _nid_setup():
    from mspl_amd import losses, models
    case = SINGLE_HEAD_LOOP_CASES['v2_nid_32x48']
    m = build_model(case, models.ESPNetv2Segmentation, models.ESPDNetSegmentation).to(DEV)
    crit = losses.SegmentationLoss(n_classes=NUM_CLASSES, device=DEV, ignore_idx=IGNORE_IDX, class_weights=torch.tensor(CLASS_WEIGHTS))
    return case, m, crit, losses.NIDLoss()


def test_additional_criterion_enters_the_step_with_its_weight():
    """What the NID golden's parameter bound (4 x a float32 gap of 3e-4, i.e. 1.2e-3 per tensor after two steps) can no longer see: a
    `weight` wrong by a factor of order 1, or applied to the cross entropy too.  So directly, for one batch: the loss of
    supervised._single_head_loss with an additional criterion is criterion(out).mean() + weight * add_criterion(inputs, out) on the
    model's own output, the gradient it sends into that output is d ce + weight * d nid (autograd on the two terms separately), and
    the meters get loss * n and weight * nid."""
    from mspl_amd import supervised
    case, m, crit, nid = _nid_setup()
    m.eval()
    x, y = [t.to(DEV) for t in loop_batches(case)[0]]
    weight = 0.5
    with torch.no_grad():                                   # (some realistic logits of this model: both sides below start from them)
        out = m(x).detach()
    o = out.clone().requires_grad_()
    ce, extra = crit(o, y).mean(), nid(x, o)
    g_ce, g_nid = torch.autograd.grad(ce, o, retain_graph=True)[0], torch.autograd.grad(extra, o)[0]
    ce, extra = ce.detach(), extra.detach()
    meters = supervised.SupervisedMeters(K, DEV)
    got = {}

    class Probe(torch.nn.Module):                           # the model's output as a leaf: what _single_head_loss differentiates
        def forward(self, inputs):
            got['o'] = out.clone().requires_grad_()
            return got['o']
    loss, logits = supervised._single_head_loss(Probe(), x, y, None, crit, nid, weight, meters)
    loss.backward()
    want = float(ce) + weight * float(extra)
    print('loss %.9g against ce %.9g + %.2g x nid %.9g = %.9g' % (float(loss.detach()), float(ce), weight, float(extra), want))
    assert abs(float(loss.detach()) - want) <= LOSS_TAU * abs(want)
    gw = g_ce + weight * g_nid
    d = float((got['o'].grad - gw).abs().max())
    assert d <= GRAD_TAU_EL * float(gw.abs().max()), d          # (NIDLoss's histograms are float sums: two evaluations differ in rounding)
    # a weight of 1 or a weight on both terms would be off by far more than that
    assert float((g_ce + g_nid - gw).abs().max()) > 100 * GRAD_TAU_EL * float(gw.abs().max())
    n = x.shape[0]
    assert abs(float(meters.meter[0]) - want * n) <= LOSS_TAU * want * n
    assert abs(float(meters.meter[1]) - weight * float(extra)) <= LOSS_TAU * weight * abs(float(extra))
    assert logits is got['o']


def test_val_seg_with_an_additional_criterion():
    """val_seg's per-batch body for an additional criterion (utilities/train_eval_seg.py:122-124: `loss += add_criterion(inputs,
    outputs)`, NO weight): the average loss is that of criterion + NID on the model's eval() outputs, the miou that of val_seg
    without the additional criterion."""
    from mspl_amd import evaluation
    case, m, crit, nid = _nid_setup()
    held = [(x.to(DEV), y.to(DEV)) for x, y in val_batches(case)]
    miou, loss = evaluation.val_seg(m, held, criterion=crit, num_classes=NUM_CLASSES, device=DEV, add_criterion=nid)
    plain_miou, plain_loss = evaluation.val_seg(m, held, criterion=crit, num_classes=NUM_CLASSES, device=DEV)
    m.eval()
    tot = cnt = 0.0
    extras = []
    with torch.no_grad():
        for x, y in held:
            o = m(x)
            e = float(nid(x, o))
            extras.append(e)
            tot += (float(crit(o, y).mean()) + e) * x.shape[0]
            cnt += x.shape[0]
    print('val_seg with NID: loss %.9g against %.9g (cross entropy alone %.9g, NID per batch %s), miou %.6g / %.6g'
          % (loss, tot / cnt, plain_loss, extras, miou, plain_miou))
    assert abs(loss - tot / cnt) <= 1e-6 * abs(tot / cnt)
    assert min(extras) > 1e-3 and loss > plain_loss + 0.5 * min(extras)           # the term is there, unweighted
    assert abs(miou - plain_miou) <= 1e-9
    del m
    gc.collect()


def test_fast_path_against_restated_body(golden):
    """v2_s05_32x48's first epoch through the graphed step and through the restated reference body (forced by the internal switch):
    the same loss-average, area and parameter bounds as against the golden."""
    name = 'v2_s05_32x48'
    g = golden('train_seg_loop')
    fast, slow = _cached(name), _run(name, epochs=1, restated=True, with_val=False)
    assert slow['spy']['graph_built'] == 0 and len(slow['optimizers'][0].state) > 0
    _check_epochs(name, g, fast, slow['loss_avg'], [r['areas'] for r in slow['spy']['reads']], 1)
    _check_params(name, g, fast['params'][0], slow['params'][0], g[name + '.params_gap_0'], 'fast against restated, epoch 0')
    _check_epochs(name, g, slow, g[name + '.loss_avg'], g[name + '.areas'].sum(1), 1)
