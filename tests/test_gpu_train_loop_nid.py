"""mspl_amd.script.train(..., add_loss=NIDLoss(image_bin=32, label_bin=5)) -- the self-training loop with the paper's NID regulariser
(uest_seg_multi_os.py:958-1089 with :1027-1030 taken, `--use-nid true`) -- against the golden written by the reference's own train()
(tests/golden/make_train_loop_nid_golden.py), and on which path it runs: ONE graphed step with one lane, the NID term taken from
the low-resolution main head inside the graph (csrc/nid_heads.hip), no host synchronisation inside the steps.

Bounds: max(LOSS_RTOL |ref| + LOSS_ATOL, GAP_FACTOR x the generator's recorded float32-against-float64 gap of the reference) for the
written averages, the per-step loss and the per-step NID term; areas within twice the near-pixel count; weights by
assert_weights_close_after_adam.  Modelled on tests/test_gpu_train_loop.py (its spies are re-declared here)."""
import argparse
import json
import os

import numpy as np
import pytest
import torch

from tests.conftest import GOLDEN
from tests.synth import assert_weights_close_after_adam, grad_sample_index, synth_state_dict
from tests.train_loop_nid_cases import (CLASS_WEIGHTS, IGNORE_IDX, LR, NID_IMAGE_BIN, NID_LABEL_BIN, TOT_ITER, TRAIN_LOOP_NID_CASES,
                                        WEIGHT_DECAY, WRITER_IDX0, loop_args, loop_batches, loss_bound)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
KEYS = json.load(open(os.path.join(GOLDEN, 'state_dict_keys.json')))
META = json.load(open(os.path.join(GOLDEN, 'train_loop_nid.json')))
CASES = sorted(TRAIN_LOOP_NID_CASES)


class Writer(object):
    def __init__(self):
        self.records = []

    def add_scalar(self, tag, value, idx):
        self.records.append([tag, float(value), int(idx)])


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


def _sample(model):
    flat = torch.cat([p.detach().reshape(-1)[grad_sample_index(p.numel()).to(DEV)] for p in model.parameters()])
    return flat.cpu().numpy()


def _model(case):
    from mspl_amd import models
    m = models.ESPDNetwithUncertaintyEstimation(argparse.Namespace(s=2.0, channels=3, num_classes=1000), classes=5,
                                                dataset='greenhouse', fix_pyr_plane_proj=True)
    m.load_state_dict(synth_state_dict(KEYS['espdnetue_s2.0_c5'], case['sd_seed']))
    return m.to(DEV).eval()


def _run(name, epochs=None, restated=False):
    """The generator's schedule through script.train.  Returns what the loop wrote and returned, the meters read per epoch, the
    per-step loss and NID term (device scalars kept per step, read after the loop), a parameter sample per epoch and the spies."""
    from mspl_amd import losses, script, training
    case = TRAIN_LOOP_NID_CASES[name]
    spy = {'inside': False, 'inside_calls': [], 'graph_built': 0, 'graph_calls': 0, 'eager_steps': 0, 'reads': [], 'lanes': [],
           'heads_calls': 0, 'full_calls': 0, 'steps': []}
    mp = pytest.MonkeyPatch()
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
        g_init, g_call, t_step, m_read, m_count = (training.GraphedTrainStep.__init__, training.GraphedTrainStep.__call__,
                                                   training.train_step, training.TrainMeters.read, training.TrainMeters.count)
        at_heads, nid_forward = losses.NIDLoss.at_heads, losses.NIDLoss.forward

        def init(self, *a, **k):
            spy['graph_built'] += 1
            spy['building'] = True
            try:
                g_init(self, *a, **k)
            finally:
                spy['building'] = False
            spy['lanes'].append((k.get('lanes'), self.lanes))

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

        def count(self, batch_size):
            # one step went in: keep the meter's running sums on the device (a clone, no sync); differences give the per-step values
            if not spy.get('building'):
                spy['steps'].append((self.meter.clone(), int(batch_size)))
            return m_count(self, batch_size)

        def heads(self, *a, **k):
            spy['heads_calls'] += 1
            return at_heads(self, *a, **k)

        def full(self, *a, **k):
            spy['full_calls'] += 1
            return nid_forward(self, *a, **k)
        mp.setattr(training.GraphedTrainStep, '__init__', init)
        mp.setattr(training.GraphedTrainStep, '__call__', call)
        mp.setattr(training, 'train_step', step)
        mp.setattr(training.TrainMeters, 'read', read)
        mp.setattr(training.TrainMeters, 'count', count)
        mp.setattr(losses.NIDLoss, 'at_heads', heads)
        mp.setattr(losses.NIDLoss, 'forward', full)
        mp.setattr(script, '_FORCE_RESTATED', bool(restated))

        m = _model(case)
        crit = losses.UncertaintyWeightedSegmentationLoss(5, class_weights=torch.tensor(CLASS_WEIGHTS), ignore_idx=IGNORE_IDX, device=DEV)
        nid = losses.NIDLoss(image_bin=NID_IMAGE_BIN, label_bin=NID_LABEL_BIN)
        loader = Loader([(x.to(DEV), y.to(DEV)) for x, y in loop_batches(case)], spy)
        ns = {'in_training_visualization_img': lambda model, **kw: None}
        assert 'train' in script.patch_script(ns, train=True)
        args, writer, idx = loop_args(case), Writer(), WRITER_IDX0
        out = {'returned': [], 'params': [], 'optimizers': []}
        epoch = 0
        for n_epochs in case['phases']:
            opt = torch.optim.Adam(m.parameters(), lr=LR, weight_decay=WEIGHT_DECAY)
            out['optimizers'].append(opt)
            for _ in range(n_epochs):
                if epochs is not None and epoch >= epochs:
                    break
                idx = ns['train'](loader, m, crit, DEV, None, opt, TOT_ITER, 0, epoch, args, None, None, None, idx, None, writer, nid)
                out['returned'].append(int(idx))
                out['params'].append(_sample(m))
                epoch += 1
        # per-step values from the meter's running sums: meter[0] += B * loss, meter[1] += loss2; reset to zero at each epoch's start
        n_steps = len(case['batches'])
        loss, loss2 = np.zeros((epoch, n_steps)), np.zeros((epoch, n_steps))
        for i, (mt, b) in enumerate(spy['steps']):
            e, s = divmod(i, n_steps)
            cur = mt.cpu().numpy()
            prev = spy['steps'][i - 1][0].cpu().numpy() if s > 0 else np.zeros(2)
            loss[e, s], loss2[e, s] = (cur[0] - prev[0]) / b, cur[1] - prev[1]
        out.update(records=writer.records, spy=spy, epochs=epoch, loss=loss, loss2=loss2)
        return out
    finally:
        mp.undo()


_RUNS = {}


def _cached(name):
    if name not in _RUNS:
        _RUNS[name] = _run(name)
    return _RUNS[name]


def _check(name, g, got, ref_records, epochs, ref=None):
    """Averages, per-step values and areas of `got` against the golden (ref=None) or against another run of this project."""
    for e in range(epochs):
        rec, want = got['records'][8 * e:8 * e + 8], ref_records[8 * e:8 * e + 8]
        for i, key in ((0, 'gap_loss_avg'), (1, 'gap_nid_avg')):
            dev, bound = abs(rec[i][1] - want[i][1]), loss_bound(want[i][1], float(g[name + '.' + key][e]))
            print('%s epoch %d %s: %.9g against %.9g (deviation %.2e, bound %.2e)' % (name, e, rec[i][0], rec[i][1], want[i][1], dev, bound))
            assert dev <= bound
        for key, gap in (('loss', 'gap_loss'), ('loss2', 'gap_loss2')):
            want_steps = g[name + '.' + key][e] if ref is None else ref[key][e]
            for s, (a, b) in enumerate(zip(got[key][e], want_steps)):
                bound = loss_bound(b, float(g[name + '.' + gap][e][s]))
                print('    step %d %s %.9g against %.9g (deviation %.2e, bound %.2e)' % (s, key, a, b, abs(a - b), bound))
                assert abs(a - b) <= bound
        cap = 2 * int(g[name + '.near'][e].sum())
        want_areas = g[name + '.areas'][e].sum(0) if ref is None else ref['spy']['reads'][e]['areas']
        l1 = np.abs(got['spy']['reads'][e]['areas'] - want_areas).sum(1)
        print('    areas L1 per histogram', l1.tolist(), 'allowed', cap)
        assert (l1 <= cap).all()


@pytest.mark.parametrize('name', CASES)
def test_nid_loop_runs_on_one_graphed_step_with_one_lane(name):
    """With NID the loop builds exactly one GraphedTrainStep, with lanes == 1 even where train_lanes = 2 is asked for, replays it for
    every full batch and takes train_step for the partial one; the NID term comes from the low-resolution head (NIDLoss.at_heads),
    never from full-size logits; nothing inside steps 2..K calls synchronize / .item() / .cpu(); the meters are read once per epoch;
    the caller's Adam never steps."""
    case, got = TRAIN_LOOP_NID_CASES[name], _cached(name)
    spy, epochs = got['spy'], sum(case['phases'])
    full = sum(1 for b in case['batches'] if b == case['batches'][0])
    assert spy['graph_built'] == 1
    asked, lanes = spy['lanes'][0]
    assert lanes == 1 and asked == (case['train_lanes'] if case['train_lanes'] is not None else 2)
    assert spy['graph_calls'] == full * epochs and spy['eager_steps'] == (len(case['batches']) - full) * epochs
    assert spy['inside_calls'] == []
    assert len(spy['reads']) == epochs
    assert all(len(o.state) == 0 for o in got['optimizers'])
    # the eager construction step, the capture, and one per partial batch; replays call nothing in Python
    assert spy['heads_calls'] == 2 + spy['eager_steps'] and spy['full_calls'] == 0


@pytest.mark.parametrize('name', CASES)
def test_nid_loop_against_the_reference_loop(name, golden):
    case, g, meta, got = TRAIN_LOOP_NID_CASES[name], golden('train_loop_nid'), META[name], _cached(name)
    steps, epochs = len(case['batches']), sum(case['phases'])
    ref = meta['records']
    assert got['epochs'] == epochs and got['returned'] == meta['returned']
    assert [r[0] for r in got['records']] == [r[0] for r in ref] and [r[2] for r in got['records']] == [r[2] for r in ref]
    for e in range(epochs):
        rec, r = got['records'][8 * e:8 * e + 8], got['spy']['reads'][e]
        assert rec[1][0] == 'uest/train/nid_loss' and r['steps'] == steps
        assert abs(rec[7][1] - ref[8 * e + 7][1]) <= 1e-12                    # learning rate after the last step
        np.testing.assert_allclose(rec[1][1], r['extra_sum'] / steps, rtol=1e-12)
    _check(name, g, got, ref, epochs)
    done, e = 0, 0
    for p, n_epochs in enumerate(case['phases']):
        e += n_epochs
        done += n_epochs * steps
        assert_weights_close_after_adam(got['params'][e - 1], g[name + '.params_%d' % p], LR, done)


def test_nid_loop_graphed_against_restated_body(golden):
    """loop_nid_32x48's first epoch through the graphed step and through the restated reference body: the same bounds."""
    name = 'loop_nid_32x48'
    case, g = TRAIN_LOOP_NID_CASES[name], golden('train_loop_nid')
    fast, slow = _cached(name), _run(name, epochs=1, restated=True)
    assert slow['spy']['graph_built'] == 0 and len(slow['optimizers'][0].state) > 0
    assert slow['spy']['heads_calls'] == 0 and slow['spy']['full_calls'] == len(case['batches'])
    _check(name, g, fast, slow['records'], 1, ref=slow)
    assert_weights_close_after_adam(fast['params'][0], slow['params'][0], LR, len(case['batches']))


def test_step_captured_without_nid_refuses_nid_later():
    """A model whose graphed step was captured without the additional loss and is then trained with it raises (and the other way
    round, and for other NIDLoss settings): a captured graph cannot change its loss."""
    from mspl_amd import losses, script
    case = TRAIN_LOOP_NID_CASES['loop_nid_32x48']
    m = _model(case)
    crit = losses.UncertaintyWeightedSegmentationLoss(5, class_weights=torch.tensor(CLASS_WEIGHTS), ignore_idx=IGNORE_IDX, device=DEV)
    loader = [(x.to(DEV), y.to(DEV)) for x, y in loop_batches(case)][:1]
    args = loop_args(case)
    opt = torch.optim.Adam(m.parameters(), lr=LR, weight_decay=WEIGHT_DECAY)
    run = lambda add: script.train(loader, m, crit, DEV, None, opt, TOT_ITER, 0, 0, args, None, None, None, 0, None, Writer(), add)
    run(None)
    with pytest.raises(RuntimeError, match='captured without an additional loss'):
        run(losses.NIDLoss(image_bin=NID_IMAGE_BIN, label_bin=NID_LABEL_BIN))
    m2 = _model(case)
    opt = torch.optim.Adam(m2.parameters(), lr=LR, weight_decay=WEIGHT_DECAY)
    run2 = lambda add: script.train(loader, m2, crit, DEV, None, opt, TOT_ITER, 0, 0, args, None, None, None, 0, None, Writer(), add)
    run2(losses.NIDLoss(image_bin=NID_IMAGE_BIN, label_bin=NID_LABEL_BIN))
    run2(losses.NIDLoss(image_bin=NID_IMAGE_BIN, label_bin=NID_LABEL_BIN))          # another object, the same settings: fine
    with pytest.raises(RuntimeError, match='is now called without an additional loss'):
        run2(None)
    with pytest.raises(RuntimeError, match='image_bin=16'):
        run2(losses.NIDLoss(image_bin=16, label_bin=NID_LABEL_BIN))
