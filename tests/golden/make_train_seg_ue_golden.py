#!/usr/bin/env python3
"""Generate tests/golden/train_seg_ue_loop.npz / .json by running the REFERENCE's own train_seg_ue
(utilities/train_eval_seg.py:164-247) on the CPU.

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout>:<this repository> python3 tests/golden/make_train_seg_ue_golden.py

`train_seg_ue` (its module's imports are not all torch-only) and `AverageMeter` are AST-extracted at run time and run with the
reference's own model in train() mode, its SegmentationLoss, NIDLoss and MIOU classes and torch.optim.SGD over the model's two
learning-rate groups; the loader is the list of seeded batches of tests/supervised_loop_cases.py.  Only data is written.

Every case runs in float64 with four threads -- the GOLDEN -- and in float32 several times (FLOAT32_RUNS of
tests/supervised_loop_cases.py): with 1, 2 and 4 threads, and with four threads on images moved by one ulp, six seeded times.  In
train() mode the level-4 maps of these cases hold 24 to 96 values per channel, one PReLU input changing side moves a channel's batch
statistics by per cent, and the float32 trajectory is bimodal under such perturbations: most runs stay within 1e-6 of float64, some
leave by 1e-4 in single tensors.  The LARGEST distance of any float32 run from the float64 run is what is recorded beside the golden
per epoch and per tensor, so that the tests' `4 x gap` speaks for the case's sensitivity and not for one lucky run.

Per case (npz keys `<case>.<name>`):
    areas          (epochs, steps, 3, 4) int64: [inter | pred | mask] of MIOU(4) per step, float64 run
    loss           (epochs, steps) float64: the flooded loss given to losses.update per step
    near           (epochs, steps) int64: pixels whose top-2 margin of the summed logits is below NEAR_MARGIN
    loss_avg       (epochs,) the returned average;  iou (epochs, 4) the returned array
    loss_gap       (epochs,) largest |float32 - float64| of the returned average over the float32 runs
    area_gap       (epochs, 3) L1 distance per histogram between the two runs' epoch sums
    params_<p>     the strided sample (tests.synth.grad_sample_index) of EVERY parameter after the last step of phase p (float64 run)
    params_gap_<p> per-tensor largest |float32 - float64| of that sample over the float32 runs
    buffers_<p>    running_mean / running_var of every BatchNorm (sampled the same way) after phase p
    params_off / buffers_off   offsets of the tensors inside a sample
The json holds the signature of the reference function and the names behind the offsets.

The generator asserts that the test has teeth: the near-tie share is at most NEAR_CAP, and a float64 run that applies the first
batch twice, and one that drops the last batch, each leave the parameter bound of the tests in tensors of BOTH learning-rate groups.
"""
import argparse
import ast
import inspect
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.supervised_loop_cases import (CLASS_WEIGHTS, FLOAT32_RUNS, IGNORE_IDX, LR_MULT, MOMENTUM, NEAR_CAP, NEAR_MARGIN, NUM_CLASSES, PARAM_FLOOR,  # noqa: E402
                                         SUPERVISED_LOOP_CASES, WEIGHT_DECAY, group_of, loop_batches, param_bounds, per_tensor_max)
from tests.synth import grad_sample_index, synth_state_dict  # noqa: E402
from tests.train_loop_cases import reference_areas  # noqa: E402

# reference imports (torch-only modules)
from model.segmentation.espdnet_ue import ESPDNetwithUncertaintyEstimation  # noqa: E402
from loss_fns.segmentation_loss import NIDLoss, PixelwiseKLD, SegmentationLoss  # noqa: E402
from utilities.metrics.segmentation_miou import MIOU  # noqa: E402
import utilities.metrics.segmentation_miou as _miou_mod  # noqa: E402

REF = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(_miou_mod.__file__))))
K = NUM_CLASSES - 1


def extract(path, names, ns, classes=()):
    tree = ast.parse(open(path).read())
    for node in tree.body:
        if (isinstance(node, ast.FunctionDef) and node.name in names) or (isinstance(node, ast.ClassDef) and node.name in classes):
            exec(compile(ast.Module([node], []), path, 'exec'), ns)
    return ns


class _run_dtype(object):
    """NIDLoss builds its tensors with hard-coded `.to('cuda')` and `.float()` (loss_fns/segmentation_loss.py:79-82, 138-141), which
    cannot run on the CPU or in float64: inside this context a 'cuda' target means "stay where you are" and `.float()`
    and the default dtype mean the dtype of the run -- the reference's arithmetic is untouched."""

    def __init__(self, dtype):
        self.dtype = dtype

    def __enter__(self):
        real_to = self.real_to = torch.Tensor.to
        self.real_float = torch.Tensor.float
        self.default = torch.get_default_dtype()
        dtype = self.dtype

        def cpu_to(t, *a, **k):
            dev = a[0] if a else k.get('device')
            if isinstance(dev, str) and dev.startswith('cuda'):
                return t
            return real_to(t, *a, **k)
        torch.Tensor.to = cpu_to
        torch.Tensor.float = lambda t: real_to(t, dtype)
        torch.set_default_dtype(dtype)

    def __exit__(self, *exc):
        torch.Tensor.to = self.real_to
        torch.Tensor.float = self.real_float
        torch.set_default_dtype(self.default)


def sample(tensors):
    parts = [t.detach().reshape(-1)[grad_sample_index(t.numel())].double() for t in tensors]
    off = np.cumsum([0] + [len(t) for t in parts])
    return torch.cat(parts).numpy(), off


def one_ulp(x, seed):
    """x with every element moved to a neighbouring float32, up or down by a seeded coin."""
    g = torch.Generator().manual_seed(9000 + seed)
    up = torch.rand(x.shape, generator=g) < 0.5
    return torch.where(up, torch.nextafter(x, torch.full_like(x, float('inf'))), torch.nextafter(x, torch.full_like(x, -float('inf'))))


def run_case(case, dtype, loaders=None, threads=4, perturb=None):
    """loaders: optional {epoch index: list of batches} replacing the case's loader in that epoch (the teeth runs).  threads: ATen's
    thread count for this run (it decides how sums are split).  perturb: a seed -- the images move by one ulp (one_ulp)."""
    torch.set_num_threads(threads)
    ns = {'torch': torch, 'np': np, 'PixelwiseKLD': PixelwiseKLD, 'print_log_message': lambda *a: None, 'print': lambda *a: None}
    import collections
    import time
    ns.update(OrderedDict=collections.OrderedDict, time=time, gather=None)
    extract(os.path.join(REF, 'utilities/utils.py'), (), ns, classes=('AverageMeter',))
    extract(os.path.join(REF, 'utilities/train_eval_seg.py'), {'train_seg_ue'}, ns)
    log = {'loss': [], 'areas': [], 'near': [], 'meters': 0}

    class RecMeter(ns['AverageMeter']):        # `losses` is the first meter train_seg_ue builds (:166)
        def __init__(self):
            super().__init__()
            self.rec = log['meters'] == 0
            log['meters'] += 1

        def update(self, val, n=1):
            if self.rec:
                log['loss'].append(float(val))
            super().update(val, n)

    class RecMIOU(MIOU):
        def get_iou(self, output, target):
            srt = torch.sort(output.detach(), dim=1, descending=True)[0]
            log['near'].append(int(((srt[:, 0] - srt[:, 1]) < NEAR_MARGIN).sum()))
            a = reference_areas(torch.max(output.detach(), 1)[1].numpy(), target.numpy(), self.num_classes)
            inter, union = super().get_iou(output, target)
            assert np.array_equal(inter.astype(np.int64), a[0]) and np.allclose(union, a[1] + a[2] - a[0] + self.epsilon)
            log['areas'].append(a)
            return inter, union

    ns.update(AverageMeter=RecMeter, MIOU=RecMIOU)
    m = ESPDNetwithUncertaintyEstimation(argparse.Namespace(s=2.0, channels=3, num_classes=1000), classes=NUM_CLASSES, dataset='greenhouse',
                                         fix_pyr_plane_proj=True)
    m.load_state_dict(synth_state_dict(m.state_dict(), case['sd_seed']))
    m = m.to(dtype)
    crit = SegmentationLoss(n_classes=NUM_CLASSES, device='cpu', ignore_idx=IGNORE_IDX, class_weights=torch.tensor(CLASS_WEIGHTS, dtype=dtype))
    base = [((x if perturb is None else one_ulp(x, 17 * perturb + i)).to(dtype), y) for i, (x, y) in enumerate(loop_batches(case))]
    out = {'loss_avg': [], 'iou': [], 'params': [], 'buffers': [], 'steps': []}
    epoch = 0
    with _run_dtype(dtype):
        add = NIDLoss() if case['nid'] is not None else None
        for n_epochs in case['phases']:
            lr0 = case['lrs'][epoch]
            opt = torch.optim.SGD([{'params': m.get_basenet_params(), 'lr': lr0}, {'params': m.get_segment_params(), 'lr': lr0 * LR_MULT}],
                                  lr0, momentum=MOMENTUM, weight_decay=WEIGHT_DECAY)
            for _ in range(n_epochs):
                lr = case['lrs'][epoch]
                opt.param_groups[0]['lr'] = lr                       # train_segmentation.py:356-358
                opt.param_groups[1]['lr'] = lr * LR_MULT
                loader = base if (loaders is None or epoch not in loaders) else [base[i] for i in loaders[epoch]]
                log['meters'] = 0
                # device='cuda' selects the branch the script runs (:199-209, `.mean()` of the loss); no tensor is moved by it here
                iou, avg = ns['train_seg_ue'](m, loader, opt, crit, NUM_CLASSES, epoch, device='cuda', add_criterion=add,
                                              weight=case['nid'] if case['nid'] is not None else 1.0)
                out['loss_avg'].append(float(avg))
                out['iou'].append(np.asarray(iou, dtype=np.float64))
                out['steps'].append(len(loader))
                epoch += 1
            out['params'].append(sample(list(m.parameters())))
            out['buffers'].append(sample([b for b in m.buffers() if b.is_floating_point()]))
    out['names'] = [n for n, _ in m.named_parameters()]
    out['buffer_names'] = [n for n, b in m.named_buffers() if b.is_floating_point()]
    out['loss'], out['areas'], out['near'] = log['loss'], log['areas'], log['near']
    return out


def by_epoch(values, steps):
    out, i = [], 0
    for s in steps:
        out.append(values[i:i + s])
        i += s
    return out


def main():
    arrays, meta = {}, {'cases': {}}
    ns = extract(os.path.join(REF, 'utilities/train_eval_seg.py'), {'train_seg_ue'}, {})
    sig = inspect.signature(ns['train_seg_ue'])
    meta['signature'] = {'names': list(sig.parameters),
                         'defaults': {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}}
    for name, case in sorted(SUPERVISED_LOOP_CASES.items()):
        g64 = run_case(case, torch.float64)
        # the reference's own float32 error at this case: other summation orders (thread counts) and images one ulp away
        g32s = [run_case(case, torch.float32, threads=nt, perturb=k) for nt, k in FLOAT32_RUNS]
        g32 = g32s[0]
        steps, epochs = len(case['batches']), sum(case['phases'])
        pixels = sum(case['batches']) * case['hw'][0] * case['hw'][1]
        near = np.asarray(g64['near'], dtype=np.int64).reshape(epochs, steps)
        share = near.sum(axis=1).max() / pixels
        assert share <= NEAR_CAP, (name, share)
        a64 = np.stack(g64['areas']).reshape(epochs, steps, 3, K)
        area_gap = np.max([np.abs(a64.sum(1) - np.stack(g['areas']).reshape(epochs, steps, 3, K).sum(1)).sum(2) for g in g32s], axis=0)
        assert (area_gap <= 2 * near.sum(axis=1)[:, None]).all(), (name, area_gap, near.sum(axis=1))
        loss_gap = np.max([np.abs(np.asarray(g['loss_avg']) - np.asarray(g64['loss_avg'])) for g in g32s], axis=0)
        off = g64['params'][0][1]
        gaps = [np.max([per_tensor_max(g['params'][p][0] - g64['params'][p][0], off) for g in g32s], axis=0)
                for p in range(len(case['phases']))]
        print('%s: near share %.4f; loss average float32 vs float64 relative %s; area L1 %s against 2*near %s; largest weight difference %s'
              % (name, share, ['%.2e' % (d / abs(r)) for d, r in zip(loss_gap, g64['loss_avg'])], area_gap.tolist(),
                 (2 * near.sum(axis=1)).tolist(), ['%.2e' % g.max() for g in gaps]))
        if case['nid'] is not None:         # conditioning of the NID case (tests/supervised_loop_cases.py)
            assert max(g.max() for g in gaps) <= PARAM_FLOOR, (name, [g.max() for g in gaps])
        # teeth: the two loop mistakes the tests must see, in float64, after the first phase
        groups = np.array([-1 if group_of(n) is None else group_of(n) for n in g64['names']])
        short = dict(case, phases=case['phases'][:1])
        bound = param_bounds(gaps[0])
        for what, loaders in (('first batch applied twice', {0: [0] + list(range(steps))}), ('last batch dropped', {0: list(range(steps - 1))})):
            bad = run_case(short, torch.float64, loaders)
            over = per_tensor_max(bad['params'][0][0] - g64['params'][0][0], off) > bound
            hit = [int(over[groups == k].sum()) for k in (0, 1)]
            print('    %s: %d / %d tensors of the two groups leave the bound' % (what, hit[0], hit[1]))
            assert hit[0] > 0 and hit[1] > 0, (name, what, hit)
        arrays[name + '.areas'] = a64
        arrays[name + '.loss'] = np.asarray(g64['loss'], dtype=np.float64).reshape(epochs, steps)
        arrays[name + '.near'] = near
        arrays[name + '.loss_avg'] = np.asarray(g64['loss_avg'], dtype=np.float64)
        arrays[name + '.iou'] = np.stack(g64['iou'])
        arrays[name + '.loss_gap'] = loss_gap
        arrays[name + '.area_gap'] = area_gap.astype(np.int64)
        for p in range(len(case['phases'])):
            arrays[name + '.params_%d' % p] = g64['params'][p][0].astype(np.float32)
            arrays[name + '.params_gap_%d' % p] = gaps[p].astype(np.float32)
            arrays[name + '.buffers_%d' % p] = g64['buffers'][p][0].astype(np.float32)
        arrays[name + '.params_off'] = off.astype(np.int64)
        arrays[name + '.buffers_off'] = g64['buffers'][0][1].astype(np.int64)
        meta['cases'][name] = {'loss_avg': g64['loss_avg'], 'loss_avg_float32': g32['loss_avg']}
        meta['names'], meta['buffer_names'] = g64['names'], g64['buffer_names']
    path = os.path.join(HERE, 'train_seg_ue_loop.npz')
    np.savez_compressed(path, **arrays)
    print('wrote %s (%.1f KiB)' % (path, os.path.getsize(path) / 1024))
    with open(os.path.join(HERE, 'train_seg_ue_loop.json'), 'w') as f:
        json.dump(meta, f, indent=1, sort_keys=True)


if __name__ == '__main__':
    main()
