#!/usr/bin/env python3
"""Generate tests/golden/train_loop.npz / .json by running the REFERENCE's own train() (uest_seg_multi_os.py:958-1089) on the CPU.

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout>:<this repository> python3 tests/golden/make_train_loop_golden.py

`train`, `lr_poly`, `adjust_learning_rate` (the script cannot be imported: argparse at import time) and `AverageMeter` are
AST-extracted at run time and run with the reference's own model, loss and MIOU classes and torch.optim.Adam; the visualiser and the
writer are stubs, the loader is the list of seeded batches of tests/train_loop_cases.py.  Only data is written.

Per case (keys `<case>.<name>`):
    records (json)     [[tag, value, index], ...] of every writer.add_scalar call, in order, and the returned indices
    areas              (epochs, steps, 3, 4) int64: [inter | pred | mask] of MIOU(4) per step
    loss               (epochs, steps) float64: the value given to losses.update per step
    near               (epochs, steps) int64: pixels whose top-2 margin of the reference's main head is below NEAR_MARGIN
    params_<p>         the strided sample (tests.synth.grad_sample_index) of EVERY parameter after the last step of phase p
    params_off         offsets of the tensors inside a sample
The generator also runs the first phase in float64 and asserts that its own float32 run stays inside the bounds the tests use.
"""
import argparse
import ast
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.synth import assert_weights_close_after_adam, grad_sample_index, synth_state_dict  # noqa: E402
from tests.train_loop_cases import (CLASS_WEIGHTS, IGNORE_IDX, LR, NEAR_CAP, NEAR_MARGIN, TOT_ITER, TRAIN_LOOP_CASES, WEIGHT_DECAY,  # noqa: E402
                                    WRITER_IDX0, loop_args, loop_batches, reference_areas)

# reference imports (torch-only modules)
from model.segmentation.espdnet_ue import ESPDNetwithUncertaintyEstimation  # noqa: E402
from loss_fns.segmentation_loss import PixelwiseKLD, SegmentationLoss, UncertaintyWeightedSegmentationLoss  # noqa: E402
from utilities.metrics.segmentation_miou import MIOU  # noqa: E402
import utilities.metrics.segmentation_miou as _miou_mod  # noqa: E402

REF = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(_miou_mod.__file__))))
torch.set_num_threads(8)


def extract(path, names, ns, classes=()):
    tree = ast.parse(open(path).read())
    for node in tree.body:
        if (isinstance(node, ast.FunctionDef) and node.name in names) or (isinstance(node, ast.ClassDef) and node.name in classes):
            exec(compile(ast.Module([node], []), path, 'exec'), ns)
    return ns


class Quiet(object):                           # tqdm(total=...) as a context manager and tqdm(iterable)
    def __init__(self, it=None, total=None):
        self.it = it

    def __iter__(self):
        return iter(self.it)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


class Writer(object):
    def __init__(self):
        self.records = []

    def add_scalar(self, tag, value, idx):
        self.records.append([tag, float(value), int(idx)])


def sample(model):
    parts = [p.detach().reshape(-1)[grad_sample_index(p.numel())].double() for p in model.parameters()]
    off = np.cumsum([0] + [len(t) for t in parts])
    return torch.cat(parts).numpy(), off


def run_case(case, dtype):
    ns = {'torch': torch, 'np': np, 'tqdm': Quiet, 'PixelwiseKLD': PixelwiseKLD}
    extract(os.path.join(REF, 'utilities/utils.py'), (), ns, classes=('AverageMeter',))
    extract(os.path.join(REF, 'uest_seg_multi_os.py'), {'train', 'lr_poly', 'adjust_learning_rate'}, ns)
    log = {'loss': [], 'areas': [], 'near': [], 'meters': 0}

    class RecMeter(ns['AverageMeter']):        # `losses` is the first meter train() builds (:964)
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

    ns.update(AverageMeter=RecMeter, MIOU=RecMIOU, in_training_visualization_img=lambda *a, **k: None)
    args = loop_args(case)
    ns['args'] = args
    m = ESPDNetwithUncertaintyEstimation(argparse.Namespace(s=2.0, channels=3, num_classes=1000), classes=5, dataset='greenhouse',
                                         fix_pyr_plane_proj=True)
    m.load_state_dict(synth_state_dict(m.state_dict(), case['sd_seed']))
    m = m.to(dtype).eval()
    cw = torch.tensor(CLASS_WEIGHTS, dtype=dtype)
    if case['use_uncertainty']:
        crit = UncertaintyWeightedSegmentationLoss(5, class_weights=cw, ignore_idx=IGNORE_IDX, device='cpu')
    else:
        crit = SegmentationLoss(n_classes=5, device='cpu', ignore_idx=IGNORE_IDX, class_weights=cw)
    loader = [(x.to(dtype), y) for x, y in loop_batches(case)]
    writer = Writer()
    idx = WRITER_IDX0
    out = {'returned': [], 'params': []}
    epoch = 0
    for n_epochs in case['phases']:
        opt = torch.optim.Adam(m.parameters(), lr=LR, weight_decay=WEIGHT_DECAY)
        for _ in range(n_epochs):
            log['meters'] = 0
            idx = ns['train'](loader, m, crit, 'cpu', None, opt, TOT_ITER, 0, epoch, args, None, None, None, idx, None, writer, None)
            out['returned'].append(int(idx))
            epoch += 1
        out['params'].append(sample(m))
    steps = len(loader)
    out['records'] = writer.records
    out['loss'] = np.asarray(log['loss'], dtype=np.float64).reshape(epoch, steps)
    out['areas'] = np.stack(log['areas']).reshape(epoch, steps, 3, 4)
    out['near'] = np.asarray(log['near'], dtype=np.int64).reshape(epoch, steps)
    return out


def main():
    arrays, meta = {}, {}
    for name, case in sorted(TRAIN_LOOP_CASES.items()):
        g = run_case(case, torch.float32)
        steps = len(case['batches'])
        pixels = sum(case['batches']) * case['hw'][0] * case['hw'][1]
        share = g['near'].sum(axis=1).max() / pixels
        assert share <= NEAR_CAP, (name, share)
        # this float32 run against the same loop in float64: inside the bounds the tests use against it
        short = dict(case, phases=case['phases'][:1])
        g64 = run_case(short, torch.float64)
        n1 = case['phases'][0]
        rec32 = [r for r in g['records'] if r[0] == 'uest/train/loss'][:n1]
        rec64 = [r for r in g64['records'] if r[0] == 'uest/train/loss']
        rel = max(abs(a[1] - b[1]) / abs(b[1]) for a, b in zip(rec32, rec64))
        assert rel <= 2e-5, (name, rel)
        for e in range(n1):
            for h in range(3):
                l1 = np.abs(g['areas'][e].sum(0)[h] - g64['areas'][e].sum(0)[h]).sum()
                assert l1 <= 2 * g['near'][e].sum(), (name, e, h, l1)
        assert_weights_close_after_adam(g['params'][0][0], g64['params'][0][0], LR, n1 * steps)
        dmax = float(np.abs(g['params'][0][0] - g64['params'][0][0]).max())
        print('%s: near share %.4f, loss avg float32 vs float64 %.2e relative, largest weight difference %.2e' % (name, share, rel, dmax))
        arrays[name + '.areas'] = g['areas']
        arrays[name + '.loss'] = g['loss']
        arrays[name + '.near'] = g['near']
        for p, (vals, off) in enumerate(g['params']):
            arrays[name + '.params_%d' % p] = vals.astype(np.float32)
        arrays[name + '.params_off'] = g['params'][0][1].astype(np.int64)
        meta[name] = {'records': g['records'], 'returned': g['returned']}
    path = os.path.join(HERE, 'train_loop.npz')
    np.savez_compressed(path, **arrays)
    print('wrote %s (%.1f KiB)' % (path, os.path.getsize(path) / 1024))
    with open(os.path.join(HERE, 'train_loop.json'), 'w') as f:
        json.dump(meta, f, indent=1, sort_keys=True)


if __name__ == '__main__':
    main()
