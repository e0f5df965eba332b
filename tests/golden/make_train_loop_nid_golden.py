#!/usr/bin/env python3
"""Generate tests/golden/train_loop_nid.npz / .json by running the REFERENCE's own train() (uest_seg_multi_os.py:958-1089) with
add_loss=NIDLoss(image_bin=32, label_bin=5) on the CPU, on the cases of tests/train_loop_nid_cases.py.

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout>:<this repository> python3 tests/golden/make_train_loop_nid_golden.py
    ... make_train_loop_nid_golden.py --search loop_nid_32x48 100 140        # print, per in_seed, whether its conditions hold

The machinery is make_train_loop_golden.py's (AST-extracted train(), recording meters and MIOU, stub writer and visualiser) with
NIDLoss's hard-coded `.to('cuda')` / `.float()` shimmed as in make_train_seg_ue_golden.py.  Every case runs in float64 with four
threads -- the GOLDEN -- and in float32 over FLOAT32_RUNS (thread counts, one-ulp perturbations of the images).  Per case (keys
`<case>.<name>`):
    records (json)     [[tag, value, index], ...] of every writer.add_scalar call, in order, and the returned indices (float64 run)
    areas, near        (epochs, steps, 3, 4) / (epochs, steps) int64 as in train_loop.npz
    loss, loss2        (epochs, steps) float64: the value given to losses.update and the additional loss per step
    gap_loss_avg, gap_nid_avg   (epochs,) largest |float32 - float64| of the two written averages over the float32 runs
    gap_loss, gap_loss2         (epochs, steps) the same per step
    params_<p>, params_off      the strided sample of every parameter after the last step of phase p (float64 run, stored as float32)
Asserted (the conditioning of tests/train_loop_nid_cases.py): both averages of every float32 run within LOSS_RTOL / LOSS_ATOL of the
float64 run, assert_weights_close_after_adam(float32, float64) per phase, area L1 within twice the near-pixel count, near share at
most NEAR_CAP.  Only data is written.
"""
import argparse
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.synth import assert_weights_close_after_adam, synth_state_dict  # noqa: E402
from tests.train_loop_nid_cases import (CLASS_WEIGHTS, FLOAT32_RUNS, IGNORE_IDX, LOSS_ATOL, LOSS_RTOL, LR, NEAR_CAP, NEAR_MARGIN,  # noqa: E402
                                        NID_IMAGE_BIN, NID_LABEL_BIN, TOT_ITER, TRAIN_LOOP_NID_CASES, WEIGHT_DECAY, WRITER_IDX0, loop_args,
                                        loop_batches, reference_areas)
from tests.golden.make_train_loop_golden import REF, Quiet, Writer, extract, sample  # noqa: E402
from tests.golden.make_train_seg_ue_golden import _run_dtype, one_ulp  # noqa: E402

from model.segmentation.espdnet_ue import ESPDNetwithUncertaintyEstimation  # noqa: E402
from loss_fns.segmentation_loss import NIDLoss, PixelwiseKLD, UncertaintyWeightedSegmentationLoss  # noqa: E402
from utilities.metrics.segmentation_miou import MIOU  # noqa: E402


def run_case(case, dtype, threads=4, perturb=None):
    torch.set_num_threads(threads)
    ns = {'torch': torch, 'np': np, 'tqdm': Quiet, 'PixelwiseKLD': PixelwiseKLD}
    extract(os.path.join(REF, 'utilities/utils.py'), (), ns, classes=('AverageMeter',))
    extract(os.path.join(REF, 'uest_seg_multi_os.py'), {'train', 'lr_poly', 'adjust_learning_rate'}, ns)
    log = {'loss': [], 'loss2': [], 'areas': [], 'near': [], 'meters': 0}

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

    class RecNID(NIDLoss):
        def forward(self, camera, label):
            out = super().forward(camera, label)
            log['loss2'].append(float(out.detach()))
            return out

    ns.update(AverageMeter=RecMeter, MIOU=RecMIOU, in_training_visualization_img=lambda *a, **k: None)
    args = loop_args(case)
    ns['args'] = args
    m = ESPDNetwithUncertaintyEstimation(argparse.Namespace(s=2.0, channels=3, num_classes=1000), classes=5, dataset='greenhouse',
                                         fix_pyr_plane_proj=True)
    m.load_state_dict(synth_state_dict(m.state_dict(), case['sd_seed']))
    m = m.to(dtype).eval()
    crit = UncertaintyWeightedSegmentationLoss(5, class_weights=torch.tensor(CLASS_WEIGHTS, dtype=dtype), ignore_idx=IGNORE_IDX, device='cpu')
    loader = [((x if perturb is None else one_ulp(x, 17 * perturb + i)).to(dtype), y) for i, (x, y) in enumerate(loop_batches(case))]
    writer = Writer()
    idx = WRITER_IDX0
    out = {'returned': [], 'params': []}
    epoch = 0
    with _run_dtype(dtype), contextlib.redirect_stdout(io.StringIO()):
        nid = RecNID(image_bin=NID_IMAGE_BIN, label_bin=NID_LABEL_BIN)
        for n_epochs in case['phases']:
            opt = torch.optim.Adam(m.parameters(), lr=LR, weight_decay=WEIGHT_DECAY)
            for _ in range(n_epochs):
                log['meters'] = 0
                idx = ns['train'](loader, m, crit, 'cpu', None, opt, TOT_ITER, 0, epoch, args, None, None, None, idx, None, writer, nid)
                out['returned'].append(int(idx))
                epoch += 1
            out['params'].append(sample(m))
    steps = len(loader)
    out['records'] = writer.records
    out['loss'] = np.asarray(log['loss'], dtype=np.float64).reshape(epoch, steps)
    out['loss2'] = np.asarray(log['loss2'], dtype=np.float64).reshape(epoch, steps)
    out['areas'] = np.stack(log['areas']).reshape(epoch, steps, 3, 4)
    out['near'] = np.asarray(log['near'], dtype=np.int64).reshape(epoch, steps)
    return out


def tagged(records, tag):
    return np.array([r[1] for r in records if r[0] == tag], dtype=np.float64)


def conditions(case, g64, g32s):
    """The gaps of the float32 runs from the float64 run, and the list of conditions that do NOT hold (empty: the seed is good)."""
    steps = len(case['batches'])
    pixels = sum(case['batches']) * case['hw'][0] * case['hw'][1]
    bad = []
    share = float(g64['near'].sum(axis=1).max()) / pixels
    if share > NEAR_CAP:
        bad.append('near share %.4f' % share)
    gaps = {}
    for key, tag in (('gap_loss_avg', 'uest/train/loss'), ('gap_nid_avg', 'uest/train/nid_loss')):
        ref = tagged(g64['records'], tag)
        gaps[key] = np.max([np.abs(tagged(g['records'], tag) - ref) for g in g32s], axis=0)
        if (gaps[key] > LOSS_RTOL * np.abs(ref) + LOSS_ATOL).any():
            bad.append('%s float32 gap %s' % (tag, gaps[key]))
    gaps['gap_loss'] = np.max([np.abs(g['loss'] - g64['loss']) for g in g32s], axis=0)
    gaps['gap_loss2'] = np.max([np.abs(g['loss2'] - g64['loss2']) for g in g32s], axis=0)
    done = 0
    for p, n_epochs in enumerate(case['phases']):
        done += n_epochs * steps
        for g in g32s:
            try:
                assert_weights_close_after_adam(g['params'][p][0], g64['params'][p][0], LR, done)
            except AssertionError as e:
                bad.append('weights after phase %d: %s' % (p, e))
                break
    for g in g32s:
        for e in range(len(g64['near'])):
            l1 = np.abs(g['areas'][e].sum(0) - g64['areas'][e].sum(0)).sum(1)
            if (l1 > 2 * g64['near'][e].sum()).any():
                bad.append('areas epoch %d L1 %s against 2 x %d' % (e, l1.tolist(), g64['near'][e].sum()))
    return gaps, bad, share


def evaluate(case):
    g64 = run_case(case, torch.float64)
    g32s = [run_case(case, torch.float32, threads=nt, perturb=k) for nt, k in FLOAT32_RUNS]
    gaps, bad, share = conditions(case, g64, g32s)
    return g64, gaps, bad, share


def main():
    if len(sys.argv) > 1 and sys.argv[1] == '--search':
        name, lo, hi = sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
        for seed in range(lo, hi):
            _, gaps, bad, share = evaluate(dict(TRAIN_LOOP_NID_CASES[name], in_seed=seed))
            print('%s in_seed %d: %s  (loss avg gap %.2e, nid avg gap %.2e, near share %.4f)'
                  % (name, seed, 'GOOD' if not bad else 'no: ' + '; '.join(bad)[:200], gaps['gap_loss_avg'].max(), gaps['gap_nid_avg'].max(), share), flush=True)
        return
    arrays, meta = {}, {}
    for name, case in sorted(TRAIN_LOOP_NID_CASES.items()):
        g64, gaps, bad, share = evaluate(case)
        assert not bad, (name, bad)
        print('%s: near share %.4f; largest float32 gaps: loss average %.2e, nid average %.2e, per-step loss %.2e, loss2 %.2e'
              % (name, share, gaps['gap_loss_avg'].max(), gaps['gap_nid_avg'].max(), gaps['gap_loss'].max(), gaps['gap_loss2'].max()))
        for k in ('areas', 'near', 'loss', 'loss2'):
            arrays['%s.%s' % (name, k)] = g64[k]
        for k, v in gaps.items():
            arrays['%s.%s' % (name, k)] = v
        for p, (vals, off) in enumerate(g64['params']):
            arrays[name + '.params_%d' % p] = vals.astype(np.float32)
        arrays[name + '.params_off'] = g64['params'][0][1].astype(np.int64)
        meta[name] = {'records': g64['records'], 'returned': g64['returned']}
    path = os.path.join(HERE, 'train_loop_nid.npz')
    np.savez_compressed(path, **arrays)
    print('wrote %s (%.1f KiB)' % (path, os.path.getsize(path) / 1024))
    with open(os.path.join(HERE, 'train_loop_nid.json'), 'w') as f:
        json.dump(meta, f, indent=1, sort_keys=True)


if __name__ == '__main__':
    main()
