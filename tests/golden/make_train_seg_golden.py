#!/usr/bin/env python3
"""Generate tests/golden/train_seg_loop.npz / .json by running the REFERENCE's own train_seg and val_seg
(utilities/train_eval_seg.py:16-162) on the CPU.

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout>:<this repository> python3 tests/golden/make_train_seg_golden.py

Built like tests/golden/make_train_seg_ue_golden.py (whose helpers are imported): `train_seg`, `val_seg` and `AverageMeter` are
AST-extracted at run time and run with the reference's own single-head models (ESPNetv2Segmentation, ESPDNetSegmentation) in
train() / eval() mode, its SegmentationLoss, NIDLoss and MIOU classes and torch.optim.SGD over the model's two learning-rate groups;
the loader is the list of seeded batches of tests/single_head_loop_cases.py.  Only data is written.

Every case runs in float64 with four threads -- the GOLDEN -- and in float32 over FLOAT32_RUNS of tests/supervised_loop_cases.py; the
LARGEST distance of any float32 run from the float64 run is recorded beside the golden per epoch and per tensor.

Per case (npz keys `<case>.<name>`): areas, loss, near, loss_avg, loss_gap, area_gap, params_<p>, params_gap_<p>, buffers_<p>,
params_off, buffers_off as in train_seg_ue_loop.npz, and
    miou           (epochs,) the returned SCALAR (iou[[1, 2, 3]].mean() * 100)
    val            (2,) val_seg's returned (miou, average loss) after the last epoch on the held-out batches;  val_gap (2,) its float32 gap
    val_areas      (3, 4) the held-out batches' summed areas;  val_near  their near-margin pixel count
The json holds both functions' signatures (names, defaults and `str(inspect.signature(...))`) and, per case, the names behind the
offsets.  The generator asserts the near-tie share and that a first batch applied twice and a dropped last batch leave the parameter
bound of the tests in tensors of BOTH learning-rate groups."""
import collections
import inspect
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.golden.make_train_seg_ue_golden import REF, _run_dtype, by_epoch, extract, one_ulp, sample  # noqa: E402,F401
from tests.single_head_loop_cases import NID_GAP_CAP, SINGLE_HEAD_LOOP_CASES, build_model, loop_batches, val_batches  # noqa: E402
from tests.supervised_loop_cases import (CLASS_WEIGHTS, FLOAT32_RUNS, IGNORE_IDX, LR_MULT, MOMENTUM, NEAR_CAP, NEAR_MARGIN, NUM_CLASSES,  # noqa: E402
                                         WEIGHT_DECAY, group_of, param_bounds, per_tensor_max)
from tests.train_loop_cases import reference_areas  # noqa: E402

from model.segmentation.espdnet import ESPDNetSegmentation  # noqa: E402
from model.segmentation.espnetv2 import ESPNetv2Segmentation  # noqa: E402
from loss_fns.segmentation_loss import NIDLoss, PixelwiseKLD, SegmentationLoss  # noqa: E402
from utilities.metrics.segmentation_miou import MIOU  # noqa: E402

K = NUM_CLASSES - 1


def run_case(case, dtype, loaders=None, threads=4, perturb=None, with_val=True):
    torch.set_num_threads(threads)
    ns = {'torch': torch, 'np': np, 'PixelwiseKLD': PixelwiseKLD, 'print_log_message': lambda *a: None, 'print_info_message': lambda *a: None,
          'print': lambda *a: None, 'OrderedDict': collections.OrderedDict, 'time': time, 'gather': None}
    extract(os.path.join(REF, 'utilities/utils.py'), (), ns, classes=('AverageMeter',))
    extract(os.path.join(REF, 'utilities/train_eval_seg.py'), {'train_seg', 'val_seg'}, ns)
    log = {'loss': [], 'areas': [], 'near': [], 'meters': 0}

    class RecMeter(ns['AverageMeter']):        # `losses` is the first meter train_seg builds (:18)
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
    m = build_model(case, ESPNetv2Segmentation, ESPDNetSegmentation).to(dtype)
    crit = SegmentationLoss(n_classes=NUM_CLASSES, device='cpu', ignore_idx=IGNORE_IDX, class_weights=torch.tensor(CLASS_WEIGHTS, dtype=dtype))
    base = [((x if perturb is None else one_ulp(x, 17 * perturb + i)).to(dtype), y) for i, (x, y) in enumerate(loop_batches(case))]
    out = {'loss_avg': [], 'miou': [], 'params': [], 'buffers': [], 'steps': []}
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
                # device='cuda' selects the branch the script runs (:41-51, `.mean()` of the loss); no tensor is moved by it here
                miou, avg = ns['train_seg'](m, loader, opt, crit, NUM_CLASSES, epoch, device='cuda', add_criterion=add,
                                            weight=case['nid'] if case['nid'] is not None else 1.0)
                out['loss_avg'].append(float(avg))
                out['miou'].append(float(miou))
                out['steps'].append(len(loader))
                epoch += 1
            out['params'].append(sample(list(m.parameters())))
            out['buffers'].append(sample([b for b in m.buffers() if b.is_floating_point()]))
        out['loss'], out['areas'], out['near'] = list(log['loss']), list(log['areas']), list(log['near'])
        if with_val:
            n0 = len(log['areas'])
            log['meters'] = 1                                        # (val_seg's meters are not the training loss meter)
            held = [(x.to(dtype), y) for x, y in val_batches(case)]
            vm, vl = ns['val_seg'](m, held, criterion=crit, num_classes=NUM_CLASSES, device='cuda')
            out['val'] = np.array([float(vm), float(vl)])
            out['val_areas'] = np.sum(log['areas'][n0:], axis=0)
            out['val_near'] = int(np.sum(log['near'][n0:]))
    out['names'] = [n for n, _ in m.named_parameters()]
    out['buffer_names'] = [n for n, b in m.named_buffers() if b.is_floating_point()]
    return out


def signature_record(fn):
    sig = inspect.signature(fn)
    return {'names': list(sig.parameters), 'text': str(sig),
            'defaults': {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}}


def main():
    arrays, meta = {}, {'cases': {}}
    ns = extract(os.path.join(REF, 'utilities/train_eval_seg.py'), {'train_seg', 'val_seg'}, {})
    meta['signatures'] = {'train_seg': signature_record(ns['train_seg']), 'val_seg': signature_record(ns['val_seg'])}
    only = sys.argv[1:]
    for name, case in sorted(SINGLE_HEAD_LOOP_CASES.items()):
        if only and name not in only:
            continue
        g64 = run_case(case, torch.float64)
        g32s = [run_case(case, torch.float32, threads=nt, perturb=k) for nt, k in FLOAT32_RUNS]
        steps, epochs = len(case['batches']), sum(case['phases'])
        pixels = sum(case['batches']) * case['hw'][0] * case['hw'][1]
        near = np.asarray(g64['near'], dtype=np.int64).reshape(epochs, steps)
        share = near.sum(axis=1).max() / pixels
        assert share <= NEAR_CAP, (name, share)
        a64 = np.stack(g64['areas']).reshape(epochs, steps, 3, K)
        area_gap = np.max([np.abs(a64.sum(1) - np.stack(g['areas']).reshape(epochs, steps, 3, K).sum(1)).sum(2) for g in g32s], axis=0)
        assert (area_gap <= 2 * near.sum(axis=1)[:, None]).all(), (name, area_gap, near.sum(axis=1))
        loss_gap = np.max([np.abs(np.asarray(g['loss_avg']) - np.asarray(g64['loss_avg'])) for g in g32s], axis=0)
        val_gap = np.max([np.abs(g['val'] - g64['val']) for g in g32s], axis=0)
        assert all(np.abs(g['val_areas'] - g64['val_areas']).sum(1).max() <= 2 * g64['val_near'] for g in g32s), name
        off = g64['params'][0][1]
        gaps = [np.max([per_tensor_max(g['params'][p][0] - g64['params'][p][0], off) for g in g32s], axis=0)
                for p in range(len(case['phases']))]
        print('%s: near share %.4f; loss average float32 vs float64 relative %s; area L1 %s against 2*near %s; largest weight difference %s; '
              'val %s gap %s' % (name, share, ['%.2e' % (d / abs(r)) for d, r in zip(loss_gap, g64['loss_avg'])], area_gap.tolist(),
                                 (2 * near.sum(axis=1)).tolist(), ['%.2e' % g.max() for g in gaps], g64['val'].tolist(), val_gap.tolist()))
        if case['nid'] is not None:         # conditioning of the NID case (tests/single_head_loop_cases.py)
            assert max(g.max() for g in gaps) <= NID_GAP_CAP, (name, [g.max() for g in gaps])
        # teeth: the two loop mistakes the tests must see, in float64, after the first phase
        groups = np.array([-1 if group_of(n) is None else group_of(n) for n in g64['names']])
        short = dict(case, phases=case['phases'][:1])
        bound = param_bounds(gaps[0])
        for what, loaders in (('first batch applied twice', {0: [0] + list(range(steps))}), ('last batch dropped', {0: list(range(steps - 1))})):
            bad = run_case(short, torch.float64, loaders, with_val=False)
            over = per_tensor_max(bad['params'][0][0] - g64['params'][0][0], off) > bound
            hit = [int(over[groups == k].sum()) for k in (0, 1)]
            print('    %s: %d / %d tensors of the two groups leave the bound' % (what, hit[0], hit[1]))
            assert hit[0] > 0 and hit[1] > 0, (name, what, hit)
        arrays[name + '.areas'] = a64
        arrays[name + '.loss'] = np.asarray(g64['loss'], dtype=np.float64).reshape(epochs, steps)
        arrays[name + '.near'] = near
        arrays[name + '.loss_avg'] = np.asarray(g64['loss_avg'], dtype=np.float64)
        arrays[name + '.miou'] = np.asarray(g64['miou'], dtype=np.float64)
        arrays[name + '.loss_gap'] = loss_gap
        arrays[name + '.area_gap'] = area_gap.astype(np.int64)
        arrays[name + '.val'] = g64['val']
        arrays[name + '.val_gap'] = val_gap
        arrays[name + '.val_areas'] = g64['val_areas'].astype(np.int64)
        arrays[name + '.val_near'] = np.asarray(g64['val_near'], dtype=np.int64)
        for p in range(len(case['phases'])):
            arrays[name + '.params_%d' % p] = g64['params'][p][0].astype(np.float32)
            arrays[name + '.params_gap_%d' % p] = gaps[p].astype(np.float32)
            arrays[name + '.buffers_%d' % p] = g64['buffers'][p][0].astype(np.float32)
        arrays[name + '.params_off'] = off.astype(np.int64)
        arrays[name + '.buffers_off'] = g64['buffers'][0][1].astype(np.int64)
        meta['cases'][name] = {'loss_avg': g64['loss_avg'], 'names': g64['names'], 'buffer_names': g64['buffer_names']}
    out_dir = os.environ.get('MSPL_GOLDEN_OUT', HERE)
    suffix = ('.' + '.'.join(only)) if only else ''
    path = os.path.join(out_dir, 'train_seg_loop%s.npz' % suffix)
    np.savez_compressed(path, **arrays)
    print('wrote %s (%.1f KiB)' % (path, os.path.getsize(path) / 1024))
    with open(os.path.join(out_dir, 'train_seg_loop%s.json' % suffix), 'w') as f:
        json.dump(meta, f, indent=1, sort_keys=True)


if __name__ == '__main__':
    main()
