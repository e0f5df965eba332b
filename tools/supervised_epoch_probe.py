#!/usr/bin/env python3
"""images/s of the drop-in train_seg_ue() loop (mspl_amd.script.train_seg_ue) against the bare graphed supervised step, in one process.

    python tools/supervised_epoch_probe.py [--steps 40] [--pairs 5] [--json FILE]

16 x 3 x 256 x 480, ESPDNet-UE s = 2.0, 5 classes, train() mode.  Two models with the same weights: one is driven by
`script.train_seg_ue` over a list of device-resident batches (one epoch = --steps steps, loss and meters from one read of the
summed logits, one read per epoch, the caller's torch.optim.SGD groups), the other by bare `GraphedSupervisedStep` calls as they
were before the meters existed (criterion + flood, no meters).  --pairs alternating (adapter, bare) measurements; the first epoch
of the adapter (capture) is a warm-up outside the timing.  `--kernel-trace-steps N`: only N adapter steps and N bare steps, nothing
timed -- the run to put under a kernel trace, where ce_meters_kernel + ce_flood_finalize_kernel show next to wce_fwd_kernel."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mspl_amd import losses, models, script, supervised  # noqa: E402
from tests.synth import synth_state_dict  # noqa: E402

CW = [1.45, 6.31, 3.78, 3.18, 0.0]
BATCH = 16


def model(dev):
    a = argparse.Namespace(s=2.0, channels=3, num_classes=1000)
    m = models.ESPDNetwithUncertaintyEstimation(a, classes=5, dataset='greenhouse', fix_pyr_plane_proj=True)
    m.load_state_dict(synth_state_dict(m.state_dict(), 9))
    return m.to(dev).train()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=40)
    ap.add_argument('--pairs', type=int, default=5)
    ap.add_argument('--kernel-trace-steps', type=int, default=0)
    ap.add_argument('--json', default=None)
    o = ap.parse_args()
    dev = 'cuda:0'
    g = torch.Generator().manual_seed(7)
    x = torch.randn((BATCH, 3, 256, 480), generator=g).to(dev)
    y = torch.randint(0, 5, (BATCH, 256, 480), generator=g).to(dev)
    steps = o.kernel_trace_steps or o.steps
    batches = [(x, y)] * steps
    ma, mb = model(dev), model(dev)
    crit = losses.SegmentationLoss(n_classes=5, device=dev, ignore_idx=4, class_weights=torch.tensor(CW))
    opt = torch.optim.SGD(supervised.segmentation_param_groups(ma, 1e-4, 10.0), 1e-4, momentum=0.9, weight_decay=4e-5)
    bare = supervised.GraphedSupervisedStep(mb, x, y, crit, lr=1e-4)

    def adapter():
        return script.train_seg_ue(ma, batches, opt, crit, 5, 0, device=dev)

    def plain():
        for bx, by in batches:
            bare(bx, by)
        torch.cuda.synchronize()

    if o.kernel_trace_steps:
        adapter()
        plain()
        return
    adapter()           # capture + one epoch
    plain()
    rows = []
    for _ in range(o.pairs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        adapter()       # (ends with the epoch's one read, which synchronises)
        t1 = time.perf_counter()
        plain()
        t2 = time.perf_counter()
        rows.append(((t1 - t0) * 1e3 / steps, (t2 - t1) * 1e3 / steps))
        print('script.train_seg_ue %.3f ms/step   bare GraphedSupervisedStep %.3f ms/step' % rows[-1], flush=True)
    a = sorted(r[0] for r in rows)[len(rows) // 2]
    b = sorted(r[1] for r in rows)[len(rows) // 2]
    res = {'shape': [BATCH, 3, 256, 480], 'steps': steps, 'pairs': o.pairs, 'adapter_ms_per_step': round(a, 4), 'bare_ms_per_step': round(b, 4),
           'adapter_images_per_s': round(BATCH * 1e3 / a, 1), 'bare_images_per_s': round(BATCH * 1e3 / b, 1),
           'adapter_over_bare_percent': round((a / b - 1) * 100, 2), 'rows_ms_per_step': [[round(v, 4) for v in r] for r in rows]}
    print('median of %d pairs, %d steps: script.train_seg_ue %.3f ms/step (%.0f images/s), bare %.3f ms/step (%.0f images/s) (%+.1f %%)'
          % (o.pairs, steps, a, res['adapter_images_per_s'], b, res['bare_images_per_s'], res['adapter_over_bare_percent']))
    if o.json:
        with open(o.json, 'w') as f:
            json.dump(res, f, indent=1, sort_keys=True)


if __name__ == '__main__':
    main()
