#!/usr/bin/env python3
"""ms per step of the drop-in train() loop (mspl_amd.script.train) against the bare graphed step, in one process.

    python tools/train_epoch_probe.py [--steps 40] [--pairs 5] [--lanes 2]

BASELINE's train shape: 16 x 3 x 256 x 480, ESPDNet-UE s = 2.0, 5 classes.  Two models with the same weights: one is driven by
`script.train` over a list of device-resident batches (one epoch = --steps steps, the meters taken inside the loss kernel, one read
per epoch), the other by bare `GraphedTrainStep` calls with the same lanes.  --pairs alternating (adapter, bare) measurements; the
first epoch of the adapter (capture) is a warm-up outside the timing.  `--kernel-trace-steps N`: only N adapter steps and N bare
steps, nothing timed -- the run to put under a kernel trace, where the METERS instantiation of uw_loss_heads_kernel shows next to the
plain one."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mspl_amd import losses, models, script, training  # noqa: E402
from tests.synth import synth_state_dict  # noqa: E402

CW = [0.0, 6.31, 3.78, 3.18, 7.64]


class Writer(object):
    def add_scalar(self, tag, value, idx):
        pass


def model(dev):
    a = argparse.Namespace(s=2.0, channels=3, num_classes=1000)
    m = models.ESPDNetwithUncertaintyEstimation(a, classes=5, dataset='greenhouse', fix_pyr_plane_proj=True)
    m.load_state_dict(synth_state_dict(m.state_dict(), 9))
    return m.to(dev).eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=40)
    ap.add_argument('--pairs', type=int, default=5)
    ap.add_argument('--lanes', type=int, default=2)
    ap.add_argument('--kernel-trace-steps', type=int, default=0)
    o = ap.parse_args()
    dev = 'cuda:0'
    g = torch.Generator().manual_seed(7)
    x = torch.randn((16, 3, 256, 480), generator=g).to(dev)
    y = torch.randint(0, 5, (16, 256, 480), generator=g).to(dev)
    steps = o.kernel_trace_steps or o.steps
    batches = [(x, y)] * steps
    args = argparse.Namespace(model='espdnetue', use_depth=False, use_uncertainty=True, use_traversable=False, learning_rate=5e-4,
                              power=0.9, train_lanes=o.lanes)
    ma, mb = model(dev), model(dev)
    crit = losses.UncertaintyWeightedSegmentationLoss(5, class_weights=torch.tensor(CW), ignore_idx=4, device=dev)
    opt = torch.optim.Adam(ma.parameters(), lr=5e-4, weight_decay=5e-4)
    bare = training.GraphedTrainStep(mb, x, y, torch.tensor(CW), ignore_idx=4, lanes=o.lanes)

    def adapter():
        return script.train(batches, ma, crit, dev, None, opt, float(5 * steps), 0, 0, args, None, None, None, 0, None, Writer(), None)

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
        print('script.train %.3f ms/step   bare GraphedTrainStep %.3f ms/step' % rows[-1], flush=True)
    a = sorted(r[0] for r in rows)[len(rows) // 2]
    b = sorted(r[1] for r in rows)[len(rows) // 2]
    print('median of %d pairs, %d steps, %d lanes: script.train %.3f ms/step, bare %.3f ms/step (%+.1f %%)'
          % (o.pairs, steps, o.lanes, a, b, (a / b - 1) * 100))


if __name__ == '__main__':
    main()
