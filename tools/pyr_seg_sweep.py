#!/usr/bin/env python3
"""Time of one launch of the pyramid streaming kernel alone, tables computed in the kernel against tables from memory, at the label
pass's three map sizes (P = 16, N = 16 and 32).  Device events around 40 launches over rotating buffers, best of 5 rounds.

The rows-per-segment knob is read once per process, and only by the tuning build:
    make -C mspl_amd/csrc TUNING=1
    for s in 0 9 18 24 36 48 72; do MSPL_HIP_LIB=mspl_amd/lib/libmspl_hip_tuning.so MSPL_PYR_SEG=$s python tools/pyr_seg_sweep.py; done
(0: the launcher's own rule.)  One JSON line per (map, N)."""
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mspl_amd import ops  # noqa: E402

DEV = 'cuda'
P, ROT, LAUNCHES, ROUNDS = 16, 4, 40, 5


def sizes_of(h, w):
    return [(max(int(math.ceil(h * s)), 5), max(int(math.ceil(w * s)), 5)) for s in (2.0, 1.5, 1.0, 0.5, 0.1)]


def main():
    knob = int(os.environ.get('MSPL_PYR_SEG', '0'))
    for h, w in ((144, 240), (72, 120), (36, 60)):
        sizes = sizes_of(h, w)
        tab = ops.pyr_stream_tables(h, w, sizes, DEV)
        for N in (16, 32):
            plan = ops.pyrpool_stream_plan((N, P, h, w), sizes)
            g = torch.Generator().manual_seed(1)
            rn = lambda *s: torch.randn(*s, generator=g).to(DEV)                # noqa: E731
            xs = [rn(N, P, h, w) for _ in range(ROT)]
            outs = [torch.empty(N, P, h, w, device=DEV) for _ in range(ROT)]
            stage = [rn(P, 1, 3, 3) / 3 for _ in range(3)] + [None, None]
            down = [None, None, None] + [rn(N, P, *sizes[i]) for i in (3, 4)]
            bs, bh, ba = rn(5 * P).abs() + 0.5, rn(5 * P) * 0.1, rn(5 * P).abs() * 0.3
            mw = rn(P, 5, 3, 3) / 7
            ep = ops.Epi(rn(P).abs() + 0.5, rn(P) * 0.3, rn(P).abs() * 0.3)
            res = {'map': [h, w], 'N': N, 'knob': knob, 'seg_tables': plan['seg'], 'seg_inkernel': plan['seg_inkernel']}
            for name, t in (('inkernel_us', None), ('tables_us', tab)):
                def launches():
                    for k in range(LAUNCHES):
                        ops.pyrpool_fused(xs[k % ROT], sizes, stage, down, bs, bh, ba, mw, ep, out=(outs[k % ROT], 0), tables=t)
                launches()                                                         # eager once, then as one graph: no host time between launches
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    launches()
                best = None
                for _ in range(ROUNDS + 1):                                        # (the first round warms up)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    graph.replay()
                    e1.record()
                    torch.cuda.synchronize()
                    us = e0.elapsed_time(e1) * 1e3 / LAUNCHES
                    best = us if best is None else min(best, us)
                res[name] = round(best, 2)
            print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
