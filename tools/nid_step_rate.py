#!/usr/bin/env python3
"""What does the NID regulariser (train(..., add_loss=NIDLoss), `--use-nid true`) cost per training step, and what do the kernels at
head resolution (csrc/nid_heads.hip) buy?  One process, one interleaved run: batch 16, 256x480, ESPDNet-UE s=2.0 with 5 classes,
NIDLoss(image_bin=32, label_bin=5).  Prints one JSON line (and writes it to --out):

  graphed_ms            the graphed step WITHOUT the additional loss, on the loop's default two lanes and on one lane
  graphed_nid_ms        the graphed step WITH it (one lane: the NID histogram couples the images of a batch)
  restated_nid_ms       the restated reference body with it (eager autograd, the caller's torch.optim.Adam, NIDLoss.forward on the
                        up-sampled head): what --use-nid cost before the graphed step took it
  ratio_restated_over_graphed_nid
  kernels               device-event time per call, 20 back-to-back calls, of the fused chain (mspl_nid_heads_fwd + mspl_nid_finalize,
                        mspl_nid_heads_bwd) against the three-step chain (mspl_bilinear_fwd + mspl_nid_hist_fwd, mspl_nid_hist_bwd +
                        mspl_bilinear_bwd), on a head without near-ties (the backward skips every pixel) and on one where 15 % of
                        the head pixels tie two adjacent classes within 4e-3

Every step time is the median of `--rounds` windows of `--steps` steps between fences; the variants alternate inside a round.

    python tools/nid_step_rate.py [--out profiles/nid_step_rate.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCH, H, W, CLASSES, K = 16, 256, 480, 5, 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    from mspl_amd import losses, models, script, training
    from mspl_amd._native import check, lib
    from mspl_amd.ops import _p, _stream
    from tests.synth import synth_nid_inputs, synth_state_dict
    assert torch.cuda.is_available(), 'needs the GPU'
    dev = 'cuda'
    fence = torch.cuda.synchronize

    def model():
        m = models.ESPDNetwithUncertaintyEstimation(argparse.Namespace(s=2.0, channels=3, num_classes=1000), classes=CLASSES,
                                                    dataset='greenhouse', fix_pyr_plane_proj=True)
        m.load_state_dict(synth_state_dict(m.state_dict(), 9))
        return m.to(dev).eval()
    g = torch.Generator().manual_seed(7)
    x0 = torch.randn((BATCH, 3, H, W), generator=g).to(dev)
    y0 = torch.randint(0, CLASSES, (BATCH, H, W), generator=g).to(dev)
    cw = torch.ones(CLASSES)
    nid = losses.NIDLoss(image_bin=K, label_bin=CLASSES)
    steps = {'graphed_lanes2': training.GraphedTrainStep(model(), x0, y0, cw, ignore_idx=4, lanes=2),
             'graphed_lanes1': training.GraphedTrainStep(model(), x0, y0, cw, ignore_idx=4, lanes=1),
             'graphed_nid': training.GraphedTrainStep(model(), x0, y0, cw, ignore_idx=4, lanes=2, add_loss=nid)}
    assert steps['graphed_nid'].lanes == 1

    # the restated body, as script.train runs it when the fast path is refused
    m_r = model()
    crit = losses.UncertaintyWeightedSegmentationLoss(CLASSES, class_weights=cw, ignore_idx=4, device=dev)
    opt = torch.optim.Adam(m_r.parameters(), lr=5e-4, weight_decay=5e-4)
    args = argparse.Namespace(model='espdnetue', use_depth=False, use_uncertainty=True, learning_rate=5e-4, power=0.9)
    meters = training.TrainMeters(4, dev)
    loader = [(x0, y0)] * a.steps

    def restated():
        script._train_restated(loader, m_r, crit, dev, opt, 1e6, args, nid, meters)

    def window(fn):
        fence()
        t0 = time.perf_counter()
        fn()
        fence()
        return (time.perf_counter() - t0) / a.steps * 1e3

    def graphed(s):
        def run():
            for _ in range(a.steps):
                s(x0, y0)
        return run
    variants = dict((k, graphed(s)) for k, s in steps.items())
    variants['restated_nid'] = restated
    for fn in variants.values():                 # warm-up of every variant
        fn()
    samples = dict((k, []) for k in variants)
    for _ in range(a.rounds):
        for k, fn in variants.items():
            samples[k].append(window(fn))
    med = dict((k, sorted(v)[len(v) // 2]) for k, v in samples.items())

    # kernel chains
    Hm, Wm = H // 2, W // 2
    Cl, E = min(CLASSES, K), K * min(CLASSES, K) + K + min(CLASSES, K)
    cam, lab = synth_nid_inputs((BATCH, 3, Hm, Wm), CLASSES, 3)              # (camera unused at this size; logits with 15 % near-ties)
    heads = {'no_ties': (torch.randn((BATCH, CLASSES, Hm, Wm), generator=g) * 3).to(dev), 'ties_15_percent': lab.to(dev).contiguous()}
    cam = torch.rand((BATCH, 3, H, W), generator=g).to(dev)
    ws = torch.empty(lib.mspl_nid_heads_workspace_floats(CLASSES, H, W, K), device=dev)
    ws3 = torch.empty(lib.mspl_nid_workspace_floats(CLASSES, H, W, K), device=dev)
    out, loss2, gj, gpl = (torch.empty(n, device=dev) for n in (E, 1, K * Cl, Cl))
    full, gfull = torch.empty((BATCH, CLASSES, H, W), device=dev), torch.empty((BATCH, CLASSES, H, W), device=dev)
    norm = float(BATCH * H * W)

    def timed(fn, reps=20):
        fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        fence()
        return e0.elapsed_time(e1) / reps * 1e3

    kernels = {}
    for tag, main in heads.items():
        gmain = torch.zeros_like(main)
        chains = {
            'fused_fwd_us': lambda: (check(lib.mspl_nid_heads_fwd(_p(cam), _p(main), BATCH, CLASSES, Hm, Wm, H, W, K, 0.005, 0.001, _p(ws), _p(out), _stream())),
                                     check(lib.mspl_nid_finalize(_p(out), K, CLASSES, CLASSES, norm, _p(loss2), _p(gj), _p(gpl), _stream()))),
            'three_step_fwd_us': lambda: (check(lib.mspl_bilinear_fwd(_p(main), BATCH, CLASSES, Hm, Wm, H, W, 1, None, _p(full), _stream())),
                                          check(lib.mspl_nid_hist_fwd(_p(cam), _p(full), BATCH, CLASSES, H, W, K, 0.005, 0.001, _p(ws3), _p(out), _stream()))),
            'fused_bwd_us': lambda: (gmain.zero_(),
                                     check(lib.mspl_nid_heads_bwd(_p(main), BATCH, CLASSES, Hm, Wm, H, W, K, 0.001, _p(ws), _p(gj), _p(gpl), None, _p(gmain), _stream()))),
            'three_step_bwd_us': lambda: (check(lib.mspl_nid_hist_bwd(_p(cam), _p(full), BATCH, CLASSES, H, W, K, 0.005, 0.001, _p(gj), _p(gpl), _p(gfull), _stream())),
                                          check(lib.mspl_bilinear_bwd(_p(gfull), BATCH, CLASSES, Hm, Wm, H, W, _p(gmain), _stream()))),
        }
        # forward chains first (they fill ws / full / gj / gpl for the backward chains); three alternating rounds, the median
        got = dict((k, []) for k in chains)
        for _ in range(3):
            for k, fn in chains.items():
                got[k].append(timed(fn))
        kernels[tag] = dict((k, round(sorted(v)[1], 1)) for k, v in got.items())
        kernels[tag]['nonzero_head_gradient_share'] = round(float((gmain != 0).float().mean()), 5)

    res = {'tool': 'nid_step_rate', 'batch': BATCH, 'size': [H, W], 'classes': CLASSES, 'image_bin': K, 'steps_per_window': a.steps,
           'rounds': a.rounds,
           'graphed_ms': {'lanes2': round(med['graphed_lanes2'], 3), 'lanes1': round(med['graphed_lanes1'], 3)},
           'graphed_nid_ms': round(med['graphed_nid'], 3), 'graphed_nid_lanes': steps['graphed_nid'].lanes,
           'restated_nid_ms': round(med['restated_nid'], 3),
           'ratio_restated_over_graphed_nid': round(med['restated_nid'] / med['graphed_nid'], 2),
           'nid_cost_ms_over_graphed_lanes1': round(med['graphed_nid'] - med['graphed_lanes1'], 3),
           'min_max_ms': dict((k, [round(min(v), 3), round(max(v), 3)]) for k, v in samples.items()),
           'kernels': kernels,
           'note': 'one machine, one process; step times move by several per cent from box to box and run to run, the ratio less'}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
