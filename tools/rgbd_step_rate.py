#!/usr/bin/env python3
"""What the RGB-D path costs and what the one-launch fusion gate and the graphed steps buy, from ONE interleaved run: batch 16,
256x480, ESPDNet-UE s = 2.0 with 5 classes (trainable fusion gates).  Every pair is timed A, B, A, B, ... in the same process and
reported as the median of its rounds, so both sides see the same clocks.  Prints one JSON line (and writes it to --out):

  gate_levels        per gate level (C, H, W): models.FusionGate as one launch / one node against MSPL_FUSION_GATE=0 (two conv1x1
                     launches + the blend kernel; cat + conv when training), in us.  inference_us: device time -- 20 calls captured
                     into one graph, replayed between two device events (no host dispatch in the figure).  training_fwd_bwd_us:
                     host wall clock of eager forward + backward between synchronizes (it INCLUDES Python / ctypes dispatch)
  uest_step          the RGB-D uest step: GraphedTrainStep with 1 and 2 lanes against the restated body (eager forward, loss,
                     backward, torch.optim.Adam), ms per step
  supervised_step    the RGB-D supervised iteration: GraphedSupervisedStep against the restated body with torch.optim.SGD, ms

    python tools/rgbd_step_rate.py [--rounds 5] [--out profiles/rgbd_step_rate.json]

--gate-only LEVEL launches the one-launch gate of level 1..4 five times and nothing else of interest: the process to put under a
counters-only profiler run (its own run: no tracing beside the counters) for the HBM bytes of the launch.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCH, H, W, CLASSES = 16, 256, 480, 5
LEVELS = [(32, H // 2, W // 2), (128, H // 4, W // 4), (256, H // 8, W // 8), (512, H // 16, W // 16)]


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=None)
    ap.add_argument('--gate-only', type=int, default=0)
    a = ap.parse_args()
    import torch
    from mspl_amd import layers, losses, models, supervised, training
    from tests.synth import synth_state_dict
    assert torch.cuda.is_available(), 'needs the GPU'
    dev = 'cuda'
    fence = torch.cuda.synchronize

    def timed(fn, iters):
        fn()
        fence()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        fence()
        return (time.perf_counter() - t0) / iters

    def ab(fa, fb, iters):
        """Median seconds of fa and fb over interleaved rounds."""
        ta, tb = [], []
        for _ in range(a.rounds):
            ta.append(timed(fa, iters))
            tb.append(timed(fb, iters))
        return median(ta), median(tb)

    def switched(on, fn):
        def run():
            prev = layers._FUSED_FUSION_GATE
            layers._FUSED_FUSION_GATE = on
            try:
                return fn()
            finally:
                layers._FUSED_FUSION_GATE = prev
        return run

    def graph_timed(fn, calls=20):
        """Seconds per call of fn on the device: `calls` of them in one captured graph, replayed between two events."""
        fn()
        fence()
        graph = torch.cuda.CUDAGraph()
        with layers.graph_capture(graph):
            for _ in range(calls):
                fn()
        graph.replay()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        graph.replay()
        e1.record()
        fence()
        return e0.elapsed_time(e1) * 1e-3 / calls

    if a.gate_only:
        C, h, w = LEVELS[a.gate_only - 1]
        gate = models.FusionGate(nchannel=C).to(dev)
        rgb, dep = torch.randn((BATCH, C, h, w), device=dev), torch.randn((BATCH, C, h, w), device=dev)
        with torch.no_grad():
            for _ in range(5):
                gate(rgb, dep)
        fence()
        print(json.dumps({'gate_only': a.gate_only, 'C': C, 'H': h, 'W': w, 'launches': 5, 'minimal_traffic_bytes': 3 * BATCH * C * h * w * 4}))
        return

    out = {'tool': 'rgbd_step_rate', 'batch': BATCH, 'size': [H, W], 'classes': CLASSES, 'rounds': a.rounds, 'gate_levels': []}
    g = torch.Generator().manual_seed(3)
    for C, h, w in LEVELS:
        gate = models.FusionGate(nchannel=C).to(dev)
        rgb = torch.randn((BATCH, C, h, w), generator=g).to(dev)
        dep = torch.randn((BATCH, C, h, w), generator=g).to(dev)
        gy = torch.randn((BATCH, C, h, w), generator=g).to(dev)

        def infer():
            with torch.no_grad():
                return gate(rgb, dep)

        def train():
            r, d = rgb.detach().requires_grad_(True), dep.detach().requires_grad_(True)
            gate.conv_1x1.conv.weight.grad = None
            gate(r, d).backward(gy)
        i1s, i0s = [], []
        for _ in range(a.rounds):
            i1s.append(graph_timed(switched(True, infer)))
            i0s.append(graph_timed(switched(False, infer)))
        i1, i0 = median(i1s), median(i0s)
        t1, t0 = ab(switched(True, train), switched(False, train), 10)
        n = BATCH * C * h * w * 4
        out['gate_levels'].append({'C': C, 'H': h, 'W': w, 'inference_us': {'one_launch': round(i1 * 1e6, 1), 'three_launches': round(i0 * 1e6, 1)},
                                   'training_fwd_bwd_us': {'one_node': round(t1 * 1e6, 1), 'cat_conv_blend': round(t0 * 1e6, 1)},
                                   'minimal_traffic_bytes': 3 * n, 'one_launch_effective_GBps': round(3 * n / i1 / 1e9, 1)})

    def model():
        m = models.ESPDNetwithUncertaintyEstimation(argparse.Namespace(s=2.0, channels=3, num_classes=1000), classes=CLASSES,
                                                    dataset='greenhouse', trainable_fusion=True, fix_pyr_plane_proj=True)
        m.load_state_dict(synth_state_dict(m.state_dict(), 9))
        return m.to(dev)
    x = torch.randn((BATCH, 3, H, W), generator=g).to(dev)
    xd = torch.randn((BATCH, 1, H, W), generator=g).to(dev)
    y = torch.randint(0, CLASSES, (BATCH, H, W), generator=g).to(dev)
    cw = torch.ones(CLASSES)

    # ---- the uest step
    crit = losses.UncertaintyWeightedSegmentationLoss(CLASSES, class_weights=cw, ignore_idx=4, device=dev)
    kld = losses.PixelwiseKLD()
    steps = {}
    for lanes in (1, 2):
        steps[lanes] = training.GraphedTrainStep(model().eval(), x, y, cw, ignore_idx=4, lanes=lanes, depth=xd)
    mr = model().eval()
    adam = torch.optim.Adam(mr.parameters(), lr=5e-4, weight_decay=5e-4)

    def restated_uest():
        adam.zero_grad()
        pred, aux = mr(x, xd)
        k = kld(pred, aux)
        (crit(pred + 0.5 * aux, y, k) * 20 + k.mean()).backward()
        adam.step()
        layers.bump_param_epoch()
    r = {}
    for lanes in (1, 2):
        tg, tr = ab(lambda: steps[lanes](x, y, xd), restated_uest, 5)
        r['graphed_lanes%d_ms' % lanes], r['restated_ms_beside_lanes%d' % lanes] = round(tg * 1e3, 3), round(tr * 1e3, 3)
    r['lanes_settled'] = getattr(steps[2], 'lane_overlap', None)
    out['uest_step'] = r
    del steps, mr, adam

    # ---- the supervised iteration
    ms = model()
    ms.train()
    sl = losses.SegmentationLoss(n_classes=CLASSES, device=dev, ignore_idx=4, class_weights=cw)
    gs = supervised.GraphedSupervisedStep(ms, x, y, sl, depth=xd)
    mr = model()
    mr.train()
    sgd = torch.optim.SGD(supervised.segmentation_param_groups(mr, 0.009, 10.0, use_depth=True), 0.009, momentum=0.9, weight_decay=4e-5)

    def restated_sup():
        main, aux = mr(x, xd)
        loss = supervised.flood(sl(main + 0.5 * aux, y).mean())
        sgd.zero_grad()
        loss.backward()
        sgd.step()
        layers.bump_param_epoch()
    tg, tr = ab(lambda: gs(x, y, xd), restated_sup, 5)
    out['supervised_step'] = {'graphed_ms': round(tg * 1e3, 3), 'restated_ms': round(tr * 1e3, 3)}
    out['rgbd_label_pass_chain'] = 'not built: the chain differs from the block walk in the summation order of the next projection'
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
