#!/usr/bin/env python3
"""The matrix modes of the ASPP heads ('fp32', 'bf16x3', 'bf16x6') next to each other at the BASELINE configs[4] shape
(16 x 2048 x 32 x 64, 20 classes), all from ONE process with the modes interleaved round by round.

    python tools/aspp_split_probe.py [--out profiles/aspp_split_probe.json] [--n 16] [--rounds 7]

Writes one JSON file:
    conv_3x3_d12      the dilation-12 3x3 convolution alone per mode: ms per call and useful TFLOP/s (2 * N*H*W * Cin * Cout * 9 FLOPs
                      over the time: a product counts once, however many matrix instructions a mode spends on it)
    head              the whole ASPP_Bottleneck(20) under graph replay per mode: ms per batch and images/s
    max_abs_logit_difference_vs_fp32   per split mode, over every logit of that batch
    speedup_vs_fp32   per split mode, for both of the above
Operands are random (seeded randn feature map, synthetic trained-scale weights), never zeros.  Times are device-event times around
--calls back-to-back launches (or graph replays), the median over --rounds rounds; in every round the three modes run one after the
other, so drift of the clock or of the neighbours hits all three alike.  Each mode is warmed up before the first round.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from mspl_amd import aspp, ops  # noqa: E402
from tests.synth import synth_state_dict  # noqa: E402

MODES = ('fp32', 'bf16x3', 'bf16x6')


def window(fn, calls):
    """Device-event time of `calls` back-to-back fn() in ms per call."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def interleaved(fns, calls, rounds):
    """{mode: median ms per call} with the modes taken in turn inside every round; also the per-round figures."""
    for fn in fns.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ts[k].append(window(fn, calls))
    return {k: sorted(v)[len(v) // 2] for k, v in ts.items()}, ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'aspp_split_probe.json'))
    ap.add_argument('--n', type=int, default=16)
    ap.add_argument('--h', type=int, default=32)
    ap.add_argument('--w', type=int, default=64)
    ap.add_argument('--classes', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--calls', type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('aspp_split_probe: needs the GPU (a CPU run measures nothing)')
    dev = 'cuda'
    N, H, W, Cin = a.n, a.h, a.w, 2048
    torch.manual_seed(0)
    x = torch.randn(N, Cin, H, W, device=dev)
    heads = {}
    for mode in MODES:
        m = aspp.ASPP_Bottleneck(num_classes=a.classes)
        m.load_state_dict(synth_state_dict(m.state_dict(), 0))
        m.matrix_mode = mode
        heads[mode] = m.to(dev).eval()
    res = {'shape': [N, Cin, H, W], 'classes': a.classes, 'device': torch.cuda.get_device_name(0),
           'rounds': a.rounds, 'calls_per_window': a.calls, 'modes': list(MODES)}

    with torch.no_grad():
        # the d = 12 dilated 3x3 alone
        conv = heads['fp32'].conv_3x3_2
        wp = ops.pack_dense_weight(conv.weight)
        ws = {2: ops.pack_dense_weight_split(conv.weight, 2), 3: ops.pack_dense_weight_split(conv.weight, 3)}
        out = torch.empty(N, 256, H, W, device=dev)
        fns = {'fp32': lambda: ops.dense_conv(x, wp, 3, 12, out=(out, 0)),
               'bf16x3': lambda: ops.dense_conv_split(x, ws[2], 3, 12, out=(out, 0)),
               'bf16x6': lambda: ops.dense_conv_split(x, ws[3], 3, 12, out=(out, 0))}
        med, per_round = interleaved(fns, a.calls, a.rounds)
        flops = 2.0 * N * H * W * Cin * 256 * 9
        res['conv_3x3_d12'] = {k: {'ms': med[k], 'useful_tflops': flops / (med[k] * 1e-3) / 1e12, 'ms_per_round': per_round[k]} for k in MODES}
        res['conv_3x3_d12']['flops'] = flops

        # the whole head under graph replay
        graphs, outs = {}, {}
        for mode in MODES:
            for _ in range(2):
                heads[mode](x)                              # packs, epilogue vectors, code objects: outside the capture
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                outs[mode] = heads[mode](x)
            graphs[mode] = g
        med, per_round = interleaved({k: graphs[k].replay for k in MODES}, a.calls, a.rounds)
        res['head'] = {k: {'ms': med[k], 'images_per_s': N / (med[k] * 1e-3), 'ms_per_round': per_round[k]} for k in MODES}
        torch.cuda.synchronize()
        res['max_abs_logit_difference_vs_fp32'] = {k: float((outs[k] - outs['fp32']).abs().max()) for k in MODES[1:]}
        res['max_abs_logit_fp32'] = float(outs['fp32'].abs().max())
    res['speedup_vs_fp32'] = {k: {'conv_3x3_d12': res['conv_3x3_d12']['fp32']['ms'] / res['conv_3x3_d12'][k]['ms'],
                                  'head': res['head']['fp32']['ms'] / res['head'][k]['ms']} for k in MODES[1:]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, indent=1, sort_keys=True))


if __name__ == '__main__':
    main()
