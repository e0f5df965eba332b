#!/usr/bin/env python3
"""ASPP_Bottleneck in train() at the BASELINE configs[4] shape (16 x 2048 x 32 x 64, 20 classes): what a training step costs next to
the inference forward, and what the backward kernels of K13 cost next to their forward counterparts FROM THE SAME RUN.

    python tools/aspp_train_probe.py [--out profiles/aspp_train_probe.json] [--n 16] [--iters 10]

Writes one JSON file:
    forward_no_grad_ms        the head in eval() under torch.no_grad() (unchanged code: the yardstick)
    train_step_ms             forward + backward in train(), feature map frozen (requires_grad=False) / trainable
    eager_step_ms             the same step by a plain nn.Conv2d / nn.BatchNorm2d restatement of nn_layers/aspp.py:54-99 under
                              PyTorch-ROCm eager on the same device
    kernels                   per dense convolution: forward, weight-gradient and (for the four spatial branches together, and for
                              conv_1x1_3) data-gradient call times, their ratio to the forward counterpart, and the share of the
                              157.3 TFLOP/s fp32 matrix peak at the convolution's nominal 2 * N*H*W * Cin * Cout * taps FLOPs;
                              wgrad_ms_by_split: the weight gradient with the pixel axis forced into 1 .. 32 ranges (the library's
                              own choice is wgrad_split)
Times are device-event times of single calls (each a launch of 0.1 .. 10 ms, or two for a split weight gradient), median of --iters
after two warm-up calls.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from torch import nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from mspl_amd import aspp, ops  # noqa: E402
from tests.synth import synth_state_dict  # noqa: E402

PEAK = 157.3e12


class EagerBottleneck(nn.Module):
    """nn_layers/aspp.py:54-99 restated with plain torch modules (the reference itself is not a dependency of this tool)."""

    def __init__(self, cin, classes):
        super().__init__()
        self.conv_1x1_1, self.bn_conv_1x1_1 = nn.Conv2d(cin, 256, 1), nn.BatchNorm2d(256)
        for i, d in enumerate((6, 12, 18)):
            setattr(self, 'conv_3x3_%d' % (i + 1), nn.Conv2d(cin, 256, 3, 1, d, d))
            setattr(self, 'bn_conv_3x3_%d' % (i + 1), nn.BatchNorm2d(256))
        self.conv_1x1_2, self.bn_conv_1x1_2 = nn.Conv2d(cin, 256, 1), nn.BatchNorm2d(256)
        self.conv_1x1_3, self.bn_conv_1x1_3 = nn.Conv2d(1280, 256, 1), nn.BatchNorm2d(256)
        self.conv_1x1_4 = nn.Conv2d(256, classes, 1)

    def forward(self, x):
        h, w = x.shape[2:]
        outs = [F.relu(self.bn_conv_1x1_1(self.conv_1x1_1(x)))]
        for i in (1, 2, 3):
            outs.append(F.relu(getattr(self, 'bn_conv_3x3_%d' % i)(getattr(self, 'conv_3x3_%d' % i)(x))))
        img = F.relu(self.bn_conv_1x1_2(self.conv_1x1_2(F.adaptive_avg_pool2d(x, 1))))
        outs.append(F.interpolate(img, size=(h, w), mode='bilinear'))
        return self.conv_1x1_4(F.relu(self.bn_conv_1x1_3(self.conv_1x1_3(torch.cat(outs, 1)))))


def timed(fn, iters):
    """Median device-event time of fn() in ms."""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'aspp_train_probe.json'))
    ap.add_argument('--n', type=int, default=16)
    ap.add_argument('--h', type=int, default=32)
    ap.add_argument('--w', type=int, default=64)
    ap.add_argument('--classes', type=int, default=20)
    ap.add_argument('--iters', type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('aspp_train_probe: needs the GPU (a CPU run measures nothing)')
    dev = 'cuda'
    N, H, W, Cin = a.n, a.h, a.w, 2048
    m = aspp.ASPP_Bottleneck(num_classes=a.classes)
    sd = synth_state_dict(m.state_dict(), 0)
    m.load_state_dict(sd)
    m = m.to(dev)
    x = torch.randn(N, Cin, H, W, device=dev)
    res = {'shape': [N, Cin, H, W], 'classes': a.classes, 'device': torch.cuda.get_device_name(0), 'peak_fp32_matrix_tflops': PEAK / 1e12}

    m.eval()
    with torch.no_grad():
        res['forward_no_grad_ms'] = timed(lambda: m(x), a.iters)

    def step(mod, inp):
        for p in mod.parameters():
            p.grad = None
        inp.grad = None
        mod(inp).sum().backward()

    m.train()
    res['train_step_ms'] = {'feature_map_frozen': timed(lambda: step(m, x), a.iters),
                            'feature_map_trainable': timed(lambda: step(m, x.clone().requires_grad_(True)), a.iters)}
    e = EagerBottleneck(Cin, a.classes)
    e.load_state_dict(sd)
    e = e.to(dev).train()
    res['eager_step_ms'] = {'feature_map_frozen': timed(lambda: step(e, x), a.iters),
                            'feature_map_trainable': timed(lambda: step(e, x.clone().requires_grad_(True)), a.iters)}

    P = N * H * W
    gz = torch.randn(N, 256, H, W, device=dev)
    cat = torch.randn(N, 1280, H, W, device=dev)
    kern = {}
    fwd_spatial = 0.0
    with torch.no_grad():
        for name, src in [('conv_1x1_1', x), ('conv_3x3_1', x), ('conv_3x3_2', x), ('conv_3x3_3', x), ('conv_1x1_3', cat)]:
            conv = getattr(m, name)
            k, dil = conv.kernel_size[0], conv.dilation[0]
            wp = ops.pack_dense_weight(conv.weight)
            flops = 2.0 * P * conv.in_channels * 256 * k * k
            fwd = timed(lambda: ops.dense_conv(src, wp, k, dil), a.iters)
            wg = timed(lambda: ops.dense_conv_wgrad(gz, src, k, dil), a.iters)
            kern[name] = {'flops': flops, 'forward_ms': fwd, 'wgrad_ms': wg, 'wgrad_over_forward': wg / fwd,
                          'forward_peak_share': flops / (fwd * 1e-3) / PEAK, 'wgrad_peak_share': flops / (wg * 1e-3) / PEAK,
                          'wgrad_split': int(ops.lib.mspl_dense_conv_wgrad_workspace_bytes(N, conv.in_channels, 256, H, W, k, dil, 0)
                                             // (4 * (k * k * 256 * conv.in_channels + 256)) or 1)}
            kern[name]['wgrad_ms_by_split'] = {str(sp): timed(lambda: ops.dense_conv_wgrad(gz, src, k, dil, split=sp), max(3, a.iters // 2))
                                               for sp in (1, 2, 3, 4, 6, 8, 16, 32)}
            if src is x:
                fwd_spatial += fwd
        convs = [m.conv_1x1_1, m.conv_3x3_1, m.conv_3x3_2, m.conv_3x3_3]
        wts = [ops.pack_dense_weight_dgrad(c.weight) for c in convs]
        ks, dils = [c.kernel_size[0] for c in convs], [c.dilation[0] for c in convs]
        dg = timed(lambda: ops.dense_conv_dgrad([gz] * 4, wts, ks, dils), a.iters)
        flops = 2.0 * P * Cin * 256 * 28
        kern['dgrad_four_branches'] = {'flops': flops, 'dgrad_ms': dg, 'forward_ms_sum_of_four': fwd_spatial, 'dgrad_over_forward': dg / fwd_spatial,
                                       'dgrad_peak_share': flops / (dg * 1e-3) / PEAK}
        wt3 = ops.pack_dense_weight_dgrad(m.conv_1x1_3.weight)
        dg3 = timed(lambda: ops.dense_conv_dgrad([gz], [wt3], [1], [1]), a.iters)
        kern['conv_1x1_3']['dgrad_ms'] = dg3
        kern['conv_1x1_3']['dgrad_over_forward'] = dg3 / kern['conv_1x1_3']['forward_ms']
        kern['conv_1x1_3']['dgrad_peak_share'] = kern['conv_1x1_3']['flops'] / (dg3 * 1e-3) / PEAK
    res['kernels'] = kern
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, indent=1, sort_keys=True))


if __name__ == '__main__':
    main()
