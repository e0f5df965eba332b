"""The single-head cross entropy at head resolution (autograd.ce_head_meters, fused=True) against the form built from the existing
kernels (fused=False: bilinear + ce_meters + weighted_ce_bwd + bilinear_bwd), forward + backward with meters, as graph replays on
resident inputs at 16 x {20, 5} x 256 x 480; then one graphed train_seg iteration of ESPNetv2 s = 0.5 with each form.  The two forms
alternate, REPS windows each; prints one JSON line per measurement (median and spread of the windows, microseconds per replay).

    python tools/ce_head_probe.py [--iters 50] [--reps 7] [--skip-step]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from mspl_amd import autograd as ag, losses, models, supervised  # noqa: E402


def captured(fn):
    """fn() once eagerly on a side stream, then captured; returns the graph."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def window(replay, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def alternate(forms, iters, reps):
    times = {k: [] for k in forms}
    for _ in range(reps):
        for k, replay in forms.items():
            times[k].append(window(replay, iters))
    return {k: {'median_us': round(statistics.median(v), 2), 'min_us': round(min(v), 2), 'max_us': round(max(v), 2)} for k, v in times.items()}


def loss_node(C, iters, reps):
    N, H, W = 16, 256, 480
    g = torch.Generator().manual_seed(C)
    # (the head is not a leaf: autograd then runs nothing on another stream than the capture's)
    base = (torch.randn(N, C, H // 2, W // 2, generator=g) * 3).cuda().requires_grad_(True)
    t = torch.randint(0, C, (N, H, W), generator=g)
    t[torch.rand(N, H, W, generator=g) < 0.05] = 255
    t = t.cuda()
    cw = torch.linspace(0.5, 2.0, C).cuda()
    meters = supervised.SupervisedMeters(C - 1, 'cuda')
    keep = {}

    def run(fused):
        head = base.view_as(base)                # (a view: no kernel)
        loss = ag.ce_head_meters(head, t, cw, 255, meters, fused=fused)
        keep[fused] = torch.autograd.grad(loss, head)[0]
    forms = {'head': captured(lambda: run(True)).replay, 'upsampled': captured(lambda: run(False)).replay}
    print(json.dumps({'what': 'ce loss + meters fwd+bwd', 'shape': [N, C, H, W], **alternate(forms, iters, reps)}), flush=True)


def train_step(iters, reps):
    N, C, H, W = 16, 20, 256, 480
    a = argparse.Namespace(s=0.5, channels=3, num_classes=1000)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(N, 3, H, W, generator=g).cuda()
    t = torch.randint(0, C, (N, H, W), generator=g)
    t[torch.rand(N, H, W, generator=g) < 0.05] = 255
    t = t.cuda()
    forms = {}
    for name, fused in (('head', True), ('upsampled', False)):
        torch.manual_seed(0)
        m = models.ESPNetv2Segmentation(a, classes=C, dataset='city').cuda().train()
        crit = losses.SegmentationLoss(n_classes=C, device='cuda', ignore_idx=255, class_weights=torch.linspace(0.5, 2.0, C))
        gs = supervised.GraphedSupervisedStep(m, x, t, crit, lr=1e-4, meters=supervised.SupervisedMeters(C - 1, 'cuda'), heads=1,
                                              ce_at_head=fused)
        forms[name] = (lambda gs=gs: gs(x, t))
    print(json.dumps({'what': 'graphed train_seg iteration, ESPNetv2 s=0.5', 'shape': [N, C, H, W], **alternate(forms, iters, reps)}),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--skip-step', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('ce_head_probe: needs the GPU')
    for C in (20, 5):
        loss_node(C, args.iters, args.reps)
    if not args.skip_step:
        train_step(max(5, args.iters // 5), args.reps)


if __name__ == '__main__':
    main()
