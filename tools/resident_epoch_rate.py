#!/usr/bin/env python3
"""Is a self-training epoch from a device-resident target set (mspl_amd.io.FrameStore + ResidentTrainLoader) bound by the train
step or by the loader?  One process, one run, the greenhouse pipeline (RandomScale (0.5, 2.0) -> Resize (480, 256) -> RandomFlip ->
Normalize, label value 0 -> 1 as greenhouse.py:248-251) on 512 synthetic 360x480 frames with 256x480 label maps, batch 16,
ESPDNet-UE s=2.0 with 5 classes on training.GraphedTrainStep.  Prints one JSON line (and writes it to --out):

  step_alone            images/s of the step on static inputs, timed as bench.py's train_step (10 steps between fences, median of 3)
  resident_epoch        images/s of an epoch `for x, y, names, reg in loader: step(x, y)`, fence to fence, resampling tables cached
                        (the epoch before it made the same draws); first_epoch: the epoch that built the tables
  ratio_to_step_alone   resident_epoch / step_alone: 1.0 = the loader costs nothing
  pil_epoch_1core       the same epoch fed by the reference's host pipeline (Pillow, one image at a time, this process's core)
  transform             device-event window and host time per batch of the loader alone (no step), tables cached
  launches_per_batch    what the loader and the hand-over to the step add per batch

    python tools/resident_epoch_rate.py [--frames 512] [--out profiles/resident_epoch.json]
"""
import argparse
import json
import math
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZE, SCALE, BATCH, HS, WS, HL, WL = (480, 256), (0.5, 2.0), 16, 360, 480, 256, 480
MEAN = np.array([0.485, 0.456, 0.406], np.float32)[:, None, None]
STD = np.array([0.229, 0.224, 0.225], np.float32)[:, None, None]


def synthetic_set(n):
    """n frames and label maps; eight distinct synthetic images, repeated (the rates do not depend on the pixels)."""
    from tests.synth import synth_image_u8
    base = [(synth_image_u8(HS, WS, 40 + k)[0], synth_image_u8(HL, WL, 60 + k)[1]) for k in range(8)]
    rgb = np.stack([base[k % 8][0] for k in range(n)])
    lab = np.stack([base[k % 8][1] for k in range(n)])
    lab[lab == 255] = 4                                  # the maps of a label pass hold class ids only
    return rgb, lab


def pil_image(rgb, lab, rng):
    """The reference's per-image train transforms with Pillow (data_transforms.py:67-91, 191-212, 49-66, 28-37)."""
    from PIL import Image
    lab = lab.copy()
    lab[lab == 0] = 1
    r0, l0 = Image.fromarray(rgb), Image.fromarray(lab)
    s = math.pow(2, math.log(SCALE[0], 2) + rng.random() * (math.log(SCALE[1], 2) - math.log(SCALE[0], 2)))
    ns = (int(round(WS * s)), int(round(HS * s)))
    r, la = r0.resize(ns, Image.LANCZOS), l0.resize(ns, Image.NEAREST)
    r, la = r.resize(SIZE, Image.BILINEAR), la.resize(SIZE, Image.NEAREST)
    if rng.random() < 0.5:
        r, la = r.transpose(Image.FLIP_LEFT_RIGHT), la.transpose(Image.FLIP_LEFT_RIGHT)
    return (np.asarray(r).transpose(2, 0, 1).astype(np.float32) / np.float32(255) - MEAN) / STD, np.asarray(la).astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=512)
    ap.add_argument('--lanes', type=int, default=2)
    ap.add_argument('--out', default=None)
    ap.add_argument('--no-pil', action='store_true')
    a = ap.parse_args()
    import torch
    from mspl_amd import models, training
    from mspl_amd.io import FrameStore, ResidentTrainLoader, TrainPreprocessor
    from tests.synth import synth_state_dict
    assert torch.cuda.is_available(), 'needs the GPU'
    dev = 'cuda'
    fence = torch.cuda.synchronize

    m = models.ESPDNetwithUncertaintyEstimation(argparse.Namespace(s=2.0, channels=3, num_classes=1000), classes=5, dataset='greenhouse',
                                                fix_pyr_plane_proj=True)
    m.load_state_dict(synth_state_dict(m.state_dict(), 9))
    m = m.to(dev).eval()
    g = torch.Generator().manual_seed(7)
    x0 = torch.randn((BATCH, 3, SIZE[1], SIZE[0]), generator=g).to(dev)
    y0 = torch.randint(0, 5, (BATCH, SIZE[1], SIZE[0]), generator=g).to(dev)
    step = training.GraphedTrainStep(m, x0, y0, torch.ones(5), ignore_idx=4, lanes=a.lanes)

    def step_alone(iters=10, repeats=3):
        for _ in range(2):
            step(x0, y0)
        samples = []
        for _ in range(repeats):
            fence()
            t0 = time.perf_counter()
            for _ in range(iters):
                step(x0, y0)
            fence()
            samples.append((time.perf_counter() - t0) / iters)
        return sorted(samples)[len(samples) // 2]
    dt_step = step_alone()

    rgb, lab = synthetic_set(a.frames)
    store = FrameStore.from_arrays(rgb, lab)
    lut = np.arange(256, dtype=np.uint8)
    lut[0] = 1
    pre = TrainPreprocessor(size=SIZE, scale=SCALE)
    loader = ResidentTrainLoader(store, pre, BATCH, shuffle=True, drop_last=True, label_lut=lut)
    images = len(loader) * BATCH

    def epoch(seed, with_step=True):
        random.seed(seed)
        fence()
        t0 = time.perf_counter()
        host = 0.0
        it = iter(loader)
        while True:
            h0 = time.perf_counter()
            batch = next(it, None)
            host += time.perf_counter() - h0
            if batch is None:
                break
            if with_step:
                loss = step(batch[0], batch[1])
        fence()
        dt = time.perf_counter() - t0
        if with_step:
            assert bool(torch.isfinite(loss))
        return dt, host
    dt_first, _ = epoch(1)                               # builds the resampling tables of the sizes these draws reach
    samples = [epoch(1) for _ in range(3)]               # the same draws: every table is cached
    dt_epoch, host_epoch = sorted(samples)[1]
    # the loader alone: device-event window per batch (the kernels plus the gaps the host leaves between them) and host time
    epoch(1, with_step=False)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    random.seed(1)
    e0.record()
    t0 = time.perf_counter()
    for _ in loader:
        pass
    host_alone = time.perf_counter() - t0
    e1.record()
    fence()
    window_ms = e0.elapsed_time(e1) / len(loader)
    dt_step_after = step_alone()

    out = {'tool': 'resident_epoch_rate', 'frames': a.frames, 'frame': [HS, WS], 'label': [HL, WL], 'size': list(SIZE), 'scale': list(SCALE),
           'batch': BATCH, 'steps_per_epoch': len(loader), 'micro_batch_lanes': step.lanes, 'store_bytes': store.nbytes(),
           'step_alone_images_per_s': round(BATCH / dt_step, 1), 'step_alone_ms': round(dt_step * 1e3, 3),
           'step_alone_after_images_per_s': round(BATCH / dt_step_after, 1),
           'resident_epoch_images_per_s': round(images / dt_epoch, 1), 'resident_epoch_ms_per_step': round(dt_epoch / len(loader) * 1e3, 3),
           'resident_epoch_min_max_images_per_s': [round(images / max(s[0] for s in samples), 1), round(images / min(s[0] for s in samples), 1)],
           'first_epoch_images_per_s': round(images / dt_first, 1),
           'ratio_to_step_alone': round(dt_step * len(loader) / dt_epoch, 4),
           'loader_host_ms_per_batch_in_epoch': round(host_epoch / len(loader) * 1e3, 3),
           'transform': {'device_window_ms_per_batch': round(window_ms, 4), 'host_ms_per_batch': round(host_alone / len(loader) * 1e3, 3)},
           'launches_per_batch': {'loader': 'one pinned-to-device copy (16 records + 16 slots), RandomScale kernel, output kernel, one fill (reg)',
                                  'hand_over': 'two device copies into the graphed step\'s static inputs (GraphedTrainStep.__call__)'},
           'tables_cached': len(pre._tables)}
    if not a.no_pil:
        try:
            import PIL  # noqa: F401
            rng = random.Random(1)
            order = torch.randperm(a.frames).tolist()
            fence()
            t0 = time.perf_counter()
            for b in range(len(loader)):
                items = [pil_image(rgb[k], lab[k], rng) for k in order[b * BATCH:(b + 1) * BATCH]]
                xb = torch.from_numpy(np.stack([i[0] for i in items])).to(dev, non_blocking=True)
                yb = torch.from_numpy(np.stack([i[1] for i in items])).to(dev, non_blocking=True)
                step(xb, yb)
            fence()
            out['pil_epoch_1core_images_per_s'] = round(images / (time.perf_counter() - t0), 1)
        except ImportError:
            out['pil_epoch_1core_images_per_s'] = 'Pillow is not installed here: not measured'
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
