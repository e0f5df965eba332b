#!/usr/bin/env python3
"""Rate of the device train transforms (mspl_amd.io.TrainPreprocessor) in the Greenhouse RGB-D form: a batch of 16 360x480 frames with
labels and depth, RandomScale (0.5, 2.0) -> Resize (480, 256) -> RandomFlip -> Normalize (greenhouse.py:211-219).  Prints one JSON line:

  device_ms_per_batch   device events around `batches` calls on device-resident frames, fresh draws per batch, after warm-up
  frames_to_tensors     images/s from pinned host uint8 frames: upload + draws + transforms, device synchronised at the end
  pil_1proc / pil_Nproc the host PIL pipeline (Pillow LANCZOS / NEAREST / BILINEAR resize, flip, to_tensor + normalize in numpy)
                        in 1 and N worker processes of this box, images/s (or a note when Pillow is missing)

    python tools/train_transform_rate.py [--batches 200] [--procs 16]
"""
import argparse
import json
import math
import multiprocessing as mp
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZE, SCALE, N, HS, WS = (480, 256), (0.5, 2.0), 16, 360, 480
MEAN = np.array([0.485, 0.456, 0.406], np.float32)[:, None, None]
STD = np.array([0.229, 0.224, 0.225], np.float32)[:, None, None]


def frames(n, seed=0):
    from tests.synth import synth_image_u8
    ims = [synth_image_u8(HS, WS, seed + k) for k in range(n)]
    return [np.stack([im[c] for im in ims]) for c in range(3)]


def pil_worker(args):
    """The reference's per-image train transforms with Pillow, `count` images; returns seconds."""
    count, seed = args
    from PIL import Image
    rgb, lab, dep = frames(1, seed)
    r0, l0, d0 = Image.fromarray(rgb[0]), Image.fromarray(lab[0]), Image.fromarray(dep[0])
    rng = random.Random(seed)
    t0 = time.perf_counter()
    for _ in range(count):
        w, h = r0.size
        s = math.pow(2, math.log(SCALE[0], 2) + rng.random() * (math.log(SCALE[1], 2) - math.log(SCALE[0], 2)))
        ns = (int(round(w * s)), int(round(h * s)))
        r, la, d = r0.resize(ns, Image.LANCZOS), l0.resize(ns, Image.NEAREST), d0.resize(ns, Image.BILINEAR)
        r, la, d = r.resize(SIZE, Image.BILINEAR), la.resize(SIZE, Image.NEAREST), d.resize(SIZE, Image.BILINEAR)
        if rng.random() < 0.5:
            r, la, d = (im.transpose(Image.FLIP_LEFT_RIGHT) for im in (r, la, d))
        t = (np.asarray(r).transpose(2, 0, 1).astype(np.float32) / np.float32(255) - MEAN) / STD
        np.asarray(la).astype(np.int64)
        np.asarray(d)[None].astype(np.float32) / np.float32(255)
    return time.perf_counter() - t0


def pil_rates(procs, count=60):
    try:
        import PIL  # noqa: F401
    except ImportError:
        return {'pil': 'Pillow is not installed on this box: host rate not measured'}
    one = count / pil_worker((count, 1))
    with mp.get_context('spawn').Pool(procs) as pool:
        t0 = time.perf_counter()
        pool.map(pil_worker, [(count, 10 + k) for k in range(procs)])
        many = procs * count / (time.perf_counter() - t0)
    return {'pil_1proc_images_per_s': round(one, 1), 'pil_%dproc_images_per_s' % procs: round(many, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=30)
    ap.add_argument('--procs', type=int, default=16)
    ap.add_argument('--no-pil', action='store_true')
    a = ap.parse_args()
    import torch
    from mspl_amd.io import TrainPreprocessor
    assert torch.cuda.is_available(), 'needs the GPU'
    pre = TrainPreprocessor(size=SIZE, scale=SCALE)
    rgb, lab, dep = [torch.from_numpy(x) for x in frames(N)]
    dev = [t.cuda() for t in (rgb, lab, dep)]
    rng = random.Random(1)
    for _ in range(a.warmup):                   # also builds the tables of the sizes the draws reach
        pre(*dev, params=pre.draw(N, (WS, HS), rng))
    torch.cuda.synchronize()
    # device time: draws and record uploads are host work between the launches; events bracket the whole window
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.batches):
        pre(*dev, params=pre.draw(N, (WS, HS), rng))
    e1.record()
    torch.cuda.synchronize()
    window_ms = e0.elapsed_time(e1) / a.batches
    # frames -> tensors: pinned uint8 frames uploaded every batch
    pinned = [t.pin_memory() for t in (rgb, lab, dep)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.batches):
        pre(*pinned)
    torch.cuda.synchronize()
    f2t = N * a.batches / (time.perf_counter() - t0)
    out = {'tool': 'train_transform_rate', 'batch': N, 'src': [HS, WS], 'size': list(SIZE), 'scale': list(SCALE), 'depth': True,
           'batches': a.batches, 'window_ms_per_batch': round(window_ms, 4),
           'frames_to_tensors_images_per_s': round(f2t, 1), 'upload_bytes_per_batch': int(N * HS * WS * 5),
           'targets': {'kernel_us_per_batch': 60, 'frames_to_tensors_images_per_s': 10000},
           'tables_cached': len(pre._tables)}
    if not a.no_pil:
        out.update(pil_rates(a.procs))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
