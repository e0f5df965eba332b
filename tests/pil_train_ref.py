"""TEST INFRASTRUCTURE ONLY -- numpy restatement of the train transforms (transforms/segmentation/data_transforms.py:15-136,191-212)
and the cases of tests/golden/train_transforms.npz (written by tests/golden/make_golden_train_transforms.py from the reference's own
classes run with Pillow).

Restated: Pillow's Resample.c for BILINEAR and LANCZOS (precompute_coeffs + normalize_coeffs_8bpc, horizontal pass first, uint8
between the passes, a pass whose size does not change skipped, an unchanged size a copy), NEAREST (oracle.imageio), torchvision's
Pad (ImageOps.expand) + crop, the mirror, to_tensor / normalize (oracle.imageio).
"""
import math

import numpy as np

from oracle import imageio as oio

PRECISION_BITS = 32 - 8 - 2
LANCZOS, BILINEAR = 1, 2          # Pillow's Image.LANCZOS / Image.BILINEAR numbers (and MSPL_FILTER_*)

# name -> (source h, w, crop size (W, H), scale or None, crop, ignore_idx, normalise, with_depth, random seed, image seed)
TRAIN_CASES = {
    'greenhouse_rgbd_norm': (360, 480, (480, 256), (0.5, 2.0), False, 255, True, True, 11, 500),
    'greenhouse_rgbd_tensorize_odd': (61, 47, (40, 24), (0.5, 2.0), False, 255, False, True, 12, 510),
    'camvid_crop': (360, 480, (480, 288), (0.5, 2.0), True, 12, True, False, 13, 520),
    'camvid_crop_small_pad': (29, 37, (48, 40), (0.5, 2.0), True, 4, False, False, 14, 530),
    'cityscapes_crop': (128, 256, (192, 96), (0.5, 2.0), True, 255, True, False, 15, 540),
    'greenhouse_rgb_crop_pad': (47, 61, (64, 48), None, True, 255, True, False, 16, 550),
    'crop_with_depth': (45, 58, (50, 40), (0.5, 2.0), True, 255, True, True, 17, 560),
}
GOLDEN_N = 8


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    if -3.0 <= x < 3.0:
        return _sinc(x) * _sinc(x / 3)
    return 0.0


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def precompute_coeffs(in_size, out_size, filt):
    """Resample.c precompute_coeffs + normalize_coeffs_8bpc over the full box.  Returns (bounds (out,2) int32, kk (out,ksize) int32)."""
    fn, support0 = (_lanczos, 3.0) if filt == LANCZOS else (_bilinear, 1.0)
    scale = filterscale = float(in_size) / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = support0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize), np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = int(center - support + 0.5)
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        xmax -= xmin
        w = [fn((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        for x in range(xmax):
            v = w[x] / ww if ww != 0.0 else w[x]
            kk[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return bounds, kk


def _resample_axis0(img, out_size, filt):
    bounds, kk = precompute_coeffs(img.shape[0], out_size, filt)
    src = img.astype(np.int64)
    out = np.empty((out_size,) + img.shape[1:], np.uint8)
    for i in range(out_size):
        a, n = bounds[i]
        acc = np.full(img.shape[1:], 1 << (PRECISION_BITS - 1), np.int64)
        for j in range(n):
            acc += src[a + j] * int(kk[i, j])
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return out


def resize_u8(img, size, filt):
    """PIL `Image.resize(size, filt)` of an (H,W) or (H,W,C) uint8 image, size = (W, H)."""
    w_out, h_out = size
    img = np.ascontiguousarray(img)
    if img.shape[0] == h_out and img.shape[1] == w_out:
        return img.copy()
    if img.shape[1] != w_out:
        img = np.swapaxes(_resample_axis0(np.swapaxes(img, 0, 1), w_out, filt), 0, 1)
    if img.shape[0] != h_out:
        img = _resample_axis0(img, h_out, filt)
    return np.ascontiguousarray(img)


def pad_crop(img, pad_w, pad_h, i, j, size, fill):
    """torchvision Pad(padding=(pad_w, pad_h), fill) then F.crop(img, i, j, h, w)."""
    w, h = size
    pad = [(pad_h, pad_h), (pad_w, pad_w)] + [(0, 0)] * (img.ndim - 2)
    p = np.pad(img, pad, mode='constant', constant_values=fill)
    return np.ascontiguousarray(p[i:i + h, j:j + w])


def train_transform(rgb, label, depth, d, size, crop, ignore_idx, normalise):
    """One image through RandomScale? -> RandomCrop | Resize -> RandomFlip -> Normalize | Tensorize with the draws d
    (sw, sh, pad_w, pad_h, i, j, flip).  Returns (rgb fp32 (3,H,W), label int64 (H,W) | None, depth fp32 (1,H,W) | None)."""
    sw, sh, pad_w, pad_h, i, j, flip = [int(v) for v in d]
    rgb = resize_u8(rgb, (sw, sh), LANCZOS)
    label = None if label is None else oio.resize_nearest_u8(label, (sw, sh))
    depth = None if depth is None else resize_u8(depth, (sw, sh), BILINEAR)
    if crop:
        rgb = pad_crop(rgb, pad_w, pad_h, i, j, size, 0)
        label = None if label is None else pad_crop(label, pad_w, pad_h, i, j, size, ignore_idx)
        depth = None if depth is None else pad_crop(depth, pad_w, pad_h, i, j, size, 0)
    else:
        rgb = resize_u8(rgb, size, BILINEAR)
        label = None if label is None else oio.resize_nearest_u8(label, size)
        depth = None if depth is None else resize_u8(depth, size, BILINEAR)
    if flip:
        rgb = rgb[:, ::-1]
        label = None if label is None else label[:, ::-1]
        depth = None if depth is None else depth[:, ::-1]
    t = oio.to_tensor(np.ascontiguousarray(rgb))
    if normalise:
        t = oio.normalize(t)
    return (t, None if label is None else np.ascontiguousarray(label).astype(np.int64),
            None if depth is None else oio.to_tensor(np.ascontiguousarray(depth)))


def case_images(name, n):
    """The n input images of a case (image k = tests.synth.synth_image_u8(h, w, image_seed + k))."""
    from tests.synth import synth_image_u8
    hs, ws = TRAIN_CASES[name][:2]
    return [synth_image_u8(hs, ws, TRAIN_CASES[name][9] + k) for k in range(n)]
