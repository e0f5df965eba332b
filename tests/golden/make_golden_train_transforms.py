#!/usr/bin/env python3
"""Generate tests/golden/train_transforms.npz by running the REFERENCE's own train transform classes with Pillow on CPU.

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=. python3 tests/golden/make_golden_train_transforms.py <reference root>

RandomScale, RandomCrop, Resize, RandomFlip, Normalize, Tensorize and Compose are AST-extracted from
transforms/segmentation/data_transforms.py and composed in each dataset's order (greenhouse.py:211-219, camvid.py:95-104,
cityscapes.py:109-117, greenhouse.py:118-125).  torchvision is absent, so the namespace carries shims: Pad -> ImageOps.expand,
F.crop -> Image.crop, F.to_tensor / F.normalize as torchvision computes them; Image.ANTIALIAS (removed in Pillow 10) is its alias
Image.LANCZOS.  Per case: random.seed(seed), then GOLDEN_N images one after the other.  Stored: the draws per image (sw, sh, pad_w,
pad_h, i, j, flip), the next random.random() (how many draws were consumed), SHA-256 per output tensor per image, strided samples of
image 0.
"""
import ast
import hashlib
import os
import random as _random
import sys

import numpy as np
import torch

REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('MSPL_REFERENCE', '')
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.pil_train_ref import GOLDEN_N, TRAIN_CASES, case_images  # noqa: E402


class RecordingRandom(object):
    """The module-level `random` of the extracted classes: the real generator, with every draw logged."""

    def __init__(self):
        self.log = []

    def random(self):
        v = _random.random()
        self.log.append(('random', v))
        return v

    def randint(self, a, b):
        v = _random.randint(a, b)
        self.log.append(('randint', a, b, v))
        return v


def namespace():
    import math
    import numbers
    from PIL import Image, ImageOps
    if not hasattr(Image, 'ANTIALIAS'):
        Image.ANTIALIAS = Image.LANCZOS

    class Pad(object):
        def __init__(self, padding, fill=0, padding_mode='constant'):
            assert padding_mode == 'constant'
            self.padding, self.fill = padding, fill

        def __call__(self, img):
            return ImageOps.expand(img, border=self.padding, fill=self.fill)

    class F(object):
        @staticmethod
        def crop(img, i, j, h, w):
            return img.crop((j, i, j + w, i + h))

        @staticmethod
        def to_tensor(pic):
            a = np.array(pic, np.uint8, copy=True)
            if a.ndim == 2:
                a = a[:, :, None]
            return torch.from_numpy(a).permute(2, 0, 1).contiguous().float().div(255)

        @staticmethod
        def normalize(t, mean, std):
            t = t.clone()
            m = torch.as_tensor(mean, dtype=t.dtype)
            s = torch.as_tensor(std, dtype=t.dtype)
            return t.sub_(m[:, None, None]).div_(s[:, None, None])

    rec = RecordingRandom()
    ns = {'random': rec, 'Image': Image, 'math': math, 'torch': torch, 'np': np, 'numbers': numbers, 'Pad': Pad, 'F': F,
          'MEAN': [0.485, 0.456, 0.406], 'STD': [0.229, 0.224, 0.225]}
    path = os.path.join(REF, 'transforms/segmentation/data_transforms.py')
    for node in ast.parse(open(path).read()).body:
        if isinstance(node, ast.ClassDef) and node.name in ('RandomScale', 'RandomCrop', 'Resize', 'RandomFlip', 'Normalize',
                                                            'Tensorize', 'Compose'):
            exec(compile(ast.Module([node], []), path, 'exec'), ns)
    return ns, rec


class SizeProbe(object):
    """Records the image size between RandomScale and the crop / resize."""

    def __init__(self):
        self.sizes = []

    def __call__(self, rgb, label, depth=None):
        self.sizes.append(rgb.size)
        return (rgb, label, depth) if depth is not None else (rgb, label)


def pipeline(ns, probe, size, scale, crop, ignore_idx, normalise):
    ts = []
    if scale is not None:
        ts.append(ns['RandomScale'](scale=scale))
    ts.append(probe)
    if crop:
        ts.append(ns['RandomCrop'](crop_size=size, ignore_idx=ignore_idx))
        ts.append(ns['Resize'](size=size))                    # camvid.py:100 lists it; the crop is the size, so it is a copy
    else:
        ts.append(ns['Resize'](size=size))
    ts.append(ns['RandomFlip']())
    ts.append(ns['Normalize']() if normalise else ns['Tensorize']())
    return ns['Compose'](ts)


def sha(t):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(t.numpy()).tobytes()).digest(), np.uint8)


def main():
    from PIL import Image
    assert os.path.isfile(os.path.join(REF, 'transforms/segmentation/data_transforms.py')), 'pass the reference root'
    out = {}
    for name, case in sorted(TRAIN_CASES.items()):
        hs, ws, size, scale, crop, ign, norm, with_depth, seed, _ = case
        ns, rec = namespace()
        probe = SizeProbe()
        comp = pipeline(ns, probe, size, scale, crop, ign, norm)
        imgs = case_images(name, GOLDEN_N)
        _random.seed(seed)
        draws, shas = [], {'rgb': [], 'label': [], 'depth': []}
        for k, (rgb, label, depth) in enumerate(imgs):
            start = len(rec.log)
            args = [Image.fromarray(rgb), Image.fromarray(label)] + ([Image.fromarray(depth)] if with_depth else [])
            res = comp(*args)
            log = rec.log[start:]
            sw, sh = probe.sizes[k]
            ints = [e for e in log if e[0] == 'randint']
            tw, th = size
            if ints:
                ph, pw = ints[0][2] + th, ints[1][2] + tw
                i, j = ints[0][3], ints[1][3]
            else:
                ph, pw, i, j = (th, tw, 0, 0) if crop else (sh, sw, 0, 0)
            flip = int(log[-1][0] == 'random' and log[-1][1] < 0.5)
            draws.append((sw, sh, (pw - sw) // 2 if crop else 0, (ph - sh) // 2 if crop else 0, i, j, flip))
            shas['rgb'].append(sha(res[0]))
            shas['label'].append(sha(res[1]))
            if with_depth:
                shas['depth'].append(sha(res[2]))
            if k == 0:
                out[name + '.rgb_s'] = res[0][:, ::23, ::29].numpy()
                out[name + '.label_s'] = res[1][::23, ::29].numpy().astype(np.uint8)
        out[name + '.draws'] = np.array(draws, np.int32)
        out[name + '.next'] = np.array(_random.random(), np.float64)
        for key, v in shas.items():
            if v:
                out['%s.%s_sha' % (name, key)] = np.stack(v)
    path = os.path.join(HERE, 'train_transforms.npz')
    np.savez_compressed(path, **out)
    print('wrote %s (%.1f KiB)' % (path, os.path.getsize(path) / 1024))


if __name__ == '__main__':
    main()
