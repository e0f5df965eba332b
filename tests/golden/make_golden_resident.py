#!/usr/bin/env python3
"""Generate tests/golden/resident_transforms.npz by running the REFERENCE's own train transform classes with Pillow on CPU, on frames
whose label images have ANOTHER size than the frame (the pseudo-labels of a self-training round: 256x480 maps for 360x480 frames).

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=. python3 tests/golden/make_golden_resident.py <reference root>

The AST extraction of RandomScale / RandomCrop / Resize / RandomFlip / Normalize / Tensorize / Compose, the torchvision shims and the
pipeline order are those of make_golden_train_transforms.py (imported from it).  As the dataset does before its transforms
(greenhouse.py:248-251), label value 0 becomes 1 first.  Per case (tests/resident_cases.py): random.seed(seed), then GOLDEN_N images one
after the other.  Stored: the draws per image (sw, sh, pad_w, pad_h, i, j, flip), the next random.random(), SHA-256 per output tensor
per image, strided samples of image 0.
"""
import os
import random as _random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

from make_golden_train_transforms import REF, SizeProbe, namespace, pipeline, sha  # noqa: E402
from tests.resident_cases import GOLDEN_N, RESIDENT_CASES, case_images, remap_lut  # noqa: E402


def main():
    from PIL import Image
    assert os.path.isfile(os.path.join(REF, 'transforms/segmentation/data_transforms.py')), 'pass the reference root'
    lut = remap_lut()
    out = {}
    for name, case in sorted(RESIDENT_CASES.items()):
        hs, ws, hl, wl, size, scale, crop, ign, norm, with_depth, seed, _ = case
        ns, rec = namespace()
        probe = SizeProbe()
        comp = pipeline(ns, probe, size, scale, crop, ign, norm)
        _random.seed(seed)
        draws, shas = [], {'rgb': [], 'label': [], 'depth': []}
        for k, (rgb, label, depth) in enumerate(case_images(name, GOLDEN_N)):
            assert label.shape == (hl, wl) and rgb.shape == (hs, ws, 3)
            start = len(rec.log)
            args = [Image.fromarray(rgb), Image.fromarray(lut[label])] + ([Image.fromarray(depth)] if with_depth else [])
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
            assert tuple(res[1].shape) == (th, tw), (name, k, tuple(res[1].shape))
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
    path = os.path.join(HERE, 'resident_transforms.npz')
    np.savez_compressed(path, **out)
    print('wrote %s (%.1f KiB)' % (path, os.path.getsize(path) / 1024))


if __name__ == '__main__':
    main()
