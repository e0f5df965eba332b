"""TEST INFRASTRUCTURE ONLY -- the cases of tests/golden/resident_transforms.npz (written by tests/golden/make_golden_resident.py from
the reference's own transform classes run with Pillow): train transforms on frames whose label maps have a size of their own, as
the pseudo-labels of a self-training round have (written at the network's size, 256x480, for 360x480 camera frames).

The restatement of the reference for these cases is tests.pil_train_ref.train_transform, whose RandomScale stage already resizes the
label from its own size (data_transforms.py:78-85).  A pipeline WITHOUT RandomScale hands the label to Resize as it is
(data_transforms.py:191-212: one NEAREST from its own size), which `reference_transform` below restates.
"""
import numpy as np

from oracle import imageio as oio
from tests import pil_train_ref as ref

# name -> (frame h, w, label h, w, size (W, H), scale or None, crop, ignore_idx, normalise, with_depth, random seed, image seed)
RESIDENT_CASES = {
    'uest_round': (360, 480, 256, 480, (480, 256), (0.5, 2.0), False, 255, True, False, 21, 600),
    'odd_two_tiles': (45, 58, 24, 40, (80, 40), (0.5, 2.0), False, 255, True, True, 22, 610),
    'crop_after_scale': (45, 58, 31, 37, (50, 40), (0.5, 2.0), True, 255, True, False, 23, 620),
    'resize_only': (45, 58, 24, 40, (40, 24), None, False, 255, False, False, 24, 630),
}
GOLDEN_N = 8


def remap_lut():
    """greenhouse.py:248-251 (`label_np[label_np==0] = 1`, the dataset without use_traversable) as a 256-entry table."""
    lut = np.arange(256, dtype=np.uint8)
    lut[0] = 1
    return lut


def case_images(name, n):
    """The n inputs of a case: (rgb (hs,ws,3), label (hl,wl) -- NOT remapped --, depth (hs,ws)) uint8; frame k and its label map are
    tests.synth.synth_image_u8 images of their own sizes and seeds."""
    from tests.synth import synth_image_u8
    hs, ws, hl, wl = RESIDENT_CASES[name][:4]
    seed = RESIDENT_CASES[name][11]
    out = []
    for k in range(n):
        rgb, _, depth = synth_image_u8(hs, ws, seed + k)
        out.append((rgb, synth_image_u8(hl, wl, seed + 100 + k)[1], depth))
    return out


def reference_transform(rgb, label, depth, d, size, scale_stage, crop, ignore_idx, normalise):
    """One image with the draws d through the pipeline; label: the (already remapped) map at its own size."""
    if scale_stage:
        return ref.train_transform(rgb, label, depth, d, size, crop, ignore_idx, normalise)
    assert not crop, 'RandomCrop of a label of another size without RandomScale: the reference crops misaligned images'
    t, _, dt = ref.train_transform(rgb, None, depth, d, size, crop, ignore_idx, normalise)
    lt = oio.resize_nearest_u8(label, size)
    if int(d[6]):
        lt = lt[:, ::-1]
    return t, np.ascontiguousarray(lt).astype(np.int64), dt
