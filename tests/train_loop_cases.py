"""Cases of the drop-in self-training loop (mspl_amd.script.train against the reference's train(), uest_seg_multi_os.py:958-1089),
shared by tests/golden/make_train_loop_golden.py (which runs the reference's own loop on them) and the tests.

Every case is ESPDNet-UE s = 2.0 with 5 classes in eval() mode (frozen BatchNorm), the greenhouse class weights below with class 4
ignored, Adam(lr 5e-4, weight decay 5e-4).  `phases` lists the epochs run on one optimizer object: a new entry is a NEW optimizer
(the script builds one per round, :594-598).  The loader serves the same seeded batches every epoch (batch b: tests.synth inputs
and labels with seed in_seed + b); `batches` are their sizes, so a last entry smaller than the others is the partial batch of a
loader without drop_last.
"""
import argparse

CLASS_WEIGHTS = [0.0, 6.31, 3.78, 3.18, 7.64]
IGNORE_IDX = 4
LR = 5e-4
WEIGHT_DECAY = 5e-4
WRITER_IDX0 = 7                  # the loop is handed a running index and returns it + 1
TOT_ITER = 6.0                   # arrives as a float (:609)
NEAR_MARGIN = 1e-3               # a pixel whose top-2 margin of the reference's main head is below this may flip its argmax
NEAR_CAP = 0.02                  # generator-asserted: at most this share of the pixels of a case is `near`

TRAIN_LOOP_CASES = {
    'loop_32x48': dict(hw=(32, 48), batches=(2, 2, 2), phases=(2, 1), power=0.9, use_uncertainty=True, use_traversable=False,
                       train_lanes=None, sd_seed=21, in_seed=100),
    'loop_64x96_tail': dict(hw=(64, 96), batches=(4, 4, 2), phases=(1,), power=0.0, use_uncertainty=True, use_traversable=True,
                            train_lanes=2, sd_seed=23, in_seed=110),
    'loop_ce_32x48': dict(hw=(32, 48), batches=(2, 2, 2), phases=(1,), power=0.0, use_uncertainty=False, use_traversable=False,
                          train_lanes=None, sd_seed=21, in_seed=100),
}


def loop_batches(case):
    """[(images (B,3,H,W) float32, labels (B,H,W) int64)] on the CPU."""
    from tests.synth import synth_input, synth_labels
    H, W = case['hw']
    return [(synth_input((b, 3, H, W), case['in_seed'] + i), synth_labels((b, H, W), 5, case['in_seed'] + i))
            for i, b in enumerate(case['batches'])]


def loop_args(case):
    """The fields of the script's `args` that train() reads."""
    a = argparse.Namespace(model='espdnetue', use_depth=False, use_uncertainty=case['use_uncertainty'],
                           use_traversable=case['use_traversable'], learning_rate=LR, power=case['power'])
    if case['train_lanes'] is not None:
        a.train_lanes = case['train_lanes']
    return a


def reference_areas(pred_argmax, target, K=4):
    """(3, K) int64 [inter | pred | mask]: utilities/metrics/segmentation_miou.py:28-41 in integer numpy (uint8 wrap-around, bins
    1..K).  pred_argmax / target: integer arrays of one shape."""
    import numpy as np
    p = (np.asarray(pred_argmax).astype(np.uint8) + np.uint8(1)).astype(np.uint8)
    t = (np.asarray(target).astype(np.int64) & 255).astype(np.uint8)
    t = (t + np.uint8(1)).astype(np.uint8)
    p = np.where(t > 0, p, 0).astype(np.uint8)
    inter = np.where(p == t, p, 0).astype(np.uint8)
    return np.stack([np.bincount(v.ravel(), minlength=256)[1:K + 1] for v in (inter, p, t)]).astype(np.int64)
