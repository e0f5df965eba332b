"""Cases of the drop-in self-training loop WITH the additional NID loss (mspl_amd.script.train(..., add_loss=NIDLoss(image_bin=32,
label_bin=5)) against the reference's train(), uest_seg_multi_os.py:958-1089 with :1027-1030 taken), shared by
tests/golden/make_train_loop_nid_golden.py (which runs the reference's own loop on them) and the tests.  Everything else is as in
tests/train_loop_cases.py: ESPDNet-UE s = 2.0 with 5 classes in eval() mode, its class weights, Adam(lr 5e-4, weight decay 5e-4),
`phases` = epochs per optimizer object, the same seeded batches every epoch.

Conditioning (the way of tests/supervised_loop_cases.py).  NIDLoss's gradient passes a soft-arg-max of slope 500 and sigmoids of width
1e-3: one pixel whose top two ADJACENT classes tie within ~1e-4 multiplies float32 rounding by ~1e5, and the reference's own float32
loop then leaves its float64 loop far beyond any bound worth asserting.  `in_seed` is therefore chosen on the CPU, from the reference
alone: the generator asserts that over FLOAT32_RUNS (thread counts and one-ulp perturbations of the images) the reference's float32
loop stays within the project's one-step loss bound (LOSS_RTOL, LOSS_ATOL) of its float64 loop in both uest/train/loss and
uest/train/nid_loss, that assert_weights_close_after_adam(float32, float64) holds, and that the near-pixel share stays below
NEAR_CAP; it records the largest gaps, and the tests allow GAP_FACTOR times them, never less than the one-step bound.  The gradient
of the NID term itself is pinned at kernel level, on blocked near-ties (tests/nid_heads_cases.py).
"""
from tests.supervised_loop_cases import FLOAT32_RUNS, GAP_FACTOR, LOSS_ATOL, LOSS_RTOL, loss_bound  # noqa: F401
from tests.train_loop_cases import (CLASS_WEIGHTS, IGNORE_IDX, LR, NEAR_CAP, NEAR_MARGIN, TOT_ITER, WEIGHT_DECAY, WRITER_IDX0,  # noqa: F401
                                    loop_args, loop_batches, reference_areas)

NID_IMAGE_BIN, NID_LABEL_BIN = 32, 5

TRAIN_LOOP_NID_CASES = {
    'loop_nid_32x48': dict(hw=(32, 48), batches=(2, 2, 2), phases=(1, 1), power=0.9, use_uncertainty=True, use_traversable=False,
                           train_lanes=None, sd_seed=23, in_seed=100),
    # train_lanes=2 is asked for and must be overridden: the NID histogram couples the images of a batch
    'loop_nid_64x96_tail': dict(hw=(64, 96), batches=(4, 4, 2), phases=(1,), power=0.0, use_uncertainty=True, use_traversable=True,
                                train_lanes=2, sd_seed=23, in_seed=110),
}
