"""Cases of the drop-in supervised loop (mspl_amd.script.train_seg_ue against the reference's train_seg_ue,
utilities/train_eval_seg.py:164-247), shared by tests/golden/make_train_seg_ue_golden.py (which runs the reference's own loop on them)
and the tests.

Every case is ESPDNet-UE s = 2.0 with 5 classes in train() mode (batch-statistics BatchNorm), the class weights below with class 4
ignored (NUM_CLASSES = 5, so MIOU has K = 4 bins), torch.optim.SGD over the script's two learning-rate groups (base network at lr,
segmentation head at lr * LR_MULT), momentum 0.9, weight decay 4e-5.  `phases` lists the epochs run on one optimizer object: a new
entry is a NEW optimizer.  `lrs` is the base learning rate the caller writes into the groups before each epoch
(train_segmentation.py:353-362).  The loader serves the same seeded batches every epoch; `batches` are their sizes, so a smaller
last entry is the partial batch of a loader without drop_last.  `nid` is the `weight` of an NIDLoss additional criterion, or None.

The rates are far below the script's default 0.009 on purpose: there the reference's own float32 run drifts 3e-4 in the loss average
and 3e-3 in the parameters from its float64 run within two epochs, which pins nothing.

Sensitivity.  In train() mode at these sizes the level-4 maps are 2 x 3 (4 x 6) pixels, 24 (96) values per channel of a batch: one
PReLU input changing side moves a channel's batch statistics by per cent, and the float32 trajectory is bimodal under perturbations
of rounding size.  With sup_32x48's images moved by one ulp the reference's own float32 loop stays within 4e-7 of its float64 loop
after the first phase in some seeded runs and leaves it by 6.9e-5 in bu_dec_l1.stages.4.weight in another; a GPU lands in
either mode from run to run (float atomics).  The generator therefore records, per epoch and per tensor, the LARGEST gap over
FLOAT32_RUNS below, and the tests allow GAP_FACTOR times that, never less than the floors.  The generator asserts that the bounds
so obtained still catch a first batch applied twice and a dropped last batch in both learning-rate groups.

The NID case's input seed is chosen for its conditioning, on the CPU and from the reference alone: NIDLoss's gradient passes a
soft-arg-max of slope 500 and sigmoids of width 1e-3, so one pixel whose top two ADJACENT classes tie within ~1e-4 multiplies float32
rounding by ~1e5, and the reference's float32 run then leaves its float64 run by 1e-3 .. 0.5 in the parameters after two
steps; at most seeds there is such a pixel, at a few there is none and the runs agree to 1e-6.  The generator asserts that the
committed case is one of the latter (largest per-tensor gap over FLOAT32_RUNS below PARAM_FLOOR); the gradient of NIDLoss itself is pinned on adversarial near-ties by its own golden (tests/golden/nid.npz).
"""
CLASS_WEIGHTS = [1.45, 6.31, 3.78, 3.18, 0.0]
IGNORE_IDX = 4
NUM_CLASSES = 5
LR_MULT = 10.0
MOMENTUM = 0.9
WEIGHT_DECAY = 4e-5
FLOOD = 0.015                    # utilities/train_eval_seg.py:178
NEAR_MARGIN = 1e-3               # a pixel whose top-2 margin of the summed logits is below this may flip its argmax
NEAR_CAP = 0.02                  # generator-asserted: at most this share of the pixels of a case is `near`
LOSS_RTOL, LOSS_ATOL = 2e-5, 1e-5        # the project's one-step loss bound
PARAM_FLOOR = 5e-5
# the generator's float32 runs of the reference loop: (threads, seed of a one-ulp perturbation of the images or None)
FLOAT32_RUNS = ((4, None), (1, None), (2, None)) + tuple((4, k) for k in range(6))
GAP_FACTOR = 4.0                 # a GPU's other summation order on top of the reference's own float32 error

SUPERVISED_LOOP_CASES = {
    'sup_32x48': dict(hw=(32, 48), batches=(4, 4, 4), phases=(2, 1), lrs=(1e-3, 5e-4, 1e-3), nid=None, sd_seed=8, in_seed=470),
    'sup_64x96_tail': dict(hw=(64, 96), batches=(4, 4, 2), phases=(1,), lrs=(1e-3,), nid=None, sd_seed=10, in_seed=310),
    'sup_nid_32x48': dict(hw=(32, 48), batches=(4, 4), phases=(1,), lrs=(1e-3,), nid=0.5, sd_seed=8, in_seed=322),
}


def loop_batches(case):
    """[(images (B,3,H,W) float32, labels (B,H,W) int64 in 0..4; a fifth of them the ignored class 4 -- nn.CrossEntropyLoss takes no
    label outside 0..C-1 other than its ignore_index, so there are no 255s here)] on the CPU."""
    from tests.synth import synth_input, synth_labels
    H, W = case['hw']
    return [(synth_input((b, 3, H, W), case['in_seed'] + i), synth_labels((b, H, W), NUM_CLASSES, case['in_seed'] + i))
            for i, b in enumerate(case['batches'])]


def group_of(name):
    """The learning-rate group of a parameter by its name (model/segmentation/espdnet_ue.py:129-156): 0 = base network, 1 =
    segmentation head, None = in neither (auxiliary decoder, depth encoder, fusion gates)."""
    head = ('bu_dec_l1.', 'bu_dec_l2.', 'bu_dec_l3.', 'bu_dec_l4.', 'merge_enc_dec_l4.', 'merge_enc_dec_l3.', 'merge_enc_dec_l2.',
            'bu_br_l4.', 'bu_br_l3.', 'bu_br_l2.')
    if name.startswith('base_net.'):
        return 0
    return 1 if name.startswith(head) else None


def loss_bound(ref, gap):
    return max(LOSS_RTOL * abs(ref) + LOSS_ATOL, GAP_FACTOR * gap)


def param_bounds(gaps):
    """Per-tensor bound from the generator's recorded per-tensor float32-against-float64 gaps."""
    import numpy as np
    return np.maximum(PARAM_FLOOR, GAP_FACTOR * np.asarray(gaps, dtype=np.float64))


def per_tensor_max(diff, off):
    """Largest |diff| per tensor of a flat parameter sample with tensor offsets `off`."""
    import numpy as np
    d = np.abs(np.asarray(diff, dtype=np.float64))
    return np.array([d[off[i]:off[i + 1]].max() if off[i + 1] > off[i] else 0.0 for i in range(len(off) - 1)])
