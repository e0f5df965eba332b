"""Cases of the drop-in single-head loops (mspl_amd.script.train_seg / mspl_amd.evaluation.val_seg against the reference's train_seg /
val_seg, utilities/train_eval_seg.py:16-162), shared by tests/golden/make_train_seg_golden.py (which runs the reference's own loops
on them) and the tests.

The settings are those of tests/supervised_loop_cases.py (imported there, not copied: 5 classes with class 4 ignored, its class
weights, momentum SGD over the script's two learning-rate groups, its low learning rates, its bounds and its float32 runs); what
differs is the model -- `net` 'espnetv2' (ESPNetv2Segmentation at width `s`) or 'espdnet' (ESPDNetSegmentation, s = 2.0, without a
depth image) -- and that there is no flooding.  `phases`, `lrs`, `batches` and `nid` as there.  After the last epoch val_seg runs on
VAL_BATCHES held-out batches (seeds in_seed + 50 + i).

Conditioning.  tests/supervised_loop_cases.py describes how the float32 trajectory of such a loop is bimodal at some inputs (its own
sup_32x48, in_seed 470: the reference's float32 runs leave its float64 run by 1e-4 in the parameters and by 1e-2 in single running
statistics, and a GPU lands in either mode from run to run).  The input seed of v2_s05_32x48 was chosen on the CPU, from the reference
alone, as the first of 470.. at which all of FLOAT32_RUNS stay within 2e-6 of the float64 run in every parameter (475: 1.8e-6, running
statistics 4.6e-6; at 470 .. 474 the gap is 1.5e-5 .. 7e-4).

The NID case.  tests/supervised_loop_cases.py describes why NIDLoss multiplies float32 rounding (a soft-arg-max of slope 500) and asks
of its NID case that the reference's float32 runs stay within PARAM_FLOOR of its float64 run.  For the single-head ESPNetv2 no input
seed of the 120 tried on the CPU (322..441, from the reference alone) does: the float32 runs leave the float64 run by 1e-4 .. 8e-2 in
the parameters after two steps.  The committed seed is the best of them; the generator asserts its largest per-tensor gap over
FLOAT32_RUNS stays below NID_GAP_CAP and records it, and the tests allow GAP_FACTOR times the recorded gap per tensor as everywhere
else.  So this case pins the loop around the additional criterion (the restated body, `weight`, the extra meter, the caller's
optimizer) to the reference's own float32 scatter; the gradient of NIDLoss itself is pinned by tests/golden/nid.npz."""
from tests.supervised_loop_cases import NUM_CLASSES

VAL_BATCHES = (4, 2)
NID_GAP_CAP = 1e-3

SINGLE_HEAD_LOOP_CASES = {
    'v2_s05_32x48': dict(net='espnetv2', s=0.5, hw=(32, 48), batches=(4, 4, 2), phases=(2, 1), lrs=(1e-3, 5e-4, 1e-3), nid=None, sd_seed=8,
                         in_seed=475),
    'espdnet_32x48': dict(net='espdnet', s=2.0, hw=(32, 48), batches=(4, 4), phases=(1,), lrs=(1e-3,), nid=None, sd_seed=8, in_seed=310),
    'v2_nid_32x48': dict(net='espnetv2', s=2.0, hw=(32, 48), batches=(4, 4), phases=(1,), lrs=(1e-3,), nid=0.5, sd_seed=8, in_seed=357),
}


def loop_batches(case):
    """[(images (B,3,H,W) float32, labels (B,H,W) int64 in 0..4)] on the CPU (tests/supervised_loop_cases.loop_batches)."""
    from tests.synth import synth_input, synth_labels
    H, W = case['hw']
    return [(synth_input((b, 3, H, W), case['in_seed'] + i), synth_labels((b, H, W), NUM_CLASSES, case['in_seed'] + i))
            for i, b in enumerate(case['batches'])]


def val_batches(case):
    from tests.synth import synth_input, synth_labels
    H, W = case['hw']
    return [(synth_input((b, 3, H, W), case['in_seed'] + 50 + i), synth_labels((b, H, W), NUM_CLASSES, case['in_seed'] + 50 + i))
            for i, b in enumerate(VAL_BATCHES)]


def build_model(case, espnetv2_cls, espdnet_cls):
    """The case's model from the given classes (the reference's in the generator, the drop-in's in the tests), seeded."""
    import argparse
    from tests.synth import synth_state_dict
    a = argparse.Namespace(s=case['s'], channels=3, num_classes=1000)
    if case['net'] == 'espnetv2':
        m = espnetv2_cls(a, classes=NUM_CLASSES, dataset='greenhouse')
    else:
        m = espdnet_cls(a, classes=NUM_CLASSES, dataset='greenhouse')
    m.load_state_dict(synth_state_dict(m.state_dict(), case['sd_seed']))
    return m
