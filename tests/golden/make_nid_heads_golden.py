#!/usr/bin/env python3
"""Generate tests/golden/nid_heads.npz: the REFERENCE's NIDLoss (loss_fns/segmentation_loss.py:54-144) on the up-sampled main head
(F.interpolate(main_lo, (H, W), mode='bilinear', align_corners=True), model/segmentation/espdnet_ue.py:301), on the CPU.

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout>:<this repository> python3 tests/golden/make_nid_heads_golden.py

Per case of tests/nid_heads_cases.py (keys `<case>.<name>`), from a float64 run:
    loss2      the scalar
    hist       joint (K,Cl) | p_c (K) | p_l (Cl) of get_probabilities, the layout of mspl_nid_hist_fwd
    grad       d loss2 / d main_lo (B,C,Hm,Wm)
and from float32 runs of the same code the largest absolute distance from each of them: gap_loss, gap_hist, gap_grad.  The float32
error of this loss is a matter of luck per pixel (a near-tie's soft-arg-max moves a sigmoid of width 1e-3; one rounding more or less
in the interpolated logit decides by how much), so one run under-samples it: the float32 runs are FLOAT32_RUNS of
tests/nid_heads_cases.py -- the inputs as they are, and with every element of the head and of the camera moved to a neighbouring
float32 by a seeded coin -- each against the float64 run on ITS inputs, and the largest distance is recorded.

NIDLoss builds its tensors with hard-coded `.to('cuda')` and `.float()`; the run happens inside a context in which a 'cuda' target
means "stay where you are" and `.float()` means the dtype of the run (the shim of make_train_seg_ue_golden.py); the reference's
arithmetic is untouched.  Asserted here: the float64 gradient is non-zero on at least NONZERO_SHARE of the head's elements and on
at least NONZERO_MIN; the float32 gradient stays within GRAD_GAP_CAP x max |float64 gradient| (the case seeds were chosen for it).
Only data is written.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.nid_heads_cases import (BW_CAMERA, BW_LABEL, FLOAT32_RUNS, GRAD_GAP_CAP, NID_HEADS_CASES, NONZERO_MIN, NONZERO_SHARE,  # noqa: E402
                                   case_inputs, hist_layout)
from tests.golden.make_train_seg_ue_golden import _run_dtype, one_ulp  # noqa: E402

from loss_fns.segmentation_loss import NIDLoss  # noqa: E402

torch.set_num_threads(4)


def reference(case, dtype, perturb=None):
    """(loss2, hist, grad) of the reference in `dtype`, as float64 numpy.  perturb: a seed -- both inputs move by one ulp (one_ulp)."""
    B, C, K, _, (H, W), _ = case
    cam, main = case_inputs(case)
    if perturb is not None:
        cam, main = one_ulp(cam, 2 * perturb), one_ulp(main, 2 * perturb + 1)
    cam = cam.to(dtype)
    m = main.to(dtype).clone().requires_grad_(True)
    with _run_dtype(dtype):
        nid = NIDLoss(image_bin=K, label_bin=C, bw_camera=BW_CAMERA, bw_label=BW_LABEL)
        up = F.interpolate(m, size=(H, W), mode='bilinear', align_corners=True)
        loss = nid(cam, up)
        loss.backward()
        with torch.no_grad():
            lab = nid.soft_arg_max_layer(up)
            joint, p_c, p_l = nid.get_probabilities(nid.get_grayscale(cam), lab.reshape(B, H, W))
    hist = hist_layout(joint.double().numpy(), p_c.double().numpy(), p_l.double().numpy(), C, K)
    return float(loss.detach().double()), hist.astype(np.float64), m.grad.detach().double().numpy()


def one_case(name, case):
    l64, h64, g64 = reference(case, torch.float64)
    nz = int((g64 != 0).sum())
    gmax = float(np.abs(g64).max())
    gaps = dict(gap_loss=0.0, gap_hist=0.0, gap_grad=0.0)
    for k in FLOAT32_RUNS:
        a64 = (l64, h64, g64) if k is None else reference(case, torch.float64, k)
        a32 = reference(case, torch.float32, k)
        for key, x, y in zip(('gap_loss', 'gap_hist', 'gap_grad'), a32, a64):
            gaps[key] = max(gaps[key], float(np.abs(np.asarray(x) - np.asarray(y)).max()))
    return dict(loss2=np.float64(l64), hist=h64, grad=g64, **{k: np.float64(v) for k, v in gaps.items()}), nz, gmax


def main():
    import contextlib
    import io
    arrays = {}
    for name, case in sorted(NID_HEADS_CASES.items()):
        with contextlib.redirect_stdout(io.StringIO()):          # (NIDLoss prints its bins)
            rec, nz, gmax = one_case(name, case)
        n = rec['grad'].size
        assert nz >= max(NONZERO_MIN, NONZERO_SHARE * n), (name, nz, n)
        assert rec['gap_grad'] <= GRAD_GAP_CAP * gmax, (name, float(rec['gap_grad']), gmax)
        print('%-16s loss2 %.6f  non-zero gradient entries %d of %d  max |grad| %.3e  gaps: loss %.2e hist %.2e grad %.2e (%.3f of max)'
              % (name, rec['loss2'], nz, n, gmax, rec['gap_loss'], rec['gap_hist'], rec['gap_grad'], rec['gap_grad'] / gmax))
        for k, v in rec.items():
            arrays['%s.%s' % (name, k)] = v
    path = os.path.join(HERE, 'nid_heads.npz')
    np.savez_compressed(path, **arrays)
    print('wrote %s (%.1f KiB)' % (path, os.path.getsize(path) / 1024))


if __name__ == '__main__':
    main()
