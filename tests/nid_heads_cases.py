"""Cases of the NID term at head resolution (csrc/nid_heads.hip: mspl_nid_heads_fwd / mspl_nid_finalize / mspl_nid_heads_bwd), shared by
tests/golden/make_nid_heads_golden.py (which runs the reference's NIDLoss on F.interpolate(main_lo, align_corners=True) in float64
and float32) and the tests.  CPU-importable.

A case is (B, C, K, (Hm, Wm), (H, W), seed): C classes (label_bin = C), K image bins, a (B,C,Hm,Wm) head, (B,3,H,W) images.

Inputs.  The camera is tests.synth.synth_nid_inputs's.  The head logits carry near-ties of ADJACENT classes laid out in blocks of 3 x 3
head pixels (fewer along an axis the head is shorter in) that share one class pair: inside a tie block the pair sits at 2 and 2 +
delta above small noise, delta a plane through the block of slope 1.5e-3 per head pixel in a seeded direction, so it crosses zero
inside the block and the INTERPOLATED pixels between its head pixels are near-ties too.  NIDLoss's gradient is exactly zero in
float32 away from |delta| < ~1.3e-4 (soft-arg-max slope 500, sigmoids of width 1e-3), so without such blocks a gradient test
compares zeros.  The generator asserts that the float64 reference gradient is non-zero on at least 1 % of the head's elements and
never on fewer than 10.

Seeds.  The same slopes multiply float32 rounding by ~5e5, so the reference's own float32 gradient leaves its float64 gradient by per
cent at unlucky pixels; a case's seed is acceptable only if, on the CPU and from the reference alone, this gap stays below 5 % of
the largest gradient entry (the generator asserts it; with the tie pair at the power of two 2.0 every seed tried does), which keeps
the bound of the GPU test -- GAP_FACTOR x the recorded gap -- far below what a wrong interpolation weight does.  The recorded gap
is the largest over FLOAT32_RUNS below (the reference in float32 on the inputs as they are and on one-ulp neighbours of them, each
against float64 on the same inputs): how far one float32 run lands from float64 is luck per near-tie pixel -- on case x2 the plain
run happens to land within 3e-4 of the largest gradient entry where its one-ulp neighbours and every other case land at 2e-3 ..
1.5e-2 -- and a single sample of it is no bound for another float32 implementation.  The tight gradient check is the one against
the three-step form on the device, which shares every per-pixel float with the fused kernels.
"""
GAP_FACTOR = 4.0                 # a GPU's other summation order on top of the reference's own float32 error (tests/supervised_loop_cases.py)
BW_CAMERA, BW_LABEL = 0.005, 0.001
BAND_ROWS, BAND_COLS = 4, 64     # what mspl_nid_heads_plan reports for every case below (the GPU tests assert it)
NONZERO_SHARE, NONZERO_MIN = 0.01, 10
# the generator's float32 runs of the reference: None = the inputs as they are, k = a seed of a one-ulp perturbation of head and camera
FLOAT32_RUNS = (None,) + tuple(range(6))
GRAD_GAP_CAP = 0.05              # generator-asserted: float32 reference gradient within this share of max |float64 gradient|

# the base table
NID_HEADS_CASES = {
    'x2': (2, 5, 16, (8, 12), (16, 24), 0),
    'bins32_c13': (3, 13, 32, (6, 10), (12, 20), 0),
    'odd_k_below_c': (1, 5, 4, (7, 9), (17, 23), 0),
    'one_row': (2, 5, 16, (1, 12), (16, 24), 0),
    'one_col': (2, 5, 16, (8, 1), (16, 24), 0),
    'same_size': (2, 5, 16, (16, 24), (16, 24), 0),
    'many_bands': (4, 5, 32, (24, 40), (48, 80), 0),
    # one case on each side of the band seams (a band is BAND_ROWS x BAND_COLS label positions): a map exactly one band wide / high,
    # and one column / row more (a second band of one column / row, whose patch is the head's last column / row alone)
    'band_cols_exact': (2, 5, 16, (4, 32), (8, 64), 0),
    'band_cols_plus1': (2, 5, 16, (4, 33), (8, 65), 0),
    'band_rows_exact': (2, 5, 16, (2, 12), (4, 24), 0),
    'band_rows_plus1': (2, 5, 16, (3, 12), (5, 24), 0),
    # the patch seam: the staged patch reaches its capacity (PATCH_ROWS x PATCH_COLS of the plan) at a non-integer scale, where bands
    # differ in how many head rows / columns they touch
    'patch_ragged': (2, 5, 16, (5, 50), (13, 70), 0),
}
# a 20-class head with 32 image bins: the plan decides whether it runs (the GPU test follows the plan); no reference fixture needed
# beyond the float64 oracle composition the CPU tier checks for every case
WIDE_CASE = ('c20_k32', (2, 20, 32, (6, 10), (12, 20), 0))
REFUSED_SHAPE = (2, 5, 16, (17, 24), (16, 24))          # a head larger than the map: MSPL_ERR_UNSUPPORTED


def head_logits(B, C, Hm, Wm, seed):
    """(B,C,Hm,Wm) float32 head logits with blocked near-ties (module docstring)."""
    import math
    import torch
    g = torch.Generator().manual_seed(7000 + seed)
    lab = torch.randn((B, C, Hm, Wm), generator=g)
    bh, bw = min(3, Hm), min(3, Wm)
    nby, nbx = -(-Hm // bh), -(-Wm // bw)
    tie = torch.rand((B, nby, nbx), generator=g) < 0.5
    c0 = torch.randint(0, C - 1, (B, nby, nbx), generator=g)
    theta = torch.rand((B, nby, nbx), generator=g) * (2 * math.pi)
    off = (torch.rand((B, nby, nbx), generator=g) - 0.5) * 6e-4
    for b in range(B):
        for by in range(nby):
            for bx in range(nbx):
                if not bool(tie[b, by, bx]):
                    continue
                y0, x0 = by * bh, bx * bw
                y1, x1 = min(y0 + bh, Hm), min(x0 + bw, Wm)
                yy = torch.arange(y0, y1, dtype=torch.float32).reshape(-1, 1) - 0.5 * (y0 + y1 - 1)
                xx = torch.arange(x0, x1, dtype=torch.float32).reshape(1, -1) - 0.5 * (x0 + x1 - 1)
                t = float(theta[b, by, bx])
                delta = 1.5e-3 * (yy * math.sin(t) + xx * math.cos(t)) + float(off[b, by, bx])
                c = int(c0[b, by, bx])
                lab[b, :, y0:y1, x0:x1] *= 0.3
                lab[b, c, y0:y1, x0:x1] = 2.0
                lab[b, c + 1, y0:y1, x0:x1] = 2.0 + delta
    return lab


def case_inputs(case):
    """(camera (B,3,H,W), main_lo (B,C,Hm,Wm)) float32 on the CPU, a pure function of the case."""
    from tests.synth import synth_nid_inputs
    B, C, K, (Hm, Wm), (H, W), seed = case
    cam, _ = synth_nid_inputs((B, 3, H, W), C, 500 + seed)
    return cam, head_logits(B, C, Hm, Wm, seed)


def hist_layout(joint, p_c, p_l, C, K):
    """The (K*Cl + K + Cl) layout of mspl_nid_hist_fwd from the reference's get_probabilities outputs (joint (K, label_bin), p_c (K),
    p_l (label_bin)): the first Cl = min(C, K) label bins -- the rest are never filled."""
    import numpy as np
    Cl = min(C, K)
    return np.concatenate([np.asarray(joint)[:, :Cl].reshape(-1), np.asarray(p_c).reshape(-1), np.asarray(p_l).reshape(-1)[:Cl]])


def oracle_nid_at_heads(cam, main_lo, K, C, dtype=None):
    """(loss2, d loss2 / d main_lo) of the oracle composition F.interpolate(align_corners=True) -> oracle.labels.nid_loss."""
    import torch
    import torch.nn.functional as F
    from oracle.labels import nid_loss
    dtype = dtype or torch.float64
    m = main_lo.to(dtype).clone().requires_grad_(True)
    up = F.interpolate(m, size=tuple(cam.shape[2:]), mode='bilinear', align_corners=True)
    loss = nid_loss(cam.to(dtype), up, image_bin=K, label_bin=C, bw_camera=BW_CAMERA, bw_label=BW_LABEL)
    loss.backward()
    return loss.detach(), m.grad.detach()
