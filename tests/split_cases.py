"""Cases and CPU oracles of the split-bf16 matrix mode of the dense convolution (mspl_dense_conv_split_fwd, ASPP heads), shared by
tests/test_split_host.py and tests/test_gpu_dense_conv_split.py.  No GPU, nothing of the code under test.

Split rule (include/mspl_hip.h):  r_0 = v,  plane_i = bf16_rne(r_i),  r_{i+1} = r_i - float(plane_i);  the mode keeps the products
plane_i(w) * plane_j(x) with i + j < planes.
"""
import functools

import torch
import torch.nn.functional as F

# (N, Cin, Cout, H, W, k, d): the shapes at which K13's own shape test found its edges
SHAPES = [
    (1, 64, 40, 7, 9, 3, 2),          # 63 pixels: less than one tile; Cout below one tile
    (2, 96, 130, 5, 13, 1, 1),        # Cout tail (two row blocks, the second with 2 rows), three K chunks, 1x1
    (1, 32, 256, 11, 6, 3, 12),       # dilation larger than the map: 8 of 9 taps dead
    (3, 128, 16, 9, 9, 3, 3),         # tiles span images
    (1, 32, 40, 250, 263, 3, 2),      # 514 tiles of 128 pixels: the smallest Cin = 32, 3x3 shape that selects the wide form
]
BATCH_SHAPE = SHAPES[3]
PLANES = (2, 3)
# |emulated - true| <= C_SPLIT[planes] * conv(|x|, |w|).  bf16 rounds to 8 significant bits (unit roundoff 2^-8): a plane is at most
# 2^-8 of the one before, a two-plane split leaves a residual of at most 2^-16 of the value, a three-plane one 2^-24.  bf16x3 drops
# lo*lo (2^-16) and carries the two split residuals (2 * 2^-16); bf16x6 drops mid*lo and lo*mid (2 * 2^-24) and carries two
# residuals (2 * 2^-24); the terms of higher order (2^-32) are far inside the slack random data leave to these worst cases.
C_SPLIT = {2: 3 * 2.0 ** -16, 3: 4 * 2.0 ** -24}


def problem(shape, seed=0):
    """Seeded randn input and weight, the weight scaled by (Cin k k)^-0.5."""
    N, Cin, Cout, H, W, k, d = shape
    g = torch.Generator().manual_seed(1000 + seed)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) * (Cin * k * k) ** -0.5
    return x, w


def split_planes(t, planes):
    """The bf16 planes of a float32 tensor, each as float32 values."""
    out, r = [], t.float()
    for _ in range(planes):
        p = r.to(torch.bfloat16).to(torch.float32)
        out.append(p)
        r = r - p
    return out


def _conv64(x, w, pad, dil):
    return F.conv2d(x.double(), w.double(), None, 1, pad, dil)


def emulated_conv(x, w, pad, dil, planes):
    """Sum over i + j < planes of conv(plane_j(x), plane_i(w)) in float64.  The inner sums of x planes are exact in float64 (at most
    3 x 8 significant bits within a span far below 53), so this is one convolution per weight plane."""
    xs, ws = split_planes(x, planes), split_planes(w, planes)
    tot = None
    for i in range(planes):
        xsum = sum(p.double() for p in xs[:planes - i])
        term = _conv64(xsum, ws[i], pad, dil)
        tot = term if tot is None else tot + term
    return tot


def true_conv(x, w, pad, dil):
    return _conv64(x, w, pad, dil)


def mag_conv(x, w, pad, dil):
    return _conv64(x.abs(), w.abs(), pad, dil)


@functools.lru_cache(maxsize=None)
def reference(index):
    """Everything the tests compare against for SHAPES[index], computed once per process and never modified by a test:
    x, w, true (float64), mag (float64), e32 = max |float32 CPU conv - true|, emu[planes] (float64)."""
    shape = SHAPES[index]
    N, Cin, Cout, H, W, k, d = shape
    pad = d * (k // 2)
    x, w = problem(shape, index)
    true = true_conv(x, w, pad, d)
    e32 = float((F.conv2d(x, w, None, 1, pad, d).double() - true).abs().max())
    return {'shape': shape, 'x': x, 'w': w, 'pad': pad, 'true': true, 'mag': mag_conv(x, w, pad, d), 'e32': e32,
            'emu': {p: emulated_conv(x, w, pad, d, p) for p in PLANES}}
