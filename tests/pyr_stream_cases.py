"""Cases of the pyramid streaming kernel's geometry-table path, shared by test_pyr_stream_plan.py (which proves from the library's
own plan query that every seam below is reached) and test_gpu_pyr_tables.py (which runs them).

A case: (name, N, P, h, w, s0, s1): an (N, P, h, w) map whose two up branches work at s0 x and s1 x its size; the other three
branches are the map itself, half of it and a tenth of it (at least 5), as in EfficientPyrPool.  A 2 x branch has a 3-tap
stencil, a 1.5 x branch a 5-tap one."""
import math

import torch
import torch.nn.functional as F

OLD_SEGMAX = 19                      # rows per segment the in-kernel tables allow

CASES = [
    # the PXL and column-block seams at 4-8 planes: w <= 62 is one column per lane, w > 124 is two column blocks
    ('pxl1_40x40', 1, 4, 40, 40, 2.0, 1.5),
    ('pxl1_24x62', 1, 8, 24, 62, 1.5, 2.0),
    ('pxl2_30x64', 2, 4, 30, 64, 2.0, 2.0),
    ('pxl2_two_blocks_20x126', 1, 4, 20, 126, 1.5, 1.5),
    # 2 048 planes: one segment of 40 rows per plane
    ('long_segment_40x40', 128, 16, 40, 40, 2.0, 1.5),
    # 2 048 planes, 73 rows: two segments, 37 + 36 rows
    ('ragged_73x40', 128, 16, 73, 40, 2.0, 1.5),
]
# image k of the big batch against the image alone: the two batches get different segment lengths
BATCH_CASE = 'long_segment_40x40'


def case(name):
    return next(c for c in CASES if c[0] == name)


def sizes_of(h, w, s0, s1):
    up = lambda v, s: int(math.ceil(v * s))                                     # noqa: E731
    return [(up(h, s0), up(w, s0)), (up(h, s1), up(w, s1)), (h, w), (max(up(h, 0.5), 5), max(up(w, 0.5), 5)),
            (max(up(h, 0.1), 5), max(up(w, 0.1), 5))]


def make_inputs(N, P, h, w, sizes, seed):
    """Random float32 planes, weights and BN / PReLU constants of the block, and the low-resolution maps the two down branches
    hand to the kernel (inputs here: other launches compute them)."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)                                # noqa: E731
    nb = len(sizes)
    inp = {'x': rn(N, P, h, w) - 0.2, 'stage_w': [rn(P, 1, 3, 3) / 3.0 for _ in sizes],
           'br_scale': torch.rand(nb * P, generator=g) + 0.5, 'br_shift': rn(nb * P) * 0.1,
           'br_alpha': torch.rand(nb * P, generator=g) * 0.3, 'merge_w': rn(P, nb, 3, 3) * (9 * nb) ** -0.5,
           'ep_scale': torch.rand(P, generator=g) + 0.5, 'ep_shift': rn(P) * 0.3, 'ep_alpha': torch.rand(P, generator=g) * 0.3}
    inp['down_e'] = {i: F.conv2d(F.adaptive_avg_pool2d(inp['x'].double(), sizes[i]), inp['stage_w'][i].double(), None, 1, 1, 1, P).float()
                     for i in (3, 4)}
    return inp


def _affine_prelu(v, s, b, a):
    v = v * s.to(v.dtype).view(1, -1, 1, 1) + b.to(v.dtype).view(1, -1, 1, 1)
    return torch.where(v > 0, v, v * a.to(v.dtype).view(1, -1, 1, 1))


def reference(inp, sizes, dtype=torch.float64):
    """nn_layers/efficient_pyramid_pool.py:39-58 between the projection and the final 1x1, in `dtype`, from the float32 inputs."""
    c = lambda t: t.to(dtype)                                                   # noqa: E731
    x = c(inp['x'])
    N, P, h, w = x.shape
    outs = []
    for i, size in enumerate(sizes):
        if i in inp['down_e']:
            t = F.interpolate(c(inp['down_e'][i]), (h, w), mode='bilinear', align_corners=True)
        elif size == (h, w):
            t = F.conv2d(x, c(inp['stage_w'][i]), None, 1, 1, 1, P)
        else:
            t = F.interpolate(x, size, mode='bilinear', align_corners=True)
            t = F.adaptive_avg_pool2d(F.conv2d(t, c(inp['stage_w'][i]), None, 1, 1, 1, P), (h, w))
        outs.append(t)
    nb = len(outs)
    a = _affine_prelu(torch.cat(outs, 1), inp['br_scale'], inp['br_shift'], inp['br_alpha'])
    a = a.view(N, nb, P, h, w).transpose(1, 2).reshape(N, nb * P, h, w)          # Shuffle(groups=nb)
    return _affine_prelu(F.conv2d(a, c(inp['merge_w']), None, 1, 1, 1, P), inp['ep_scale'], inp['ep_shift'], inp['ep_alpha'])
