"""The sweep of the pyramid kernels' host-side plan queries, shared by tests/golden/make_pyr_plans_golden.py (which records what the
library answers) and tests/test_pyr_plans_golden.py (which asks again).  No GPU: every query looks at shapes only.

A record is (N, P, h, w, sizes); `answers(record)` asks every plan query of the pyramid family about it and returns one dict of
name -> tuple of ints.  The up-only sublists of a record's sizes go to the branch-backward queries, its low-resolution tail to the
prologue's LDS query."""
import ctypes
import itertools

from mspl_amd import _native as nv
from mspl_amd import ops
from tests import epilogue_cases as E
from tests import pyr_stream_cases as C
from tests import resample_cases as R

# 6x9 .. 128x240; the seams the case files name: w = 39/40 (narrowest streamed map), 62/64 (columns per lane), 124/126 (column
# blocks), odd w, h = 19/20 (in-kernel segment), 72/73 (table segment)
MAPS = [(6, 9), (14, 22), (16, 30), (18, 30), (33, 47), (40, 39), (40, 40), (19, 40), (20, 40), (24, 62), (30, 64), (30, 65),
        (36, 60), (20, 124), (20, 126), (72, 40), (73, 40), (64, 120), (72, 120), (128, 240)]
BATCHES = (1, 2, 16, 128)
PLANES = (4, 6, 16, 32)
SCALES = (1.5, 2.0, 3.0, 4.0)
SCALE_PAIRS = list(itertools.product(SCALES, SCALES))
FORM_ID = {name: value for value, name in R.BRANCH.items()}          # mspl_pyr_branch_bwd_form_t


def records():
    """Every map with the reference's own branch sizes and with the 2.0 / 1.5 pair at every (N, P); every map with every scale pair at
    the smallest and at a training-sized (N, P)."""
    out = []
    for h, w in MAPS:
        for N, P in itertools.product(BATCHES, PLANES):
            out.append((N, P, h, w, tuple(E.pyr_sizes(h, w))))
            out.append((N, P, h, w, tuple(C.sizes_of(h, w, 2.0, 1.5))))
        for s0, s1 in SCALE_PAIRS:
            if (s0, s1) != (2.0, 1.5):
                for N, P in ((1, 4), (16, 16)):
                    out.append((N, P, h, w, tuple(C.sizes_of(h, w, s0, s1))))
    return out


def _arr(sizes, k):
    return (ctypes.c_int32 * len(sizes))(*[int(s[k]) for s in sizes])


def branch_lists(sizes):
    """[up], [up, up], [up, same], [up, up, same], the same-size branch first (the one-launch-per-branch form) and one list with a
    down branch, from a five-branch list."""
    up0, up1, same, down = sizes[0], sizes[1], sizes[2], sizes[3]
    return [[up0], [up0, up1], [up0, same], [up0, up1, same], [same, up0], [up0, down]]


def answers(rec):
    N, P, h, w, sizes = rec
    lib = nv.lib
    a = {}
    p = ops.pyrpool_stream_plan((N, P, h, w), sizes)
    a['stream_plan'] = tuple(p[k] for k in ('taken', 't0', 't1', 'pxl', 'ncb', 'cbw', 'seg', 'nseg', 'waves', 'seg_inkernel',
                                            'nseg_inkernel', 'waves_inkernel'))
    hs, ws = _arr(sizes, 0), _arr(sizes, 1)
    a['tables_bytes'] = (int(lib.mspl_pyr_stream_tables_bytes(h, w, len(sizes), hs, ws)),)
    a['train_fits'] = (int(lib.mspl_pyrpool_fused_train_fits(N, P, h, w, len(sizes), hs, ws)),)
    bwd = []
    for sub in branch_lists(sizes):
        for al in (0, 1):
            q = R.branch_plan(N, P, h, w, sub, aligned8=al)
            bwd += [FORM_ID[q.form], q.ncb, q.nseg, q.seg, *q.taps, q.tiles_x, q.tiles_y]
        bwd.append(int(R.branch_fits(N, P, h, w, sub)))
    a['branch_bwd'] = tuple(bwd)
    prep = []
    for sub in (sizes[3:], sizes[2:], sizes[1:]):        # [down, down], [same, down, down], and a list with an up branch
        prep.append(int(lib.mspl_pyr_down_prep_lds_bytes(N, P, h, w, len(sub), _arr(sub, 0), _arr(sub, 1))))
    a['prep_lds'] = tuple(prep)
    return a


QUERIES = ('stream_plan', 'tables_bytes', 'train_fits', 'branch_bwd', 'prep_lds')
BWD_STRIDE = 19                      # ints per sublist in 'branch_bwd': 2 x (form, ncb, nseg, seg, taps[3], tiles_x, tiles_y) + fits
