"""The pyramid's training backward (pyrpool_train.hip: mspl_pyrpool_merge_bwd, mspl_pyrpool_branch_bwd in its three forms) through
the C ABI against float64 autograd of the plain torch expression, on the cases of tests/resample_cases.py;
tests/test_resample_cases.py proves on the CPU that each case reaches the form, column block, row segment, tap pair or tile seam it
is in the table for.

Dense random data: every output per plane within 4 * max(err32, 2^-23 * M) (tests/resample_cases.py).  Overwritten destinations
(gt, gx) are pre-filled with NaN, accumulated ones (every parameter gradient) with 0.5, which is subtracted afterwards; a second
call gives the same bits in the overwritten outputs.  A shape the library refuses raises, leaves its destinations alone and does
not disturb the next call.  Seam probes: gt one-hot on either side of a column-block, row-segment or tile seam; the footprint in gx
must cross the seam intact.  (The merge backward on integer data, EQUAL to float64: tests/test_gpu_exact_grad.py, op pyr_merge.)"""
import ctypes

import pytest
import torch

from tests import resample_cases as rc
from tests.test_gpu_resample_grad import _dev, _p, _stream, _sync, assert_within

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAN = float('nan')
PRE = 0.5
MERGE = [c.id for c in rc.CASES if c.op == 'pyr_merge']
BRANCH = [c.id for c in rc.CASES if c.op == 'pyr_branch']
MERGE_PARAMS = ('g_br_scale', 'g_br_shift', 'g_br_alpha', 'g_merge_w', 'g_m_scale', 'g_m_shift', 'g_m_alpha')


def run_pyr_merge(shape, p, lib, check, pre=PRE):
    """mspl_pyrpool_merge_bwd -> its eight outputs; gt starts as NaN, the accumulated parameter gradients as `pre`."""
    N, P, h, w, nb = shape
    d = {k: _dev(p[k]) if k in p else None for k in ('gy', 'mraw', 'zcat', 'br_scale', 'br_shift', 'br_alpha', 'br_mean', 'br_inv', 'merge_w',
                                                     'm_scale', 'm_shift', 'm_alpha', 'm_mean', 'm_inv')}
    o = {'gt': torch.full((nb, N, P, h, w), NAN, device=DEV)}
    for name, shp in zip(MERGE_PARAMS, [(nb * P,)] * 3 + [(P, nb, 3, 3)] + [(P,)] * 3):
        o[name] = torch.full(shp, float(pre), device=DEV)
    if 'm_alpha' not in p:
        del o['g_m_alpha']
    check(lib.mspl_pyrpool_merge_bwd(_p(d['gy']), _p(d['mraw']), _p(d['zcat']), N, P, h, w, nb, _p(d['br_scale']), _p(d['br_shift']),
                                     _p(d['br_alpha']), _p(d['br_mean']), _p(d['br_inv']), _p(d['merge_w']), _p(d['m_scale']), _p(d['m_shift']),
                                     _p(d['m_alpha']), _p(d['m_mean']), _p(d['m_inv']), _p(o['gt']), *[_p(o.get(n)) for n in MERGE_PARAMS],
                                     _stream()))
    return o


@pytest.mark.parametrize('cid', MERGE)
def test_merge_backward_against_float64(cid):
    from mspl_amd._native import check, lib
    case = rc.BY_ID[cid]
    p = rc.inputs(case)
    got = run_pyr_merge(case.shape, p, lib, check)
    _sync(cid)
    assert_within(cid, {k: (v - PRE if k != 'gt' else v) for k, v in got.items()}, rc.refs(cid))
    again = run_pyr_merge(case.shape, p, lib, check)
    _sync(cid)
    assert torch.equal(again['gt'], got['gt']), '%s: a second call gives other bits in gt' % cid


def run_branch(case, p, lib, check, outs=None):
    """mspl_pyrpool_branch_bwd -> {'gx', 'gw<i>'}; gx starts as NaN, gw<i> as 0.5.  outs: use these destinations."""
    N, P, h, w = case.shape
    sizes = rc.sizes_of(case)
    nb = len(sizes)
    x = _dev(p['x'])
    ws, gts = [_dev(p['w%d' % i]) for i in range(nb)], [_dev(p['gt%d' % i]) for i in range(nb)]
    adds = [_dev(p['add%d' % k]) for k in range(case.cfg['adds'])] + [None, None]
    if outs is None:
        outs = {'gx': _dev(torch.full((N, P, h, w), NAN), bool(case.cfg.get('misalign')))}
        outs.update({'gw%d' % i: torch.full((P, 1, 3, 3), PRE, device=DEV) for i in range(nb)})
    arr = lambda ts: (ctypes.c_void_p * nb)(*[t.data_ptr() for t in ts])          # noqa: E731
    hsa, wsa = (ctypes.c_int32 * nb)(*[s[0] for s in sizes]), (ctypes.c_int32 * nb)(*[s[1] for s in sizes])
    check(lib.mspl_pyrpool_branch_bwd(_p(x), N, P, h, w, nb, hsa, wsa, arr(ws), arr(gts), arr([outs['gw%d' % i] for i in range(nb)]),
                                      _p(adds[0]), _p(adds[1]), _p(outs['gx']), _stream()))
    return outs


def _check_branch(case, p, refs, note=''):
    from mspl_amd._native import check, lib
    got = run_branch(case, p, lib, check)
    _sync(case.id)
    form = rc.plan(case)
    assert_within(case.id, {k: (v - PRE if k != 'gx' else v) for k, v in got.items()}, refs, ' (%s)%s' % (form, note))
    again = run_branch(case, p, lib, check)
    _sync(case.id)
    assert torch.equal(again['gx'], got['gx']), '%s: a second call gives other bits in gx' % case.id
    return got


@pytest.mark.parametrize('cid', BRANCH)
def test_branch_backward_against_float64(cid):
    from mspl_amd._native import check, lib
    case = rc.BY_ID[cid]
    N, P, h, w = case.shape
    fits = rc.branch_fits(N, P, h, w, rc.sizes_of(case))
    assert fits == (case.form != 'unsupported')
    if fits:
        _check_branch(case, rc.inputs(case), rc.refs(cid))
        return
    # refused: an error, untouched destinations, and the next valid call is right
    p = rc.inputs(case)
    outs = {'gx': torch.full((N, P, h, w), 7.0, device=DEV)}
    outs.update({'gw%d' % i: torch.full((P, 1, 3, 3), PRE, device=DEV) for i in range(len(case.cfg['scales']))})
    with pytest.raises(RuntimeError, match='not covered'):
        run_branch(case, p, lib, check, outs)
    _sync(cid)
    assert bool((outs['gx'] == 7.0).all()) and all(bool((v == PRE).all()) for k, v in outs.items() if k != 'gx')
    nxt = rc.BY_ID['pyr_branch-nup1-same']
    _check_branch(nxt, rc.inputs(nxt), rc.refs(nxt.id), ' after a refused call')


def _seams():
    """(case id, branch, row, column, what): one-hot positions of gt on either side of each seam of the case's form."""
    out = []
    for cid in ('pyr_branch-two-blocks', 'pyr_branch-stream-blocks'):
        case = rc.BY_ID[cid]
        N, P, h, w = case.shape
        seg = rc.branch_plan(N, P, h, w, rc.sizes_of(case)).seg
        for i in range(len(case.cfg['scales'])):
            out += [(cid, i, seg, c, 'column block 123 | 124') for c in (123, 124, 125)]
            out += [(cid, i, r, 60, 'row segment %d | %d' % (seg - 1, seg)) for r in (seg - 1, seg)]
            out += [(cid, i, r, c, 'segment and block corner') for r in (seg - 1, seg) for c in (123, 124)]
    cid = 'pyr_branch-tile-odd-w'
    for i in range(3):
        out += [(cid, i, 8, c, 'tile column 31 | 32') for c in (31, 32)] + [(cid, i, r, 8, 'tile row 15 | 16') for r in (15, 16)]
        out += [(cid, i, r, c, 'tile corner') for r in (15, 16) for c in (31, 32)]
    return out


@pytest.mark.parametrize('cid', ['pyr_branch-two-blocks', 'pyr_branch-stream-blocks', 'pyr_branch-tile-odd-w'])
def test_branch_seam_probes(cid):
    """P probes per launch, each on a plane of its own (gt of its branch one-hot there, every other gt zero): gx against the
    float64 reference of the same data under the dense bound, and every element of the float64 footprint that stands clear of
    the bound is non-zero in the kernel's -- on both sides of the seam wherever the footprint crosses it."""
    case = rc.BY_ID[cid]
    N, P, h, w = case.shape
    nb = len(case.cfg['scales'])
    base = {k: v for k, v in rc.inputs(case).items() if not k.startswith(('add', 'gt'))}
    quiet = rc.Case(case.op, case.id, case.shape, case.form, case.where, dict(case.cfg, adds=0))
    probes = [s for s in _seams() if s[0] == cid]
    crossed = set()
    for p0 in range(0, len(probes), P):
        run = probes[p0:p0 + P]
        q = dict(base)
        q.update({'gt%d' % i: torch.zeros(N, P, h, w) for i in range(nb)})
        for c, (_, i, r, col, what) in enumerate(run):
            q['gt%d' % i][0, c, r, col] = 1.0
        r64, r32, mag = rc.reference(quiet, q), rc.reference(quiet, q, torch.float32), rc.reference(quiet, {k: v.abs() for k, v in q.items()})
        refs = {}
        for n in r64:
            err, m = rc.plane_max(n, r32[n].double() - r64[n]), rc.plane_max(n, mag[n])
            refs[n] = rc.Ref(r64[n], err, m, rc.MARGIN * torch.maximum(err, rc.EPS * m))
        got = _check_branch(quiet, q, refs, ' seam probes %d..%d' % (p0, p0 + len(run) - 1))
        gx = got['gx'].cpu().double()
        for c, (_, i, r, col, what) in enumerate(run):
            foot = r64['gx'][0, c].abs() > 64 * float(refs['gx'].bound[0, c])
            rows, cols = torch.nonzero(foot, as_tuple=True)
            assert len(rows), (cid, i, r, col)
            ce = 32 if 'tile' in what else 124
            if bool((cols < ce).any()) and bool((cols >= ce).any()):
                crossed.add('column')
            if 'row' in what or 'corner' in what:
                edge = 16 if 'tile' in what else rc.branch_plan(N, P, h, w, rc.sizes_of(case)).seg
                if bool((rows < edge).any()) and bool((rows >= edge).any()):
                    crossed.add('row')
            assert bool((gx[0, c][foot] != 0).all()), '%s branch %d probe (%d, %d) at %s: %d elements of the footprint are 0' % (
                cid, i, r, col, what, int((gx[0, c][foot] == 0).sum()))
    assert crossed == {'column', 'row'}, '%s: no float64 footprint crosses a %s seam' % (cid, {'column', 'row'} - crossed)
