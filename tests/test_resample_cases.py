"""The table of tests/resample_cases.py, checked without a GPU: (a) the library's plan queries confirm that every case reaches the
kernel form and the seam it is in the table for, and that the table as a whole reaches every form; (b) the probe sets are valid --
decided from the float64 operator alone, no two hot elements of one plane share a receiver; (c) the float32 CPU evaluation of
every reference is finite, and its gap to float64 (the tolerance unit of the GPU tests) is recorded.  A case whose property is
not met FAILS."""
import ctypes
import math

import pytest
import torch

from mspl_amd import _native as nv
from tests import resample_cases as rc

IDS = [c.id for c in rc.CASES]
PLANNED = [c.id for c in rc.CASES if c.form is not None]
BRANCH = [c.id for c in rc.CASES if c.op == 'pyr_branch']
LINEAR = [c.id for c in rc.CASES if c.op in rc.LINEAR]


@pytest.mark.parametrize('cid', PLANNED)
def test_case_reaches_its_form(cid):
    case = rc.BY_ID[cid]
    assert rc.plan(case) == case.form, '%s (%s): the library takes %s' % (cid, case.where, rc.plan(case))
    if case.cfg.get('misalign'):
        aligned = rc.avgpool_plan(*case.shape) if case.op == 'avgpool' else rc.branch_plan(*case.shape, rc.sizes_of(case)).form
        assert aligned != case.form, 'the aligned call takes the same form: nothing falls back'


def test_bilinear_seams():
    plan = {c.id: rc.bilinear_plan(*c.shape) for c in rc.CASES if c.op == 'bilinear'}
    want = {'bilinear-8x64-16x128': ('tile8', 1, 1), 'bilinear-8x65-16x130': ('tile8', 2, 1), 'bilinear-9x70-18x140': ('tile8', 2, 2),
            'bilinear-17x33-29x57': ('tile8', 1, 3), 'bilinear-30x40-20x25': ('tile8', 1, 4), 'bilinear-6x70-18x210': ('tile12', 2, 2),
            'bilinear-6x66-21x261': ('tile12', 2, 2)}
    for cid, w in want.items():
        assert plan[cid][:3] == w, (cid, plan[cid])
    # the staged window of the full tile: all 16 x 128 output gradients; with a 65th input column the first tile's window takes the
    # extra candidate on its right (clamped to the map)
    assert plan['bilinear-8x64-16x128'][3:] == (16, 128)
    assert plan['bilinear-8x65-16x130'][3:] == (16, 130)
    for cid, p in plan.items():
        assert (p[1] > 0) == p[0].startswith('tile') and (p[3] > 0) == p[0].startswith('tile')
    assert sorted({p[0] for p in plan.values()}) == sorted(rc.BIL.values()), 'not all six forms are reached'
    # both grid-wrap cases have more planes than one grid row of 65535 holds
    assert all(rc.BY_ID[c].shape[0] > 65535 for c in ('bilinear-wrap-tile', 'bilinear-wrap-generic', 'avgpool-wrap'))
    assert {rc.plan(c) for c in rc.CASES if c.op == 'avgpool'} == {'vec', 'plain'}


@pytest.mark.parametrize('cid', BRANCH)
def test_branch_seams(cid):
    case = rc.BY_ID[cid]
    N, P, h, w = case.shape
    sizes = rc.sizes_of(case)
    p = rc.branch_plan(N, P, h, w, sizes, aligned8=not case.cfg.get('misalign'))
    cfg = case.cfg
    assert rc.branch_fits(N, P, h, w, sizes) == (case.form != 'unsupported')
    if p.form in ('stream3', 'stream'):
        assert p.ncb == -(-w // 124) and p.nseg == -(-h // p.seg) and 0 < p.seg <= 19 and (p.tiles_x, p.tiles_y) == (0, 0)
        assert all(t in (3, 5) for t in p.taps[:len(sizes)]) and all(t == 0 for t in p.taps[len(sizes):])
    if p.form == 'tile':
        assert (p.tiles_x, p.tiles_y) == (-(-w // 32), -(-h // 16)) and (p.ncb, p.nseg, p.seg) == (0, 0, 0)
    if p.form == 'unsupported':
        assert p[1:] == (0, 0, 0, (0, 0, 0), 0, 0)
    for key in ('ncb', 'seg', 'nseg'):
        if key in cfg:
            assert getattr(p, key) == cfg[key], (key, p)
    if 'nseg_min' in cfg:
        assert p.nseg >= cfg['nseg_min']
    if 'tiles' in cfg:
        assert (p.tiles_x, p.tiles_y) == cfg['tiles']
    if 'taps' in cfg:
        assert p.taps[:2] == cfg['taps']
    # the up-scales give the tap counts the table says: 2.0 and 3.0 three taps, 1.5, 1.25 and 2.5 five
    if p.form in ('stream3', 'stream'):
        for s, sz, t in zip(cfg['scales'], sizes, p.taps):
            if sz == (math.ceil(h * s), math.ceil(w * s)):              # (not where the floor of 5 changes the ratio: 4 -> 5 columns)
                assert t == (3 if s in (1.0, 2.0, 3.0) else 5), (s, t)


def test_branch_table_coverage():
    plans = {c: rc.branch_plan(*rc.BY_ID[c].shape, rc.sizes_of(rc.BY_ID[c]), aligned8=not rc.BY_ID[c].cfg.get('misalign')) for c in BRANCH}
    assert {p.form for p in plans.values()} == {'stream3', 'stream', 'tile', 'unsupported'}
    s3 = [(c, p) for c, p in plans.items() if p.form == 'stream3']
    # every tap pair of the one-launch form, with and without the trailing same-size branch; one up branch, both ways
    got = {(p.taps[:2], len(rc.BY_ID[c].cfg['scales']) == 3) for c, p in s3 if len(rc.BY_ID[c].cfg['scales']) - (rc.BY_ID[c].cfg['scales'][-1] == 1.0) == 2}
    assert got == {(t, s) for t in ((3, 3), (5, 5), (5, 3), (3, 5)) for s in (False, True)}, got
    one = {(p.taps[0], rc.BY_ID[c].cfg['scales'][-1] == 1.0) for c, p in s3 if len(rc.BY_ID[c].cfg['scales']) - (rc.BY_ID[c].cfg['scales'][-1] == 1.0) == 1}
    assert {(3, False), (3, True)} <= one
    assert max(p.ncb for _, p in s3) >= 2 and any(p.seg == 19 and p.nseg >= 2 for _, p in s3)
    assert any(p.form == 'stream' and p.ncb >= 2 for p in plans.values())
    assert max(p.tiles_x for p in plans.values()) >= 2 and max(p.tiles_y for p in plans.values()) >= 2
    assert {rc.BY_ID[c].cfg['adds'] for c, _ in s3} == {0, 1, 2}


def test_plans_reject_what_the_launchers_reject():
    f = ctypes.c_int32()
    lib = nv.lib
    assert lib.mspl_bilinear_bwd_plan(1, 2, 0, 4, 8, 8, 1, ctypes.byref(f), None, None, None, None) == nv.ERR_BAD_SHAPE
    assert lib.mspl_bilinear_bwd_plan(1, 2, 4, 4, 8, 8, 1, None, None, None, None, None) == nv.ERR_NULL_POINTER
    assert lib.mspl_bilinear_bwd_plan(1, 2, 4, 4, 8, 8, 1, ctypes.byref(f), None, None, None, None) == 0          # the rest is optional
    assert lib.mspl_avgpool3x3s2_bwd_plan(1, 2, 0, 8, 1, ctypes.byref(f)) == nv.ERR_BAD_SHAPE
    assert lib.mspl_avgpool3x3s2_bwd_plan(1, 2, 70000, 300, 1, ctypes.byref(f)) == nv.ERR_BAD_SHAPE              # H * W * W >= 2^32
    hs, ws = (ctypes.c_int32 * 1)(20), (ctypes.c_int32 * 1)(24)
    assert lib.mspl_pyrpool_branch_bwd_plan(1, 4, 10, 12, 1, hs, ws, 1, None, None, None, None, None, None, None) == nv.ERR_NULL_POINTER
    assert lib.mspl_pyrpool_branch_bwd_plan(1, 4, 10, 12, 1, hs, ws, 1, ctypes.byref(f), None, None, None, None, None, None) == 0
    assert f.value == nv.PYR_BRANCH_BWD_STREAM3
    for nb in (0, 4):                                                                                            # 1..3 branches
        assert lib.mspl_pyrpool_branch_bwd_plan(1, 4, 10, 12, nb, hs, ws, 1, ctypes.byref(f), None, None, None, None, None, None) == 0
        assert f.value == nv.PYR_BRANCH_BWD_UNSUPPORTED


@pytest.mark.parametrize('cid', LINEAR)
def test_probe_sets_are_valid(cid):
    """From the float64 operator alone: within one probe plane no input element receives from two hot outputs, every hot output's
    receivers are owned by it, and every output is hot exactly once."""
    case = rc.BY_ID[cid]
    Ho, Wo = rc.out_shape(case)
    for k, (Hi, Wi) in enumerate(rc.in_shapes(case)):
        if case.shape[0] > 65535:
            continue                                            # full basis (Ho * Wo <= 9), repeated over the planes
        pr = rc.bwd_probes(cid, k)
        planes = pr.hot.shape[0]
        assert pr.owner.shape == (planes, Hi * Wi)
        live = pr.hot >= 0
        assert torch.equal(torch.bincount(pr.hot[live], minlength=Ho * Wo), torch.ones(Ho * Wo, dtype=torch.int64)), \
            'an output is hot in no plane or in several'
        if Ho * Wo <= rc.FULL_BASIS:
            assert planes == Ho * Wo
        plane_of = torch.empty(Ho * Wo, dtype=torch.int64)                      # the plane in which output o is hot
        plane_of[pr.hot[live]] = torch.arange(planes)[:, None].expand_as(pr.hot)[live]
        A = rc.dense_operator(case, k) != 0                                     # (Ho*Wo, Hi*Wi)
        o_idx, i_idx = torch.nonzero(A, as_tuple=True)
        # how many hot outputs of its plane reach each input
        reach = torch.bincount(plane_of[o_idx] * (Hi * Wi) + i_idx, minlength=planes * Hi * Wi)
        assert int(reach.max()) <= 1, '%s: %d hot elements of one plane share a receiver' % (cid, int(reach.max()))
        # ... and each reached input is owned by exactly that output
        assert torch.equal(pr.owner[plane_of[o_idx], i_idx], o_idx)
        # the axis operators the colouring used are the operator's factors
        Ay, Ax = rc.axis_operator(case, k, 0), rc.axis_operator(case, k, 1)
        assert torch.equal(torch.kron(Ay != 0, Ax != 0), A)


RECORD = {}


@pytest.mark.parametrize('cid', IDS)
def test_float32_reference_is_finite(cid):
    case = rc.BY_ID[cid]
    if case.form == 'unsupported':
        return
    for name, r in rc.refs(cid).items():
        assert torch.isfinite(r.r64).all() and torch.isfinite(r.err32).all() and torch.isfinite(r.mag).all(), (cid, name)
        assert bool((r.bound > 0).all()) or float(r.mag.max()) == 0.0
        assert bool((rc.plane_max(name, r.r64) <= r.mag * (1 + 1e-12)).all()), '%s %s: the magnitude evaluation is not a bound' % (cid, name)
        unit = r.err32 / (rc.EPS * r.mag).clamp_min(1e-300)
        RECORD[(cid, name)] = float(unit.max())
        # the float32 CPU evaluation itself stays within a few hundred roundings of the magnitude: a gap beyond that is a
        # broken reference, not a tolerance unit
        assert float(unit.max()) < 512, '%s %s: float32 CPU is %.0f x 2^-23 x M away from float64' % (cid, name, float(unit.max()))
    print('%s: err32 / (2^-23 M) = %s' % (cid, {n: '%.2f' % RECORD[(cid, n)] for n in rc.refs(cid)}))
