"""The table of tests/label_cases.py, checked without a GPU: (a) the table is sound by the reference alone -- at most 1 % of a
case's pixels are unclear and float32 ATen on the CPU agrees with float64 on every clear pixel; (b) the library's plan query
(mspl_label_epilogue_plan, the host function the launcher itself switches on) confirms that every case reaches the kernel form,
staging mode, instantiation, LDS size and pair count it is in the table for, and that the table as a whole reaches every one of
them; (c) mspl_label_epilogue_hist_fits answers what the plan answers; (d) the magic division of the staged pair index is exact
on the range the launcher's guard keeps it in.  A case whose property is not met FAILS."""
import ctypes
import itertools

import pytest
import torch

from mspl_amd import _native as nv
from mspl_amd import ops
from tests import label_cases as lc


def _plan(case, general=False, aligned=True):
    return ops.label_epilogue_plan(case.shape, general=general, aligned16=aligned)


@pytest.mark.parametrize('name', lc.NAMES)
def test_reference_alone_meets_the_label_rule(name):
    main, aux, size, ref, seed = lc.problem(name)
    print('%s seed %d: unclear %.3f %% (tau %.3e); err32 %s' % (name, seed, 100 * ref['unclear'], ref['tau'],
                                                                  {k: '%.2e' % v for k, v in ref['err32'].items()}))
    assert ref['unclear'] <= lc.UNCLEAR_CAP
    assert torch.equal(ref['labels32'][ref['clear']], ref['labels'][ref['clear']]), 'float32 ATen disagrees with float64 on a clear pixel'
    assert all(torch.isfinite(ref[k]).all() for k in ('prob', 'kld', 'main_up'))
    assert float(ref['kld'].min()) > -1e-12 and (lc.two_heads(lc.BY_NAME[name]) or float(ref['kld'].abs().max()) == 0.0)


@pytest.mark.parametrize('name,mag', lc.TRAINED)
def test_trained_reference_alone_meets_the_label_rule(name, mag):
    main, aux, size, ref, seed = lc.trained_problem(name, mag)
    print('%s m%d seed %d: unclear %.3f %%; max|o| %.1f; err32 %s' % (name, mag, seed, 100 * ref['unclear'], float(ref['o'].abs().max()),
                                                                        {k: '%.2e' % v for k, v in ref['err32'].items()}))
    assert ref['unclear'] <= lc.UNCLEAR_CAP
    assert torch.equal(ref['labels32'][ref['clear']], ref['labels'][ref['clear']])


@pytest.mark.parametrize('name', lc.SINGLE_HEAD)
def test_single_head_reference(name):
    ref = lc.problem(name, single_head=True)[3]
    assert ref['unclear'] <= lc.UNCLEAR_CAP and float(ref['kld'].abs().max()) == 0.0


@pytest.mark.parametrize('name', lc.NAMES)
def test_case_reaches_its_form(name):
    case = lc.BY_NAME[name]
    p = _plan(case)
    want = dict(case.expect)
    big = want.pop('big', None)
    got = {k: p[k] for k in want}
    assert got == want, '%s (%s): the library plans %s' % (name, case.why, p)
    N, C, Hm, Wm, Ha, Wa, H, W = case.shape
    if p['form'] == 'lds':
        assert (p['lds_bytes'] > lc.LDS_64K) == big and p['lds_bytes'] <= 128 * 1024
        assert p['lds_bytes'] == 4 * (p['nrm'] * C * p['wms'] + p['nra'] * C * p['was'] + 32)
        assert (p['pairs_main'], p['pairs_aux']) == (p['nrm'] * C, p['nra'] * C) and p['pairs_main'] + p['pairs_aux'] < 4096
        assert p['wms'] % 4 == 0 and p['was'] % 4 == 0 and p['wms'] <= 256 and p['was'] <= 256
        assert p['bands'] == -(-H // 4) and p['rowslots'] == 4 * -(-p['bands'] // 4)
    elif p['form'] == 'register':
        assert p['bands'] == H and p['rowslots'] == 4 * -(-H // 4) and p['vec'] == p['lds_bytes'] == 0
    assert p['colblocks'] == -(-W // 256)
    # asking for probabilities or up-sampled logits always takes the general kernel
    g = _plan(case, general=True)
    assert g['form'] == 'general' and all(v == 0 for k, v in g.items() if k != 'form')
    # pointers that are not 16-byte aligned: 4-byte staging, never a wider tile
    u = _plan(case, aligned=False)
    assert u['vec'] == 0
    if p['form'] == 'lds':
        assert u['form'] == 'lds' and u['wms'] <= p['wms'] and u['was'] <= p['was'] and u['cmax'] == p['cmax']
    if case.offset:
        assert p['vec'] == 1, 'the shape alone must allow 16-byte staging: the pointers switch it off'


def test_table_reaches_every_form_and_instantiation():
    plans = {c.name: _plan(c) for c in lc.CASES}
    lds = [p for p in plans.values() if p['form'] == 'lds']
    assert {p['form'] for p in plans.values()} == {'register', 'lds'}          # (general: every case, asked with general=True)
    assert {p['vec'] for p in lds} == {0, 1}
    assert {(p['cmax'], p['exact']) for p in lds} == {(5, 1), (13, 1), (20, 1), (8, 0), (16, 0), (24, 0)}
    assert {p['wide480'] for p in lds} == {0, 1}
    assert {(p['cmax'], p['wide480']) for p in lds if p['wide480']} == {(5, 1), (13, 1), (20, 1)}
    assert {p['lds_bytes'] > lc.LDS_64K for p in lds} == {False, True}
    assert {(p['cmax'], p['lds_bytes'] > lc.LDS_64K) for p in lds if p['exact']} >= {(13, True)}, 'an EXACT instantiation above 64 KB'
    assert {p['cmax'] for p in plans.values() if p['form'] == 'register'} == {8, 16, 24}
    assert max(p['pairs_main'] + p['pairs_aux'] for p in lds) == 4080
    assert any(p['wms'] == 256 for p in lds)
    # wide480 with one head and with two; a wide480 shape whose class count has no such instantiation stays on the runtime strides
    assert plans['wide480_c13_1head']['was'] == 4
    assert ops.label_epilogue_plan((1, 8, 10, 240, 5, 120, 19, 480))['wide480'] == 0
    assert ops.label_epilogue_plan((1, 25, 10, 240, 5, 120, 19, 480))['form'] == 'general'      # more than 24 classes


def _hist_fits(shape):
    return bool(nv.lib.mspl_label_epilogue_hist_fits(*[int(v) for v in shape]))


def test_hist_fits_is_the_plan():
    for c in lc.CASES:
        assert _hist_fits(c.shape) == (_plan(c)['form'] == 'lds'), c.name
    n = 0
    sweep = itertools.product((1, 3), (1, 5, 8, 13, 17, 24, 25), (1, 7, 40, 300), (1, 30, 64, 130, 257, 520), (0, 1), (3, 16, 61), (1, 85, 256, 260, 480))
    for N, C, Hm, Wm, two, H, W in sweep:
        shape = (N, C, Hm, Wm, (Hm + 1) // 2 if two else 0, (Wm + 1) // 2 if two else 0, H, W)
        a, u = ops.label_epilogue_plan(shape), ops.label_epilogue_plan(shape, aligned16=False)
        assert _hist_fits(shape) == (a['form'] == 'lds'), shape
        assert a['form'] != 'lds' or u['form'] == 'lds', shape           # 4-byte staging never needs more room
        n += 1
    assert n > 300
    # shapes the launcher refuses answer 0 / an error, never a plan
    assert not _hist_fits((0, 5, 8, 8, 4, 4, 16, 16)) and not _hist_fits((1, 5, 8, 8, -1, 4, 16, 16))
    out = (ctypes.c_int32 * nv.LE_PLAN_LEN)()
    assert nv.lib.mspl_label_epilogue_plan(1, 5, 8, 8, 4, 0, 16, 16, 0, 1, out) == nv.ERR_BAD_SHAPE
    assert nv.lib.mspl_label_epilogue_plan(1, 256, 8, 8, 0, 0, 16, 16, 0, 1, out) == nv.ERR_UNSUPPORTED
    assert nv.lib.mspl_label_epilogue_plan(1, 5, 8, 8, 0, 0, 16, 16, 0, 1, None) == nv.ERR_NULL_POINTER


def test_pair_decode_is_exact_below_the_guard():
    """labels.hip decodes a staged (row, class) pair index as row = (pair * magc) >> 16 with magc = ceil(65536 / C), for
    pair < (nrm + nra) * C < 4096 and C <= 24.  The invariant that guard protects: the decode equals pair // C on that whole range.
    C = 17 is the tightest (4095 * 16 = 65520 < 65536); at 8192 pairs it is already wrong, which is what a relaxed guard would admit."""
    for C in range(1, 25):
        magc = (65536 + C - 1) // C
        assert magc * C - 65536 < C
        for pair in range(4096):
            assert (pair * magc) >> 16 == pair // C, (C, pair)
    wrong = [C for C in range(1, 25) if any((pair * ((65536 + C - 1) // C)) >> 16 != pair // C for pair in range(4096, 8192))]
    assert 17 in wrong
    # the lane decode of the 16-byte staging: lane // cq for lane < 64 and every chunk count a staged row can have (cq <= 64)
    for cq in range(1, 65):
        mag = ((1 << 20) + cq - 1) // cq
        assert all((lane * mag) >> 20 == lane // cq for lane in range(64)), cq
    # the table's pair counts stay under the guard, the one case meant to cross it does
    over = lc.BY_NAME['pairs_over']
    N, C, Hm, Wm, Ha, Wa, H, W = over.shape
    p15 = ops.label_epilogue_plan((N, 15, Hm, Wm, Ha, Wa, H, W))          # the same geometry with fewer classes fits
    rows = (p15['pairs_main'] + p15['pairs_aux']) // 15
    assert p15['form'] == 'lds' and rows * 15 < 4096 <= rows * 16 and (p15['wms'], p15['was']) == (4, 4)
    assert ops.label_epilogue_plan((N, 16, Hm, Wm, Ha, Wa, H, W))['form'] == 'register'
    assert _plan(over)['form'] == 'register' and 4 * (rows * C * 4 + 32) <= 128 * 1024, 'only the pair guard can have refused it'


@pytest.mark.parametrize('P', lc.PLANES_P)
def test_planes_cases(P):
    """Every LDS case is served by the planes entry at every plane count, and its reference meets the label rule by itself."""
    served = 0
    for c in lc.CASES:
        N, C, Hm, Wm, Ha, Wa, H, W = c.shape
        fits = bool(nv.lib.mspl_label_epilogue_planes_fits(N, P, C, Hm, Wm, Ha, Wa, H, W))
        assert fits == (c.expect['form'] == 'lds'), c.name
        if not fits:
            continue
        served += 1
        ref = lc.planes_problem(c.name, P)[3]
        assert ref['unclear'] <= lc.UNCLEAR_CAP, c.name
        assert torch.equal(ref['labels32'][ref['clear']], ref['labels'][ref['clear']]), c.name
    assert served >= 1
    assert not nv.lib.mspl_label_epilogue_planes_fits(1, P + 1, 13, 8, 12, 4, 6, 16, 24)


def test_merge_reference_is_the_oracle():
    """The numpy statement of the merge contract equals the oracle's merge_outputs wherever a policy of the reference exists."""
    import numpy as np
    from oracle import labels as olab
    for S in lc.MERGE_S:
        src = lc.merge_sources(S, 5, 4099)
        assert (src >= 5).mean() > 0.05, 'labels outside the classes'
        # ('none' is no rule of its own in merge_outputs: any name but 'all' takes the majority threshold of 'half', uest_seg_multi_os.py:697-705;
        # a threshold of 1 is reached as the integer 1)
        for policy, thresh in (('all', S), ('half', S // 2 + 1), ('none', S // 2 + 1), (1, 1)):
            out, hist = lc.merge_reference(src, 5, thresh, olab.NO_AGREEMENT_CLASS)
            np.testing.assert_array_equal(out, olab.merge_outputs(src, 5, policy))
            np.testing.assert_array_equal(hist, olab.class_histogram(out).astype(np.int64))
        if S % 2 == 0:        # the engineered ties: the first source holds the HIGHER class, the first maximum is the lower one
            tie = np.arange(4099) % 3 == 0
            out = lc.merge_reference(src, 5, 1, 255)[0]
            assert (out[tie] == src[S - 1][tie]).all() and (src[0][tie] > src[S - 1][tie]).all()
