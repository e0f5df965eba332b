"""mspl_pyrpool_stream_plan -- the host function the streaming pyramid kernel's launcher switches on -- says that the cases of
tests/pyr_stream_cases.py reach every seam of the geometry-table path, and that the table path takes no shape the launcher used to
leave to the other kernel forms.  No GPU: the query looks at shapes only."""
import ctypes

import pytest

from mspl_amd import _native as nv
from mspl_amd import ops
from tests import pyr_stream_cases as C


def _plan(name):
    _, N, P, h, w, s0, s1 = C.case(name)
    return ops.pyrpool_stream_plan((N, P, h, w), C.sizes_of(h, w, s0, s1))


PLANS = {c[0]: _plan(c[0]) for c in C.CASES}


def test_every_case_takes_the_streaming_form_with_consistent_numbers():
    for (name, N, P, h, w, _, _), p in zip(C.CASES, PLANS.values()):
        assert p['taken'] == 1, name
        assert p['pxl'] == (1 if w <= 62 else 2) and p['cbw'] == 62 * p['pxl'] and p['ncb'] == -(-w // p['cbw']), name
        for seg, nseg, waves in ((p['seg'], p['nseg'], p['waves']), (p['seg_inkernel'], p['nseg_inkernel'], p['waves_inkernel'])):
            assert nseg == -(-h // seg) and waves == N * P * p['ncb'] * nseg and waves % 4 == 0, name
        assert 1 <= p['seg_inkernel'] <= C.OLD_SEGMAX and 1 <= p['seg'] <= 72, name


def test_both_pxl_forms_and_two_column_blocks():
    assert {p['pxl'] for p in PLANS.values()} == {1, 2}
    assert PLANS['pxl1_24x62']['pxl'] == 1 and PLANS['pxl1_24x62']['ncb'] == 1            # the widest one-column map
    assert PLANS['pxl2_30x64']['pxl'] == 2 and PLANS['pxl2_30x64']['ncb'] == 1
    assert PLANS['pxl2_two_blocks_20x126']['ncb'] == 2 and C.case('pxl2_two_blocks_20x126')[4] > 124


def test_all_four_tap_pairs():
    assert {(p['t0'], p['t1']) for p in PLANS.values()} == {(3, 3), (3, 5), (5, 3), (5, 5)}
    small = {(PLANS[n]['t0'], PLANS[n]['t1']) for n in ('pxl1_40x40', 'pxl1_24x62', 'pxl2_30x64', 'pxl2_two_blocks_20x126')}
    assert small == {(3, 3), (3, 5), (5, 3), (5, 5)}


def test_a_segment_longer_than_the_in_kernel_tables_allow():
    p = PLANS['long_segment_40x40']
    assert p['nseg'] == 1 and p['seg'] == 40 > C.OLD_SEGMAX
    assert p['seg_inkernel'] <= C.OLD_SEGMAX and p['nseg_inkernel'] > 1


def test_a_ragged_last_segment():
    p = PLANS['ragged_73x40']
    h = C.case('ragged_73x40')[3]
    assert p['nseg'] >= 2 and h % p['seg'] != 0 and p['seg'] > C.OLD_SEGMAX


def test_the_batch_changes_the_segment_length():
    _, N, P, h, w, s0, s1 = C.case(C.BATCH_CASE)
    sizes = C.sizes_of(h, w, s0, s1)
    whole, one = ops.pyrpool_stream_plan((N, P, h, w), sizes), ops.pyrpool_stream_plan((1, P, h, w), sizes)
    assert whole['taken'] and one['taken'] and whole['seg'] != one['seg']
    assert (whole['t0'], whole['t1'], whole['pxl'], whole['ncb']) == (one['t0'], one['t1'], one['pxl'], one['ncb'])


DECLINED = [
    ('narrow map', (1, 4, 40, 39), C.sizes_of(40, 39, 2.0, 1.5)),
    ('planes not a multiple of 4', (1, 6, 40, 40), C.sizes_of(40, 40, 2.0, 1.5)),
    ('odd width at two columns per lane', (1, 4, 30, 65), C.sizes_of(30, 65, 2.0, 1.5)),
    ('four branches', (1, 4, 40, 40), C.sizes_of(40, 40, 2.0, 1.5)[:4]),
    ('first branch not up', (1, 4, 40, 40), [(40, 40)] + C.sizes_of(40, 40, 2.0, 1.5)[1:]),
    ('up in one direction only', (1, 4, 40, 40), [(80, 40)] + C.sizes_of(40, 40, 2.0, 1.5)[1:]),
    ('third branch not the map', (1, 4, 40, 40), C.sizes_of(40, 40, 2.0, 1.5)[:2] + [(41, 41)] + C.sizes_of(40, 40, 2.0, 1.5)[3:]),
    ('fourth branch as large as the map', (1, 4, 40, 40), C.sizes_of(40, 40, 2.0, 1.5)[:3] + [(40, 40), (5, 5)]),
    ('fifth branch larger than the map', (1, 4, 40, 40), C.sizes_of(40, 40, 2.0, 1.5)[:4] + [(45, 45)]),
    ('second branch not up', (1, 4, 40, 40), C.sizes_of(40, 40, 2.0, 1.0)),
]


@pytest.mark.parametrize('why,shape,sizes', DECLINED, ids=[d[0] for d in DECLINED])
def test_shapes_the_launcher_declined_stay_declined(why, shape, sizes):
    """Every shape-only reason pyrpool_stream_try had for leaving a launch to the other forms: the plan is all zeros, and no table
    is offered for the geometry where the reason lies in the geometry."""
    p = ops.pyrpool_stream_plan(shape, sizes)
    assert not any(p.values()), (why, p)
    if why != 'planes not a multiple of 4':
        nb = len(sizes)
        hs = (ctypes.c_int32 * nb)(*[s[0] for s in sizes])
        ws = (ctypes.c_int32 * nb)(*[s[1] for s in sizes])
        assert nv.lib.mspl_pyr_stream_tables_bytes(shape[2], shape[3], nb, hs, ws) == 0


def test_table_size():
    for name, N, P, h, w, s0, s1 in C.CASES:
        p = PLANS[name]
        sizes = C.sizes_of(h, w, s0, s1)
        hs = (ctypes.c_int32 * 5)(*[s[0] for s in sizes])
        ws = (ctypes.c_int32 * 5)(*[s[1] for s in sizes])
        want = 4 * (2 * (h + 2) * 24 + 2 * 3 * 5 * (p['ncb'] * 62 + 2) * p['pxl'])
        assert nv.lib.mspl_pyr_stream_tables_bytes(h, w, 5, hs, ws) == want
