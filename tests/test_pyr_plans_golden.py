"""Every host-side decision of the pyramid kernels that a plan query reports -- which form takes a shape, its taps, how the planes are
cut, what fits LDS -- is what tests/golden/pyr_plans.json recorded (tests/golden/make_pyr_plans_golden.py, at the commit the file
names).  It fails when a limit of a launcher moves.  No GPU: the queries look at shapes only."""
import hashlib
import json
import os

import pytest

from tests import pyr_plan_cases as S

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pyr_plans.json')) as _f:
    GOLD = json.load(_f)
RECORDS = S.records()


def test_the_sweep_is_the_recorded_one():
    assert len(RECORDS) == GOLD['records']
    assert hashlib.sha1(repr(RECORDS).encode()).hexdigest() == GOLD['sweep_sha1']


@pytest.fixture(scope='module')
def got():
    return [S.answers(r) for r in RECORDS]


@pytest.mark.parametrize('query', S.QUERIES)
def test_the_library_answers_what_was_recorded(got, query):
    want = GOLD[query]
    bad = [(rec, a[query], tuple(want['unique'][k])) for rec, a, k in zip(RECORDS, got, want['index'])
           if a[query] != tuple(want['unique'][k])]
    assert not bad, '%d of %d records differ from %s; first (record, got, recorded): %r' % (
        len(bad), len(RECORDS), GOLD['parent'][:12], bad[0])
