"""Every host-side decision of the convolution weight gradient, the bilinear backward and the avg-pool backward that a plan query
reports -- which form takes a shape, into how many parts the reduction is cut, the tile grid and the staged extents -- is what
tests/golden/train_plans.json recorded (tests/golden/make_train_plans_golden.py, at the commit the file names).  It fails when a
limit of a launcher moves.  No GPU: the queries look at shapes only."""
import hashlib
import json
import os

import pytest

from tests import train_plan_cases as S

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'train_plans.json')) as _f:
    GOLD = json.load(_f)
RECORDS = S.records()


def test_the_sweep_is_the_recorded_one():
    assert {q: len(RECORDS[q]) for q in S.QUERIES} == GOLD['records']
    assert hashlib.sha1(repr(sorted(RECORDS.items())).encode()).hexdigest() == GOLD['sweep_sha1']


@pytest.mark.parametrize('query', S.QUERIES)
def test_the_library_answers_what_was_recorded(query):
    want = GOLD[query]
    bad = []
    for rec, k in zip(RECORDS[query], want['index']):
        a = S.answers(query, rec)
        if a != tuple(want['unique'][k]):
            bad.append((rec, a, tuple(want['unique'][k])))
    assert not bad, '%d of %d records differ from %s; first (record, got, recorded): %r' % (
        len(bad), len(RECORDS[query]), GOLD['parent'][:12], bad[0])


def test_every_form_is_in_the_recording():
    assert {u[0] for u in GOLD['wgrad']['unique']} == S.WGRAD_FORMS
    assert {u[0] for u in GOLD['bilinear']['unique']} == S.BILINEAR_FORMS
    assert {u[0] for u in GOLD['avgpool']['unique']} == S.AVGPOOL_FORMS


@pytest.mark.parametrize('shape,rc', S.AVGPOOL_EDGE)
def test_the_avgpool_query_at_the_32_bit_limit(shape, rc):
    assert S.avgpool_edge(shape) == rc
