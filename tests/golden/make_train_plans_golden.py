#!/usr/bin/env python3
"""Generate tests/golden/train_plans.json: what the plan queries of the convolution weight gradient, the bilinear backward and the
avg-pool backward answer over the sweep of tests/train_plan_cases.py.  To be run ONCE, on the commit whose decisions are to be kept
(its hash is recorded), with the library built:

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_train_plans_golden.py

Per query the file holds the distinct answers (`unique`) and, per record of the sweep, the position of its answer (`index`).
Nothing is written unless every enumerator of mspl_wgrad_form_t, mspl_bilinear_bwd_form_t and mspl_avgpool_bwd_form_t occurs in the
answers, the weight gradient is split into 1, 2 and more parts in every form that splits, and the tile forms answer one and
several tiles each way.  What no query can reach is printed with its reason (train_plan_cases.UNREACHABLE).  Only data is written."""
import hashlib
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from mspl_amd import _native as nv        # noqa: E402
from tests import train_plan_cases as S   # noqa: E402


def main():
    recs = S.records()
    got = {q: [S.answers(q, r) for r in recs[q]] for q in S.QUERIES}
    wg, bl, av = got['wgrad'], got['bilinear'], got['avgpool']
    tiles = [a for a in bl if a[0] in (nv.BILINEAR_BWD_TILE8, nv.BILINEAR_BWD_TILE12)]
    need = {
        'every mspl_wgrad_form_t': {a[0] for a in wg} == S.WGRAD_FORMS,
        'every mspl_bilinear_bwd_form_t': {a[0] for a in bl} == S.BILINEAR_FORMS,
        'every mspl_avgpool_bwd_form_t': {a[0] for a in av} == S.AVGPOOL_FORMS,
        'both tile forms with one and several tiles each way': all(
            {min(a[k], 2) for a in tiles if a[0] == f} == {1, 2} for f in (nv.BILINEAR_BWD_TILE8, nv.BILINEAR_BWD_TILE12) for k in (1, 2)),
        'avg-pool query at the 32-bit limit': [S.avgpool_edge(s) for s, _ in S.AVGPOOL_EDGE] == [rc for _, rc in S.AVGPOOL_EDGE],
    }
    for f in S.WGRAD_FORMS - {nv.WGRAD_1X1_MFMA}:
        need['1, 2 and more parts in weight-gradient form %d' % f] = {min(a[1], 4) for a in wg if a[0] == f} >= {1, 2, 4}
    missing = [k for k, ok in need.items() if not ok]
    if missing:
        sys.exit('the sweep does not hold: ' + '; '.join(missing))
    for what, why in S.UNREACHABLE.items():
        print('not reachable from a plan query: %s (%s)' % (what, why))
    head = subprocess.check_output(['git', '-C', ROOT, 'rev-parse', 'HEAD'], text=True).strip()
    dirty = subprocess.check_output(['git', '-C', ROOT, 'status', '--porcelain', '--', 'mspl_amd', 'include'], text=True).strip()
    if dirty:
        sys.exit('the library sources differ from %s: commit or stash first\n%s' % (head, dirty))
    doc = {'parent': head, 'records': {q: len(recs[q]) for q in S.QUERIES},
           'sweep_sha1': hashlib.sha1(repr(sorted(recs.items())).encode()).hexdigest()}
    for q in S.QUERIES:
        uniq = sorted(set(got[q]))
        pos = {u: i for i, u in enumerate(uniq)}
        doc[q] = {'unique': uniq, 'index': [pos[a] for a in got[q]]}
    path = os.path.join(HERE, 'train_plans.json')
    with open(path, 'w') as f:
        json.dump(doc, f, separators=(',', ':'))
        f.write('\n')
    size = os.path.getsize(path)
    assert size <= os.path.getsize(os.path.join(HERE, 'pyr_plans.json')), '%d bytes' % size
    print('wrote', path, size, 'bytes;', {q: (len(recs[q]), len(doc[q]['unique'])) for q in S.QUERIES})


if __name__ == '__main__':
    main()
