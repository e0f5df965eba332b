#!/usr/bin/env python3
"""Generate tests/golden/pyr_plans.json: what the pyramid kernels' host-side plan queries answer over the sweep of
tests/pyr_plan_cases.py.  To be run ONCE, on the commit whose decisions are to be kept (its hash is recorded), with the library built:

    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/make_pyr_plans_golden.py

Per query the file holds the distinct answers (`unique`) and, per record of the sweep, the position of its answer (`index`).
Nothing is written unless the sweep holds both sides of every decision the queries report: the streaming forward taken and declined,
all four tap pairs, one and two columns per lane, one and two column blocks, every mspl_pyr_branch_bwd_form_t, `fits` 0 and 1 of
both `fits` queries, prologue LDS bytes zero and positive.  Only data is written."""
import hashlib
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import pyr_plan_cases as S     # noqa: E402


def main():
    recs = S.records()
    got = [S.answers(r) for r in recs]
    plans = [a['stream_plan'] for a in got]
    taken = [p for p in plans if p[0]]
    need = {
        'stream plan taken and declined': {p[0] for p in plans} == {0, 1},
        'all four tap pairs': {(p[1], p[2]) for p in taken} == {(3, 3), (3, 5), (5, 3), (5, 5)},
        'both PXL': {p[3] for p in taken} == {1, 2},
        'ncb 1 and 2': {1, 2} <= {p[4] for p in taken},
        'table bytes zero and positive': {a['tables_bytes'][0] > 0 for a in got} == {False, True},
        'train_fits 0 and 1': {a['train_fits'][0] for a in got} == {0, 1},
        'prep LDS bytes zero and positive': {v > 0 for a in got for v in a['prep_lds']} == {False, True},
    }
    forms, fits = set(), set()
    for a in got:
        b = a['branch_bwd']
        for k in range(0, len(b), S.BWD_STRIDE):
            forms |= {b[k], b[k + 9]}
            fits.add(b[k + 18])
    need['every branch-backward form'] = forms == set(S.FORM_ID.values())
    need['branch_bwd_fits 0 and 1'] = fits == {0, 1}
    missing = [k for k, ok in need.items() if not ok]
    if missing:
        sys.exit('the sweep does not hold both sides of: ' + '; '.join(missing))
    head = subprocess.check_output(['git', '-C', ROOT, 'rev-parse', 'HEAD'], text=True).strip()
    dirty = subprocess.check_output(['git', '-C', ROOT, 'status', '--porcelain', '--', 'mspl_amd', 'include'], text=True).strip()
    if dirty:
        sys.exit('the library sources differ from %s: commit or stash first\n%s' % (head, dirty))
    doc = {'parent': head, 'records': len(recs), 'sweep_sha1': hashlib.sha1(repr(recs).encode()).hexdigest()}
    for q in S.QUERIES:
        uniq = sorted({a[q] for a in got})
        pos = {u: i for i, u in enumerate(uniq)}
        doc[q] = {'unique': uniq, 'index': [pos[a[q]] for a in got]}
    path = os.path.join(HERE, 'pyr_plans.json')
    with open(path, 'w') as f:
        json.dump(doc, f, separators=(',', ':'))
        f.write('\n')
    size = os.path.getsize(path)
    assert size < 100 * 1024, '%d bytes' % size
    print('wrote', path, size, 'bytes,', len(recs), 'records;', {q: len(doc[q]['unique']) for q in S.QUERIES})


if __name__ == '__main__':
    main()
