#!/usr/bin/env python3
"""Launch-by-launch table of one steady-state label pass from a rocprofv3 kernel trace, and the time per kernel name.
Usage: python tools/pass_table.py <kernel_trace.csv> <out.txt>; the collecting command (GPU box):
  rocprofv3 --kernel-trace --stats -d DIR -o pp --output-format csv -- python3 bench.py --profile-pass --in-flight 1 --no-graph --steps 6 --warmup 2"""
import csv, sys, collections
rows = list(csv.DictReader(open(sys.argv[1])))
rows.sort(key=lambda r: int(r['Start_Timestamp']))
marks = [i for i, r in enumerate(rows) if 'label_epilogue' in r['Kernel_Name']]
a, b = marks[len(marks) // 2] + 1, marks[len(marks) // 2 + 1] + 1
out = open(sys.argv[2], 'w')
out.write('one steady-state label pass (batch 16 x 3 x 288 x 480, eager launches, one pass in flight), rocprofv3 --kernel-trace\n\n')
t0 = int(rows[a]['Start_Timestamp'])
tot = 0.0
agg = collections.OrderedDict()
for r in rows[a:b]:
    k = r['Kernel_Name'].replace('void mspl::', '').replace('mspl::', '').split('(')[0][:60]
    s, e = int(r['Start_Timestamp']), int(r['End_Timestamp'])
    tot += (e - s) / 1e3
    agg.setdefault(k, [0, 0.0]); agg[k][0] += 1; agg[k][1] += (e - s) / 1e3
    out.write('%9.1f us  +%7.1f us  %s\n' % ((s - t0) / 1e3, (e - s) / 1e3, k))
out.write('\nlaunches %d, kernel time %.1f us, span %.1f us\n\n' % (b - a, tot, (int(rows[b - 1]['End_Timestamp']) - t0) / 1e3))
for k, (n, t) in sorted(agg.items(), key=lambda kv: -kv[1][1]):
    out.write('%3d x %-60s %8.1f us\n' % (n, k, t))
out.close()
print(open(sys.argv[2]).read()[-2500:])
