#!/usr/bin/env python3
"""Do the kernels of a .hip file compile to the same code as at another revision?  For a refactor that must not touch device code.

    python tools/kernel_isa_diff.py REV [file.hip ...]        (default: every .hip of mspl_amd/csrc)

mspl_amd/csrc and include of REV are extracted into a temporary directory; each file is compiled there and in the working tree to
device-only assembly (--cuda-device-only -S) with the flags that tree's own Makefile gives it (read from `make -n`).  Per kernel
three texts are compared: the instructions between its label and its .Lfunc_end (comments and blank lines stripped, the function
number inside local labels -- .LBB<n>_<k> -- dropped: it only counts the functions ahead of it in the file), its .amdhsa_kernel
descriptor (registers, LDS, scratch, kernarg size) and its entry in the amdhsa.kernels metadata.  One line per kernel that differs
or exists on one side only, then a count; the exit status is the number of such kernels (capped at 255)."""
import os
import re
import shlex
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join('mspl_amd', 'csrc')


def compile_lines(tree):
    """{file.hip: argv} of the Makefile's compile commands in `tree`."""
    txt = subprocess.run(['make', '-n', '-B', '-C', os.path.join(tree, CSRC)], capture_output=True, text=True, check=True).stdout
    out = {}
    for line in txt.splitlines():
        argv = shlex.split(line)
        if '-c' in argv and argv[argv.index('-c') + 1].endswith('.hip'):
            out[argv[argv.index('-c') + 1]] = argv
    return out


def assembly(tree, name, argv, dst):
    argv = list(argv)
    k = argv.index('-c')
    argv[k:k + 2] = ['--cuda-device-only', '-S', name]
    argv[argv.index('-o') + 1] = dst
    r = subprocess.run(argv, cwd=os.path.join(tree, CSRC), capture_output=True, text=True)
    if r.returncode:
        sys.exit('%s in %s:\n%s' % (name, tree, r.stderr[-4000:]))
    with open(dst) as f:
        return f.read()


def kernels(asm):
    """{symbol: (instructions, descriptor, metadata)}"""
    lines = asm.splitlines()
    desc, k = {}, 0
    while k < len(lines):
        m = re.match(r'\s*\.amdhsa_kernel\s+(\S+)', lines[k])
        if m:
            e = next(i for i in range(k, len(lines)) if lines[i].strip() == '.end_amdhsa_kernel')
            desc[m.group(1)] = '\n'.join(s.split(';')[0].strip() for s in lines[k + 1:e])
            k = e
        k += 1
    body = {}
    for sym in desc:
        a = next(i for i, s in enumerate(lines) if s.startswith(sym + ':'))
        e = next(i for i in range(a, len(lines)) if lines[i].startswith('.Lfunc_end'))
        code = [s.split(';')[0].strip() for s in lines[a + 1:e]]
        body[sym] = re.sub(r'\.LBB\d+_', '.LBB_', '\n'.join(s for s in code if s))
    meta = {}
    a = next((i for i, s in enumerate(lines) if s.strip() == 'amdhsa.kernels:'), None)
    if a is not None:
        e = next(i for i in range(a + 1, len(lines)) if not lines[i].startswith('  '))
        for chunk in re.split(r'\n(?=  - )', '\n'.join(lines[a + 1:e])):
            m = re.search(r'^\s+\.name:\s+(\S+)', chunk, re.M)
            if m:
                meta[m.group(1)] = chunk
    return {s: (body[s], desc[s], meta.get(s, '')) for s in desc}


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    rev = sys.argv[1]
    with tempfile.TemporaryDirectory() as tmp:
        old = os.path.join(tmp, 'rev')
        os.mkdir(old)
        tar = subprocess.run(['git', '-C', ROOT, 'archive', rev, CSRC, 'include'], capture_output=True, check=True).stdout
        subprocess.run(['tar', '-x', '-C', old], input=tar, check=True)
        cmd_old, cmd_new = compile_lines(old), compile_lines(ROOT)
        files = [os.path.basename(f) for f in sys.argv[2:]] or sorted(set(cmd_old) | set(cmd_new))
        jobs = []
        for f in files:
            if f not in cmd_old or f not in cmd_new:
                print('%-24s only in %s' % (f, 'the working tree' if f in cmd_new else rev))
                continue
            jobs.append((old, f, cmd_old[f], os.path.join(tmp, 'old_' + f + '.s')))
            jobs.append((ROOT, f, cmd_new[f], os.path.join(tmp, 'new_' + f + '.s')))
        with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
            asm = list(ex.map(lambda j: kernels(assembly(*j)), jobs))
        bad = total = 0
        for k in range(0, len(jobs), 2):
            f, ko, kn = jobs[k][1], asm[k], asm[k + 1]
            for sym in sorted(set(ko) | set(kn)):
                total += 1
                if sym not in ko or sym not in kn:
                    what = ['only in ' + (rev if sym in ko else 'the working tree')]
                else:
                    what = [n for n, a, b in zip(('instructions', 'descriptor', 'metadata'), ko[sym], kn[sym]) if a != b]
                if what:
                    bad += 1
                    print('%-24s %s: %s' % (f, sym, ', '.join(what)))
        print('%d of %d kernels in %d files differ from %s' % (bad, total, len(jobs) // 2, rev))
        sys.exit(min(bad, 255))


if __name__ == '__main__':
    main()
