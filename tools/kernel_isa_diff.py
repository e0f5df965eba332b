#!/usr/bin/env python3
"""Do the kernels of the library compile to the same code as at another revision?  For a refactor that must not touch device code.

    python tools/kernel_isa_diff.py REV [file.hip ...]        (default: every .hip of mspl_amd/csrc, on both sides)

mspl_amd/csrc and include of REV are extracted into a temporary directory; each file is compiled there and in the working tree to
device-only assembly (--cuda-device-only -S) with the flags that tree's own Makefile gives it (tools/build_flags.py).  Kernels are
matched BY SYMBOL across all files of a side, so a kernel may move between files (a named file is compiled on every side that has
it).  Per kernel three texts are compared: the instructions between its label and its .Lfunc_end (comments and blank lines stripped,
the function number inside local labels -- .LBB<n>_<k> -- dropped: it only counts the functions ahead of it in the file), its
.amdhsa_kernel descriptor (registers, LDS, scratch, kernarg size) and its entry in the amdhsa.kernels metadata.  One line per kernel
that differs or exists on one side only, one per kernel that moved, then a count; the exit status is the number of kernels that
differ or exist on one side only (capped at 255).  A symbol defined in two files of one side is an error, except a kernel with
internal linkage (a static one in a shared header), which is matched within its file."""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

from build_flags import CSRC, ROOT, compile_lines, device_only


def assembly(tree, name, argv, dst):
    r = subprocess.run(device_only(argv, '-S', dst), cwd=os.path.join(tree, CSRC), capture_output=True, text=True)
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


def internal_linkage(sym):
    """_ZL<name> or _ZN<len><name>...L<len><name>: walks the length-prefixed components of the nested name."""
    if not sym.startswith('_ZN'):
        return sym.startswith('_ZL')
    k = 3
    while k < len(sym):
        m = re.match(r'\d+', sym[k:])
        if not m:
            return sym[k] == 'L' and sym[k + 1:k + 2].isdigit()
        k += len(m.group(0)) + int(m.group(0))
    return False


def side(tree, label, cmds, files, tmp):
    """{symbol: (file, texts)} over `files` of one side.  A kernel with internal linkage (a static one in a header that several files
    include; its mangled name carries an L before the length) stays with its file, as 'file:symbol'."""
    jobs = [(tree, f, cmds[f], os.path.join(tmp, '%s_%s.s' % (label, f))) for f in files]
    with ThreadPoolExecutor(16) as ex:
        per_file = list(ex.map(lambda j: kernels(assembly(*j)), jobs))
    out = {}
    for f, ks in zip(files, per_file):
        for sym, texts in ks.items():
            if internal_linkage(sym):
                sym = '%s:%s' % (f, sym)
            if sym in out:
                sys.exit('%s: %s is defined in %s and in %s' % (label, sym, out[sym][0], f))
            out[sym] = (f, texts)
    return out


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
        named = [os.path.basename(f) for f in sys.argv[2:]]
        for f in named:
            if f not in cmd_old and f not in cmd_new:
                sys.exit('%s is in neither tree' % f)
        ko = side(old, 'old', cmd_old, sorted(f for f in cmd_old if not named or f in named), tmp)
        kn = side(ROOT, 'new', cmd_new, sorted(f for f in cmd_new if not named or f in named), tmp)
        bad = moved = 0
        for sym in sorted(set(ko) | set(kn)):
            if sym not in ko or sym not in kn:
                f = (ko.get(sym) or kn[sym])[0]
                what = ['only in ' + (rev if sym in ko else 'the working tree')]
            else:
                fo, fn = ko[sym][0], kn[sym][0]
                f = fo if fo == fn else '%s -> %s' % (fo, fn)
                moved += fo != fn
                what = [n for n, a, b in zip(('instructions', 'descriptor', 'metadata'), ko[sym][1], kn[sym][1]) if a != b]
            if what:
                bad += 1
            if what or ' -> ' in f:
                print('%-40s %s: %s' % (f, sym, ', '.join(what) or 'moved, identical'))
        print('%d of %d kernels differ from %s (%d files there, %d here); %d moved to another file' % (
            bad, len(set(ko) | set(kn)), rev, len({v[0] for v in ko.values()}), len({v[0] for v in kn.values()}), moved))
        sys.exit(min(bad, 255))


if __name__ == '__main__':
    main()
