"""The compile command the Makefile of mspl_amd/csrc gives each .hip file, read from `make -n`: the one source of the per-file flags
(-fno-slp-vectorize and friends) for the tools that compile kernels on their own (kernel_isa_diff.py, resource_audit.py)."""
import os
import shlex
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join('mspl_amd', 'csrc')


def compile_lines(tree=ROOT):
    """{file.hip: argv} of the Makefile's compile commands in `tree`."""
    txt = subprocess.run(['make', '-n', '-B', '-C', os.path.join(tree, CSRC)], capture_output=True, text=True, check=True).stdout
    out = {}
    for line in txt.splitlines():
        argv = shlex.split(line)
        if '-c' in argv and argv[argv.index('-c') + 1].endswith('.hip'):
            out[argv[argv.index('-c') + 1]] = argv
    return out


def device_only(argv, mode, dst, extra=()):
    """The command with `-c file -o obj` turned into a device-only compilation: mode is '-S' (assembly) or '-c'."""
    argv = list(argv)
    k = argv.index('-c')
    argv[k:k + 2] = ['--cuda-device-only', mode, argv[k + 1]]
    argv[argv.index('-o') + 1] = dst
    return argv + list(extra)
