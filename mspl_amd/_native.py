"""ctypes binding of libmspl_hip.so (the C ABI declared in include/mspl_hip.h).

There is no CPU or eager-PyTorch fallback: if the library is missing the import fails loudly, and
every entry point raises RuntimeError with the library's own error text on a non-zero status --
mirroring the reference's failure mode (a RuntimeError from ATen on a shape mismatch).
"""
import ctypes
import os

# torch first, always: torch carries its own copy of the HIP runtime and this library binds /opt/rocm's.  The two coexist in
# one process only when torch's is loaded first (the order every test and bench.py use); with this library first, the first
# launch from it fails with hipErrorNoDevice (seen with `python __graft_entry__.py smoke`, where build() imports the package
# before anything imported torch).
import torch  # noqa: F401,E402

from ._header import parse  # noqa: E402

_HERE = os.path.dirname(os.path.abspath(__file__))
# (the probes under tools/ point MSPL_HIP_LIB at a `make TUNING=1` / `STAMPS=1` build, libmspl_hip_tuning.so; the product library
# itself reads no environment variable)
LIB_PATH = os.environ.get('MSPL_HIP_LIB') or os.path.join(_HERE, 'lib', 'libmspl_hip.so')

# The header IS the binding: argument and return types, both structs and every constant are read from it here, so a new entry
# point needs its prototype there and its definition in a .hip file, nothing in Python.  (The package is used in-tree only.)
HEADER_PATH = os.path.join(os.path.dirname(_HERE), 'include', 'mspl_hip.h')
with open(HEADER_PATH) as _f:
    SIGNATURES, RESTYPES, _STRUCTS, CONSTANTS = parse(_f.read())      # name -> argtypes, name -> restype, ...

Epilogue = _STRUCTS['mspl_epilogue_t']
TrainRec = _STRUCTS['mspl_train_rec_t']      # one image's outcome of the train transforms' random draws, with its device tables
_EP = ctypes.POINTER(Epilogue)
# MSPL_FILTER_LANCZOS -> FILTER_LANCZOS, MSPL_ERR_UNSUPPORTED -> ERR_UNSUPPORTED, MSPL_WGRAD_*, MSPL_LAUNCH_*, MSPL_ABI_VERSION, ...
globals().update(CONSTANTS)


def _load():
    if not os.path.isfile(LIB_PATH):
        raise ImportError(
            'mspl_amd: %s not found. Build it with `python -c "import __graft_entry__ as g; g.build()"` or '
            '`make -C mspl_amd/csrc` (hipcc --offload-arch=gfx950). There is no CPU fallback.' % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = RESTYPES[name]
    # the library was built from the header read above?
    if lib.mspl_abi_version() != CONSTANTS['ABI_VERSION']:
        raise ImportError('mspl_amd: %s has ABI revision %d, %s says revision %d: rebuild the library (make -C mspl_amd/csrc)'
                          % (LIB_PATH, lib.mspl_abi_version(), HEADER_PATH, CONSTANTS['ABI_VERSION']))
    return lib


lib = _load()


def last_error():
    buf = ctypes.create_string_buffer(512)
    lib.mspl_last_error(buf, 512)
    return buf.value.decode()


def check(status):
    if status != 0:
        raise RuntimeError('mspl_hip (%d): %s' % (status, last_error()))


def version():
    return lib.mspl_version().decode()
