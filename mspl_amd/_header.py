"""ctypes view of a C header in the plain-C subset include/mspl_hip.h is written in: prototypes, two structs, enums and
integer #defines.  Regular expressions only; whatever it does not understand raises ImportError instead of being guessed."""
import ctypes
import re

SCALARS = {'int': ctypes.c_int32, 'int32_t': ctypes.c_int32, 'uint32_t': ctypes.c_uint32, 'int64_t': ctypes.c_int64,
           'size_t': ctypes.c_size_t, 'float': ctypes.c_float, 'double': ctypes.c_double}
# what a pointer may point at besides a scalar or a struct of the header (a misspelt type must not pass as "some pointer")
POINTEES = {'void', 'char', 'uint8_t', 'uint16_t', 'unsigned long long'}
TYPED_STRUCT = 'mspl_epilogue_t'      # the one struct callers build themselves and hand over with byref()


def _ctype(decl, where, structs, named):
    """`decl`: a parameter (`named`: its last word is its name), a return type or the type part of a struct field."""
    s, arrays = re.subn(r'\[\s*\d*\s*\]', ' ', re.sub(r'\bconst\b', ' ', decl))
    depth = s.count('*') + arrays
    words = s.replace('*', ' ').split()
    base = ' '.join(words[:-1] if named and len(words) > 1 else words)
    if depth == 0 and base in SCALARS:
        return SCALARS[base]
    if depth in (1, 2) and (base in SCALARS or base in POINTEES or base in structs):
        if depth == 2:
            return ctypes.POINTER(ctypes.c_char_p if base == 'char' else ctypes.c_void_p)
        if base == 'char':
            return ctypes.c_char_p
        # host arrays and device pointers look alike in C: everything else is an address
        return ctypes.POINTER(structs[base]) if base == TYPED_STRUCT else ctypes.c_void_p
    raise ImportError('%s: no ctypes mapping for `%s`' % (where, ' '.join(decl.split())))


def _struct(cname, body, structs):
    fields = []
    for line in filter(None, (f.strip() for f in body.split(';'))):
        m = re.fullmatch(r'(.*?)(\w+(?:\s*,\s*\w+)*)', line, re.S)         # `int32_t sh, sw`: one type, several names
        if not m or not m.group(1).strip():
            raise ImportError('%s: cannot read the field `%s`' % (cname, line))
        ctype = _ctype(m.group(1), cname, structs, named=False)
        fields += [(name.strip(), ctype) for name in m.group(2).split(',')]
    pyname = ''.join(w.capitalize() for w in re.sub(r'^mspl_|_t$', '', cname).split('_'))      # mspl_train_rec_t -> TrainRec
    return type(pyname, (ctypes.Structure,), {'_fields_': fields, '__doc__': cname + '.'})


def parse(text):
    """-> (signatures: name -> argtypes, restypes: name -> restype, structs: C name -> Structure, constants: name without
    its MSPL_ prefix -> int)."""
    code = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)      # comments hold parentheses, semicolons, even calls
    constants = {k: int(v) for k, v in re.findall(r'^[ \t]*#[ \t]*define[ \t]+MSPL_(\w+)[ \t]+(-?\d+)[uU]?[ \t]*$', code, re.M)}
    code = re.sub(r'^[ \t]*#.*$', ' ', code, flags=re.M)

    def enum(m):
        members = [e.strip() for e in m.group(1).split(',') if e.strip()]
        valued = re.findall(r'\bMSPL_(\w+)\s*=\s*(-?\d+)\s*(?:,|$)', m.group(1))
        if len(valued) != len(members):
            raise ImportError('%s: every member needs an explicit integer value' % m.group(2))
        constants.update((k, int(v)) for k, v in valued)
        return ' '
    code = re.sub(r'\btypedef\s+enum\s*\w*\s*\{(.*?)\}\s*(\w+)\s*;', enum, code, flags=re.S)

    structs = {}

    def struct(m):
        structs[m.group(2)] = _struct(m.group(2), m.group(1), structs)
        return ' '
    code = re.sub(r'\btypedef\s+struct\s*\w*\s*\{(.*?)\}\s*(\w+)\s*;', struct, code, flags=re.S)

    signatures, restypes = {}, {}
    for ret, name, params in re.findall(r'([\w\s*]+?)\b(mspl_\w+)\s*\(([^()]*)\)\s*;', code):
        restypes[name] = _ctype(ret, name, structs, named=False)
        params = [] if params.strip() in ('', 'void') else params.split(',')
        signatures[name] = [_ctype(p, name, structs, named=True) for p in params]
    # the plain search the symbol-export test runs: a prototype hidden from the pattern above (an unusual line break, a
    # parameter with parentheses of its own) must not end up silently unbound
    named = set(re.findall(r'\b(mspl_[a-z0-9_]+)\s*\(', text))
    if named != set(signatures):
        raise ImportError('header names %d functions, %d prototypes parsed; unmatched: %s'
                          % (len(named), len(signatures), ', '.join(sorted(named ^ set(signatures)))))
    return signatures, restypes, structs, constants
