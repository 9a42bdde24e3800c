"""ctypes binding of librnr_hip.so, derived from the C ABI's own declaration, include/rnr_hip.h.

The header is parsed once at import: its `typedef struct` blocks become the ctypes.Structure classes (RnrMesh, RnrConvDesc, ...),
its `#define RNR_X` / `enum` constants the module's integers (the RNR_ prefix dropped: CONV_WINOGRAD, ADAM_CHUNK, ...) and its
prototypes SIGNATURES and PARAMS.  A new entry point is declared there and nowhere here.

The HIP library is the product: there is no CPU fallback.  If the shared object is missing or a symbol
cannot be resolved this module raises — callers never silently route elsewhere.
"""
import collections
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# RNR_HIP_LIB: load another build of the same library (kernel ablation experiments); default is the in-tree build
LIB_PATH = os.environ.get('RNR_HIP_LIB') or os.path.join(os.path.dirname(_HERE), 'librnr_hip.so')
# where csrc/ includes it from: ../../include/rnr_hip.h
HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(_HERE)), 'include', 'rnr_hip.h')


class RnrError(RuntimeError):
    pass


# ---------------------------------------------------------------------------------------------------
# the header as data
# ---------------------------------------------------------------------------------------------------
SCALAR_TYPES = ('int', 'float', 'double', 'size_t', 'long', 'int32_t', 'int64_t', 'uint8_t', 'char', 'void')

# one declared name: a struct field, a parameter or a function (its return type).  pointer: number of `*`; count: array length
Decl = collections.namedtuple('Decl', 'name type pointer count')
# structs: name -> [Decl]; protos: name -> (Decl of the function, [Decl of the parameters]); constants: RNR_X -> int, defines and
# enumerators; enums: the enumerator names of every `enum { }`, in order
Header = collections.namedtuple('Header', 'structs protos constants enums')


def parse_header(text):
    """The C subset rnr_hip.h is written in -> Header.  Strict: whatever is not a comment, an include guard, `#define RNR_X
    <integer expression>`, `enum { }`, `typedef struct x { } x;` or a prototype over SCALAR_TYPES and the header's own structs
    raises RnrError naming the line, rather than being skipped."""
    structs, protos, constants, enums = {}, {}, {}, []

    def fail(pos, why):
        raise RnrError('rnr_hip.h line %d: %s' % (text.count('\n', 0, pos) + 1, why))

    def value(expr, pos):
        if not re.fullmatch(r'[\w\s|&()+\-*<>~]+', expr):
            fail(pos, 'not an integer expression: %r' % expr.strip())
        try:
            v = eval(expr, {'__builtins__': {}}, dict(constants))
        except Exception:
            v = None
        if type(v) is not int:
            fail(pos, 'cannot evaluate %r' % expr.strip())
        return v

    def declare(decl, pos):
        """`[const] type declarator {, declarator}` with declarator = {* | const} name [[length]]"""
        toks = re.findall(r'\w+|\[[^\]]*\]|\S', decl)
        shown = ' '.join(decl.split())
        if toks[:1] == ['const']:
            toks.pop(0)
        if not toks or (toks[0] not in SCALAR_TYPES and toks[0] not in structs):
            fail(pos, 'unknown type in %r' % shown)
        base, out, i = toks[0], [], 1
        while True:
            depth = 0
            while i < len(toks) and toks[i] in ('*', 'const'):
                depth += toks[i] == '*'
                i += 1
            if i == len(toks) or not re.fullmatch(r'[A-Za-z_]\w*', toks[i]) or toks[i] in SCALAR_TYPES or toks[i] in structs:
                fail(pos, 'expected a name in %r' % shown)
            name, count, i = toks[i], None, i + 1
            if i < len(toks) and toks[i][0] == '[':
                count, i = value(toks[i][1:-1], pos), i + 1
            if base == 'void' and not depth:
                fail(pos, 'a void value in %r' % shown)
            out.append(Decl(name, base, depth, count))
            if i == len(toks):
                return out
            if toks[i] != ',':
                fail(pos, 'cannot parse %r' % shown)
            i += 1

    blank = lambda m: re.sub(r'[^\n]', ' ', m.group(0))         # keeps every offset and line number
    code = re.sub(r'//[^\n]*', blank, re.sub(r'/\*.*?\*/', blank, text, flags=re.S))
    # preprocessor lines: the include guard, the includes, the extern "C" bracket and the constants
    cplusplus = False
    for m in list(re.finditer(r'^[^\n]*$', code, flags=re.M)):
        line = m.group(0).strip()
        if cplusplus or line.startswith('#'):
            code = code[:m.start()] + ' ' * len(m.group(0)) + code[m.end():]
        if not line.startswith('#'):
            continue
        if re.fullmatch(r'#\s*ifdef\s+__cplusplus', line):
            cplusplus = True
        elif re.fullmatch(r'#\s*endif', line):
            cplusplus = False
        elif re.fullmatch(r'#\s*(ifndef\s+\w+|define\s+\w+|include\s*<\w+\.h>)', line):
            pass
        else:
            d = re.fullmatch(r'#\s*define\s+(RNR_\w+)\s+(.+)', line)
            if d is None:
                fail(m.start(), 'unsupported preprocessor line %r' % line)
            constants[d.group(1)] = value(d.group(2), m.start())
    # statements: everything up to a `;` outside braces
    start = depth = 0
    for pos, ch in enumerate(code):
        depth += (ch == '{') - (ch == '}')
        if ch != ';' or depth:
            continue
        stmt, at = code[start:pos].strip(), start + len(code[start:pos]) - len(code[start:pos].lstrip())
        start = pos + 1
        s = re.fullmatch(r'typedef\s+struct\s+(\w+)\s*\{(.*)\}\s*(\w+)', stmt, flags=re.S)
        e = re.fullmatch(r'enum\s*\{(.*)\}', stmt, flags=re.S)
        f = re.fullmatch(r'([^()]*?)\b(rnr_\w+)\s*\(([^()]*)\)', stmt, flags=re.S)
        if s is not None:
            if s.group(1) != s.group(3) or s.group(1) in structs:
                fail(at, 'struct %s: tag and typedef name must agree and be new' % s.group(1))
            fields, offset = [], at + stmt.index('{') + 1
            for part in s.group(2).split(';'):
                if part.strip():
                    fields += declare(part, offset + len(part) - len(part.lstrip()))
                offset += len(part) + 1
            structs[s.group(1)] = fields
        elif e is not None:
            names, nxt = [], 0
            for part in e.group(1).split(','):
                n = re.fullmatch(r'\s*(RNR_\w+)\s*(?:=(.*))?', part, flags=re.S)
                if n is None:
                    fail(at, 'cannot parse enumerator %r' % part.strip())
                nxt = constants[n.group(1)] = (value(n.group(2), at) if n.group(2) else nxt)
                nxt += 1
                names.append(n.group(1))
            enums.append(tuple(names))
        elif f is not None and f.group(2) not in protos:
            params = [] if f.group(3).strip() == 'void' else [declare(p, at) for p in f.group(3).split(',')]
            if any(len(p) != 1 or p[0].count is not None for p in params):
                fail(at, 'cannot parse the parameters of %s' % f.group(2))
            protos[f.group(2)] = (declare('%s %s' % (f.group(1), f.group(2)), at)[0], [p[0] for p in params])
        else:
            fail(at, 'not a struct, an enum or an rnr_* prototype: %r' % ' '.join(stmt.split())[:80])
    if code[start:].strip():
        fail(start + len(code[start:]) - len(code[start:].lstrip()), 'unterminated declaration')
    return Header(structs, protos, constants, enums)


try:
    with open(HEADER_PATH) as _f:
        HEADER = parse_header(_f.read())
except OSError as _e:
    raise RnrError('the C ABI declaration %s cannot be read (%s): the binding is derived from it' % (HEADER_PATH, _e))

# ---------------------------------------------------------------------------------------------------
# ... as ctypes
# ---------------------------------------------------------------------------------------------------
_CTYPES = {'int': ctypes.c_int, 'float': ctypes.c_float, 'double': ctypes.c_double, 'size_t': ctypes.c_size_t,
           'long': ctypes.c_long, 'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64, 'uint8_t': ctypes.c_uint8,
           'char': ctypes.c_char}
STRUCTS = {}        # header name -> ctypes.Structure class; also module attributes in CamelCase (rnr_conv_desc -> RnrConvDesc)


def _value_type(d):
    return STRUCTS.get(d.type) or _CTYPES[d.type]


def _field_type(d):             # pointer fields are plain addresses: callers fill them with tensor.data_ptr() or None
    t = ctypes.c_void_p if d.pointer else _value_type(d)
    return t * d.count if d.count else t


for _name, _fields in HEADER.structs.items():
    STRUCTS[_name] = type(''.join(w.capitalize() for w in _name.split('_')), (ctypes.Structure,),
                          {'_fields_': [(d.name, _field_type(d)) for d in _fields]})
globals().update((c.__name__, c) for c in STRUCTS.values())

# RNR_X -> X
CONSTANTS = {k[len('RNR_'):]: v for k, v in HEADER.constants.items()}
globals().update(CONSTANTS)


def _enum_keys(first):          # the enum that starts with RNR_<first>, as lower-case keys without their common prefix
    names = next(e for e in HEADER.enums if e[0] == 'RNR_' + first)
    cut = len(os.path.commonprefix(names))
    return tuple(n[cut:].lower() for n in names)


EMU_FLAGS = {'f32': 0, 'bf16x6': CONSTANTS['CONV_F32_EMU_BF16X6'], 'f16x3': CONSTANTS['CONV_F32_EMU_F16X3']}
# every UNetPlan / RNRPipeline precision -> its descriptor flag: the emulations of fp32 and plain half precision (RNR_CONV_F16)
PRECISION_FLAGS = dict(EMU_FLAGS, f16=CONSTANTS['CONV_F16'])
BN_BWD_MODES = {k: CONSTANTS['BN_BWD_' + k.upper()] for k in _enum_keys('BN_BWD_BATCH')}
PRESENT_MODES = {k: CONSTANTS['PRESENT_' + k.upper()] for k in _enum_keys('PRESENT_FRAME')}
# RNR_METRIC_* outputs, in the order of rnr_image_metrics' out columns
METRIC_KEYS = _enum_keys('METRIC_MAE')

# The one place where the binding does not follow the header: these two tables of rnr_adam_step live in DEVICE memory and are
# passed as integer addresses (tensor.data_ptr()), which a POINTER(struct) argtype refuses.
_ARGTYPE_OVERRIDES = {('rnr_adam_step', 'tensors'): ctypes.c_void_p, ('rnr_adam_step', 'chunks'): ctypes.c_void_p}


def _argtype(fn, d):
    if (fn, d.name) in _ARGTYPE_OVERRIDES:
        return _ARGTYPE_OVERRIDES[fn, d.name]
    if not d.pointer:
        return _value_type(d)
    if d.pointer == 1 and d.type == 'char':
        return ctypes.c_char_p
    if d.pointer == 1 and d.type in STRUCTS:
        return ctypes.POINTER(STRUCTS[d.type])
    if d.pointer > 1:               # `T* const*`: a host table of addresses, (c_void_p * n)(...)
        return ctypes.POINTER(ctypes.c_void_p)
    return ctypes.c_void_p


# name -> (restype, argtypes) of every entry point the header declares
SIGNATURES = {name: (_argtype(name, ret), [_argtype(name, p) for p in params]) for name, (ret, params) in HEADER.protos.items()}
# name -> the parameters as the header declares them (Decl: name, pointee type, pointer depth); rnr_amd.ops checks tensors by them
PARAMS = {name: tuple(params) for name, (ret, params) in HEADER.protos.items()}

_lib = None


def _build_from_source():
    """A source checkout without the built library: compile it with hipcc if the ROCm toolchain is there (still the
    HIP path — there is nothing else to fall back to).  Safe under torchrun: an exclusive file lock serialises the
    ranks (the first one builds, the others find the library once they get the lock), the Makefile links to a
    temporary name and renames it into place.  Returns the captured build log on failure, None otherwise."""
    import fcntl
    import shutil
    import subprocess
    hipcc = shutil.which('hipcc') or ('/opt/rocm/bin/hipcc' if os.path.isfile('/opt/rocm/bin/hipcc') else None)
    if hipcc is None:
        return 'hipcc not found (PATH, /opt/rocm/bin)'
    csrc = os.path.join(os.path.dirname(_HERE), 'csrc')
    try:
        lock = open(os.path.join(csrc, '.build.lock'), 'w')
    except OSError as e:
        return 'cannot create build lock in %s: %s' % (csrc, e)
    with lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            if os.path.isfile(LIB_PATH):        # another rank built it while we waited
                return None
            p = subprocess.run(['make', '-C', csrc, '-s', '-j4', 'HIPCC=' + hipcc], capture_output=True, text=True)
            if p.returncode != 0:
                return 'make exited with %d\n%s\n%s' % (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
            return None
        except OSError as e:
            return 'could not run make: %s' % e
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)


def load():
    """Load librnr_hip.so (does not need a GPU; launching kernels does)."""
    global _lib
    if _lib is not None:
        return _lib
    log = None
    if not os.path.isfile(LIB_PATH) and not os.environ.get('RNR_HIP_LIB'):
        log = _build_from_source()
    if not os.path.isfile(LIB_PATH):
        raise RnrError('librnr_hip.so not found at %s - build it first: `python -c "import __graft_entry__ as g; '
                       'g.build()"` or `make -C relightable-nr_amd/csrc`. There is no CPU fallback.%s'
                       % (LIB_PATH, ('\nautomatic build failed: ' + log) if log else ''))
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)     # AttributeError if the symbol is missing: fail loudly
        fn.restype = res
        fn.argtypes = args
    ver = lib.rnr_abi_version()
    if ver != CONSTANTS['ABI_VERSION']:
        raise RnrError('librnr_hip.so ABI version %d, python binding expects %d' % (ver, CONSTANTS['ABI_VERSION']))
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        raise RnrError(load().rnr_last_error().decode('utf-8', 'replace'))
