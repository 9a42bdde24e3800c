"""CPU: the C-ABI library loads and exports every symbol include/rnr_hip.h declares, and the Python binding, which rnr_amd._lib
derives from that header, says what the header says: completeness, layouts and constants against a C compiler, hand-pinned
signatures, the parser's strictness, and the argument checks of rnr_amd.ops._call (no kernel launches)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'rnr_hip.h')


def _code():
    return re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)


def test_header_symbols_exported():
    from rnr_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, 'include', 'rnr_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    declared = set(re.findall(r'\b(rnr_[a-z0-9_]+)\s*\(', hdr))
    assert declared, 'no declarations parsed'
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    lib = _lib.load()
    for name in sorted(declared):
        assert hasattr(lib, name), 'librnr_hip.so does not export %s' % name
        assert name in _lib.SIGNATURES, 'python binding lacks a signature for %s' % name
    assert set(_lib.SIGNATURES) <= declared, set(_lib.SIGNATURES) - declared
    assert lib.rnr_abi_version() == 1


def test_product_does_not_import_oracle():
    """The product package must never route through the oracle (or any CPU fallback)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, 'relightable-nr_amd')
    for dp, _, fns in os.walk(pkg):
        for fn in fns:
            if fn.endswith('.py'):
                src = open(os.path.join(dp, fn)).read()
                assert not re.search(r'^\s*(from|import)\s+oracle\b', src, flags=re.M), os.path.join(dp, fn)


def test_missing_gpu_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    from rnr_amd import ops
    with pytest.raises(RuntimeError):
        ops.sh_basis(torch.zeros(4, 3), 2)          # CPU tensor -> loud error, not a CPU fallback


# ------------------------------------------------------------------------------------------------
# the binding is derived from the header
# ------------------------------------------------------------------------------------------------
def test_binding_covers_the_whole_header():
    from rnr_amd import _lib
    code = _code()
    declared = set(re.findall(r'\b(rnr_[a-z0-9_]+)\s*\(', code))
    assert len(declared) >= 80 and declared == set(_lib.SIGNATURES) == set(_lib.PARAMS)
    for name, (restype, argtypes) in _lib.SIGNATURES.items():
        assert len(argtypes) == len(_lib.PARAMS[name]), name
    assert len(re.findall(r'\btypedef\s+struct\b', code)) == len(_lib.STRUCTS) >= 11
    for cls in _lib.STRUCTS.values():
        assert issubclass(cls, ctypes.Structure) and getattr(_lib, cls.__name__) is cls
    names = re.findall(r'^[ \t]*#[ \t]*define[ \t]+(RNR_\w+)[ \t]+\S', code, flags=re.M)
    for body in re.findall(r'\benum\s*\{(.*?)\}', code, flags=re.S):
        names += [part.split('=')[0].strip() for part in body.split(',') if part.strip()]
    assert len(names) >= 40 and len(set(names)) == len(names)
    for n in names:
        assert n.startswith('RNR_') and n[4:] in _lib.CONSTANTS and getattr(_lib, n[4:]) == _lib.CONSTANTS[n[4:]], n
    assert len(_lib.CONSTANTS) == len(names)
    # the dictionaries built from them
    assert _lib.EMU_FLAGS == {'f32': 0, 'bf16x6': 2, 'f16x3': 4}
    assert _lib.BN_BWD_MODES == {'batch': 0, 'batch_all': 1, 'running': 2}
    assert _lib.PRESENT_MODES == {'frame': 0, 'composite': 1, 'background': 2} and _lib.PRESENT_RGB == 8
    assert _lib.METRIC_KEYS == ('mae', 'mae_bb', 'mae_valid', 'mse', 'mse_bb', 'mse_valid', 'psnr', 'psnr_bb', 'psnr_valid', 'ssim',
                                'ssim_bb', 'ssim_valid')
    assert _lib.ADAM_MAX_MIRRORS == 3 and _lib.RnrAdamTensor.mirror.size == 3 * ctypes.sizeof(_lib.RnrAdamMirror)


def test_layouts_and_constants_against_the_c_compiler(tmp_path):
    """sizeof / offsetof of every struct and field and the value of every constant, as a C compiler sees the header, equal
    what ctypes lays out and what the parser evaluated."""
    from rnr_amd import _lib
    cc = shutil.which('cc') or shutil.which('gcc')
    if cc is None:
        pytest.skip('no C compiler on this machine')
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rnr_hip.h"', 'int main(void) {']
    expected = []
    for name, cls in _lib.STRUCTS.items():
        lines.append('    printf("sizeof %s %%zu\\n", sizeof(%s));' % (name, name))
        expected.append('sizeof %s %d' % (name, ctypes.sizeof(cls)))
        for field, _ in cls._fields_:
            lines.append('    printf("field %s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));'
                         % (name, field, name, field, name, field))
            expected.append('field %s.%s %d %d' % (name, field, getattr(cls, field).offset, getattr(cls, field).size))
    for name, value in _lib.CONSTANTS.items():
        lines.append('    printf("constant %s %%lld\\n", (long long)(RNR_%s));' % (name, name))
        expected.append('constant %s %d' % (name, value))
    lines += ['    return 0;', '}']
    assert len(expected) > 11 + 60 + 40
    src, exe = tmp_path / 'abi_probe.c', tmp_path / 'abi_probe'
    src.write_text('\n'.join(lines) + '\n')
    subprocess.run([cc, '-std=c99', '-Wall', '-Werror', '-I', os.path.dirname(HEADER), str(src), '-o', str(exe)], check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split('\n')
    assert got[:-1] == expected


def test_pinned_signatures():
    """Argtypes written out by hand for entry points that between them cover every scalar kind and pointer flavour."""
    from rnr_amd import _lib
    from ctypes import POINTER as P, c_char_p, c_double, c_float, c_int, c_long, c_size_t, c_void_p
    desc, src = P(_lib.RnrConvDesc), P(_lib.RnrConvSrc)
    pinned = {
        'rnr_last_error': (c_char_p, []),
        'rnr_raster_workspace_bytes': (c_size_t, [c_int, c_int, c_int]),
        'rnr_forward_face_index_map': (c_int, [c_void_p] * 6 + [c_int, c_int, c_int, c_float, c_float, c_int, c_int, c_int, c_void_p,
                                                                c_void_p]),
        'rnr_rasterize_gbuffer': (c_int, [P(_lib.RnrMesh), c_void_p, c_void_p, c_int, c_int, c_float, c_float, P(_lib.RnrGbuffer),
                                          c_void_p, c_void_p]),
        # textures_host is a host table of addresses, tex_sizes_host a host array of int: a plain address
        'rnr_shade_inputs': (c_int, [c_void_p] * 5 + [c_int, c_void_p, c_void_p, P(c_void_p), c_void_p, c_int, c_int, c_int,
                                                      P(_lib.RnrRays), c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                                      c_int, c_void_p]),
        'rnr_conv2d_fused': (c_int, [desc, src, src, c_void_p, c_void_p, P(_lib.RnrConvBn), c_int, c_int, c_int, c_void_p, c_size_t,
                                     c_void_p, c_size_t, c_void_p, c_void_p]),
        'rnr_bn_finalize_saved': (c_int, [c_void_p] * 7 + [c_float, c_void_p, c_int, c_int, c_int, c_int, c_double, c_float, c_void_p]),
        'rnr_tbn_matvec': (c_int, [c_void_p, c_void_p, c_void_p, c_long, c_int, c_void_p]),
        'rnr_probe_prepare': (c_int, [c_void_p, c_void_p, c_double, c_void_p, c_void_p, c_int, c_int, c_void_p]),
        'rnr_stitch_accumulate': (c_int, [c_void_p, c_int] + [c_void_p] * 6 + [c_size_t, c_int, c_int, c_int, c_int, c_int, c_void_p]),
        # tensors and chunks are DEVICE tables passed as integer addresses: the binding's one override of the header
        'rnr_adam_step': (c_int, [c_void_p, c_int, c_void_p, c_int, P(_lib.RnrAdamScalars), c_int, c_void_p]),
        'rnr_pack_conv_weights': (c_int, [desc, P(c_void_p), P(c_void_p), c_int, c_void_p]),
        'rnr_obj_parse': (c_int, [c_char_p, c_size_t, P(_lib.RnrObjCounts)] + [c_void_p] * 6),
        'rnr_calibrate_mfma_f32': (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    }
    for name, (restype, argtypes) in pinned.items():
        got = _lib.SIGNATURES[name]
        assert got[0] is restype, name
        assert len(got[1]) == len(argtypes) and all(a is b for a, b in zip(got[1], argtypes)), \
            (name, [i for i, (a, b) in enumerate(zip(got[1], argtypes)) if a is not b])
    assert [(p.name, p.type, p.pointer) for p in _lib.PARAMS['rnr_adam_step'][:3]] == \
        [('tensors', 'rnr_adam_tensor', 1), ('num_tensors', 'int', 0), ('chunks', 'rnr_adam_chunk', 1)]
    assert [(p.name, p.type, p.pointer) for p in _lib.PARAMS['rnr_pack_conv_weights'][1:3]] == \
        [('weights', 'float', 2), ('packed', 'float', 2)]


SMALL_HEADER = '''/* a comment
over two lines */
#ifndef X_H
#define X_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define RNR_N 3
#define RNR_BOTH (RNR_N | 4)      /* trailing comment */
enum { RNR_A = 5, RNR_B, RNR_C = RNR_N };
typedef struct rnr_in { float* p; int64_t stride[4]; int a, b; } rnr_in;
typedef struct rnr_out {
    const float* g;     /* [n] */
    rnr_in inner[RNR_N];
} rnr_out;
const char* rnr_name(void);
size_t rnr_bytes(const rnr_out* o, long n);
int rnr_run(const float* const* tables_host, const uint8_t* mask, double gamma,
            void* stream);
#ifdef __cplusplus
}
#endif
#endif
'''


def test_parser_reads_the_c_subset_of_the_header():
    from rnr_amd._lib import Decl, parse_header
    h = parse_header(SMALL_HEADER)
    assert h.constants == {'RNR_N': 3, 'RNR_BOTH': 7, 'RNR_A': 5, 'RNR_B': 6, 'RNR_C': 3} and h.enums == [('RNR_A', 'RNR_B', 'RNR_C')]
    assert h.structs == {'rnr_in': [Decl('p', 'float', 1, None), Decl('stride', 'int64_t', 0, 4), Decl('a', 'int', 0, None),
                                    Decl('b', 'int', 0, None)],
                         'rnr_out': [Decl('g', 'float', 1, None), Decl('inner', 'rnr_in', 0, 3)]}
    assert h.protos == {'rnr_name': (Decl('rnr_name', 'char', 1, None), []),
                        'rnr_bytes': (Decl('rnr_bytes', 'size_t', 0, None), [Decl('o', 'rnr_out', 1, None), Decl('n', 'long', 0, None)]),
                        'rnr_run': (Decl('rnr_run', 'int', 0, None),
                                    [Decl('tables_host', 'float', 2, None), Decl('mask', 'uint8_t', 1, None),
                                     Decl('gamma', 'double', 0, None), Decl('stream', 'void', 1, None)])}


@pytest.mark.parametrize('text, line', [
    ('int rnr_a(int x);\nint rnr_b(short x);\n', 2),                                            # an unknown type
    ('int rnr_a(int x);\n\nunsigned int rnr_b(int x);\n', 3),                                   # ... as a return type
    ('int rnr_a(int x,\n#if RNR_WIDE\n          int y,\n#endif\n          void* stream);\n', 2),    # a prototype split by a conditional
    ('int rnr_a(int x);\nint rnr_b(int y)\nint rnr_c(int z);\n', 2),                            # ... run into the next one
    ('int rnr_a(int x);\nint rnr_b(void (*done)(int), void* stream);\n', 2),                    # ... by a function-pointer parameter
    ('int rnr_a(int x);\nint rnr_b(int x', 2),                                                  # ... never closed
    ('typedef struct rnr_s {\n    int a;\n    unsigned flags;\n} rnr_s;\n', 3),                 # a struct field it cannot type
    ('typedef struct rnr_s {\n    int a;\n    int b : 3;\n} rnr_s;\n', 3),                      # ... a bit field
    ('typedef struct rnr_s {\n    int a[RNR_UNKNOWN];\n} rnr_s;\n', 2),                         # ... an array of unknown length
    ('#define RNR_X 1u\n', 1),                                                                  # a constant that is not a plain integer
    ('int rnr_a(int x);\nstatic inline int helper(int x) { return x; }\n', 2),                  # anything else
])
def test_parser_is_strict(text, line):
    from rnr_amd._lib import RnrError, parse_header
    with pytest.raises(RnrError, match=r'line %d\b' % line):
        parse_header(text)


def test_missing_header_is_an_error_naming_the_path(tmp_path):
    """A copy of the binding with no include/ directory two levels up: importing it raises, it does not come up empty."""
    import importlib.util
    from rnr_amd import _lib
    pkg = tmp_path / 'pkg' / 'rnr_amd'
    pkg.mkdir(parents=True)
    shutil.copy(_lib.__file__, str(pkg / '_lib.py'))
    spec = importlib.util.spec_from_file_location('rnr_lib_without_header', str(pkg / '_lib.py'))
    with pytest.raises(RuntimeError, match=re.escape(str(tmp_path / 'include' / 'rnr_hip.h'))) as e:
        spec.loader.exec_module(importlib.util.module_from_spec(spec))
    assert type(e.value).__name__ == 'RnrError'


def test_cpu_tensor_is_refused_by_name_before_the_library_is_loaded(monkeypatch):
    """One wrapper of each family: the RuntimeError names the parameter as the header spells it, and nothing has asked for the
    library by then (so the refusal is as loud on a machine where nothing is built)."""
    import torch
    from rnr_amd import _lib, ops

    def no_load():
        raise AssertionError('the library was loaded before the arguments were checked')
    monkeypatch.setattr(_lib, 'load', no_load)
    f32, i32 = torch.zeros(2, 4, 4), torch.zeros(2, 4, 4, dtype=torch.int32)
    img = torch.zeros(1, 3, 12, 12)
    cases = {
        'faces': lambda: ops.forward_face_index_map(torch.zeros(1, 2, 3, 3), i32[:1], f32, f32, None, f32, 4, 0.1, 100.0, 0, 1, 0),
        'proj_inv': lambda: ops.view_dir_map((4, 4), torch.eye(3)[None], torch.eye(3)[None]),
        'est': lambda: ops.masked_l1_loss(img, img, torch.ones(1, 1, 12, 12), 5),
        'rays_lt': lambda: ops.rays_chrom_loss(torch.ones(1, 2, 3, 4, 4), torch.ones(1, 1, 4, 4)),
        r'\best\b': lambda: ops.image_metrics(img, img),
        'sum': lambda: ops.stitch_finalize(torch.zeros(4, 8, 3, dtype=torch.float64), torch.zeros(4, 8, dtype=torch.int32)),
        'lp': lambda: ops.probe_prepare(torch.zeros(4, 8, 3), torch.ones(4, 8, dtype=torch.uint8)),
        'dirs': lambda: ops.sh_basis(torch.zeros(4, 3), 2),
    }
    for param, call in cases.items():
        with pytest.raises(RuntimeError, match=r'^%s must be a CUDA \(HIP\) tensor$' % param):
            call()
