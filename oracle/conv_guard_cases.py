"""ORACLE (test infrastructure): the plan table of the convolution tests — ONE table for the CPU planner check
(tests/test_conv_guard_cpu.py), the guard-band sweep and NaN tracer (tests/test_gpu_conv_guard.py) and the value sweep on exact
inputs (tests/test_gpu_conv_exact_sweep.py, CPU twin tests/test_conv_exact_cpu.py).

Together the cases reach every launcher of CONV_TILES (conv.hip) for every kind it is instantiated for, the emulation rows in
both formats, and the features FEATURES lists.  The eleven families, by the lower-case names of conv.hip's ConvFamily:
  gather    conv_mfma_kernel          direct, any map                      GATHER_ROWS
  halo      conv_halo_kernel          direct, exact fp32                   HALO_ROWS
  emu       conv_halo_emu_kernel      direct, bf16x6 / f16x3 (HALO_EMU)    EMU_ROWS
  wino      conv_wino_kernel          F(2x2, 3x3)                          WINO_TILES, FAMILY: (algorithm, m)
  wino80    conv_wino80_kernel        F(2x2, 3x3), the 80-column out layer
  wino2     conv_wino2_kernel         F(2x2, 2x2), stride 2
  wino2t    conv_wino2p_kernel        F(2x2, 2x2), transposed
  wino4     conv_wino4_kernel         F(4x4, 3x3)
  wino42t   conv_wino42p_kernel       F(4x4, 2x2), transposed              (RNR_CONV_WINOGRAD42)
  wino80f4  conv_wino80f4_kernel      F(4x4, 3x3), the 80-column out layer (RNR_CONV_WINOGRAD4_OUT)
  wino42s   conv_wino42s_kernel       F(4x4, 2x2), stride 2                (RNR_CONV_WINOGRAD42S)
A family is the pair (rnr_conv_algorithm, rnr_conv_winograd_tile): the F(4x4, .) kernels share the algorithm codes 2 and 3
with the F(2x2, .) ones, and only m — the m of F(m x m, .), 0 for a direct plan — tells them apart.

The C ABI reveals the algorithm, m, the split depth (workspace bytes) and, for a maskable plan, the tile count — not the
CONV_TILES row of a plan that cannot be masked.  direct_row() below therefore restates the tile-size arithmetic of try_halo /
try_gather (default thresholds); the CPU test holds it against everything the ABI does reveal (split depth of every case — it
depends on the tile count —, tile count where maskable), and each case names the row it is there for.  Channel counts are the
smallest that still land on the row (16 - 64 inputs wherever the thresholds allow); the Winograd plans need 256 workgroups
unsplit (F(2x2, 2x2): 200) and 4 chunks per split-K slice; the three F(4x4, .) kernels behind a flag of their own have no
split-K form.

UNREACHABLE instantiations (the planner never selects them, whatever the shape; at most 3 — the CPU test holds that cap):
  halo 32 x 8 x 64, kind 1    the narrow-column branch of try_halo needs a 4x4 stride-2 call that is NOT wide_columns(), i.e.
  halo 32 x 8 x 80, kind 1    Wo % 32 == 0 and Ho % 4 != 0 — and then no tile 8 rows high fits (Ho % 8 != 0): the call goes to
  halo 32 x 4 x 64, kind 1    the gather kernel.  (32 x 4 x 64 is otherwise reached through the narrow branch, kinds 0 and 2,
                              or through RNR_CFG4_MAX, kind 0 only.)
"""
import ctypes

pad16 = lambda c: (c + 15) // 16 * 16
# RNR_CONV_* of include/rnr_hip.h (tests/test_conv_guard_cpu.py holds every CONV_* name here against rnr_amd._lib's)
CONV_F32_EMU_BF16X6, CONV_F32_EMU_F16X3, CONV_WINOGRAD, CONV_WINOGRAD4 = 2, 4, 8, 16
CONV_WINOGRAD42, CONV_WINOGRAD4_OUT, CONV_WINOGRAD42S = 32, 64, 128
EMU_FORMATS = CONV_F32_EMU_BF16X6 | CONV_F32_EMU_F16X3

# the direct rows of CONV_TILES: (pixel tile width, height, columns) -> kinds that have a launcher
HALO_ROWS = {(32, 8, 64): (0, 1, 2), (32, 8, 80): (0, 1, 2), (32, 8, 128): (0, 1, 2), (32, 4, 128): (0, 1, 2),
             (32, 4, 64): (0, 1, 2), (32, 2, 64): (0, 1, 2), (16, 8, 128): (0, 1, 2), (16, 4, 64): (0, 1, 2)}
EMU_ROWS = {(32, 8, 64): (0, 2), (32, 8, 96): (0, 2), (32, 8, 128): (0, 1, 2), (32, 4, 128): (0, 1, 2), (32, 2, 128): (1,),
            (16, 8, 128): (0, 1, 2)}
GATHER_ROWS = {(256, 1, 64): (0, 1, 2), (256, 1, 96): (0, 1, 2), (128, 1, 128): (0, 1, 2)}


def direct_row(kind, N, H, W, cins, c_out, flags=0):
    """The CONV_TILES row try_halo / try_gather of conv.hip select for a call that runs the direct kernels, restated from
    their tile-size arithmetic with the default thresholds: {'family', 'tile' (tw, th, bn), 'mtiles', 'wgs', 'splitk',
    'maskable'}."""
    emu = bool(flags & EMU_FORMATS)
    s2 = kind == 1
    c = pad16(c_out)
    Ho, Wo = (H // 2, W // 2) if s2 else (H, W)
    par = 4 if kind == 2 else 1
    chunks = sum(pad16(x) for x in cins) // 16
    taps = 9 if kind == 0 else (16 if s2 else 4)
    rows = EMU_ROWS if emu else HALO_ROWS

    def tile(tw, th, bn):
        ok = kind in rows.get((tw, th, bn), ()) and Wo % tw == 0 and Ho % th == 0 and Ho >= th
        return (tw, th, bn) if ok else None

    def count(t):
        return N * (Ho // t[1]) * (Wo // t[0]) * (-(-c // t[2])) * par

    few = lambda t: count(t) < (32 if s2 else 128)
    wide = c > 80 or (s2 and Wo % 32 == 0 and Ho % 4 == 0)
    t = None
    if Wo % 32 != 0:
        t = tile(16, 8, 128)
        if t and not emu and few(t):
            t = tile(16, 4, 64)
    elif not wide:
        t = tile(32, 8, 64 if c <= 64 else (96 if emu else 80))
        if t and not emu and c <= 64 and count(t) <= 1024:
            t = tile(32, 4, 64)
    elif emu:
        for th in (8, 4, 2):
            t = t or tile(32, th, 128)
    else:
        t = tile(32, 8, 128)
        if not t or count(t) < 512:
            t = tile(32, 4, 128)
            if t and few(t):
                t = tile(32, 2, 64)
            elif t and kind == 0 and count(t) <= 512:
                t = tile(32, 4, 64)
    if t:
        family, mtiles, wgs, units = ('emu' if emu else 'halo'), N * (Ho // t[1]) * (Wo // t[0]), count(t), chunks
    else:
        family = 'gather'
        t = (128, 1, 128) if wide else (256, 1, 64 if c <= 64 else 96)
        mtiles = -(-(N * Ho * Wo) // t[0])
        wgs, units = mtiles * (-(-c // t[2])) * par, taps * chunks // 4
    sk = 1 if wgs >= 257 else max(1, min(-(-512 // wgs), units, 64))
    return {'family': family, 'tile': t, 'mtiles': mtiles, 'wgs': wgs, 'splitk': sk,
            'maskable': kind == 0 and sk == 1 and family != 'gather' and t[0] == 32}


UNREACHABLE = [('halo', (32, 8, 64), 1), ('halo', (32, 8, 80), 1), ('halo', (32, 4, 64), 1)]

FEATURES = ('splitk_direct', 'splitk_wino', 'splitk_wino2', 'splitk_wino4', 'two_sources_unequal', 'one_tile_high',
            'tiles_straddle_views', 'pad_in_20_32', 'pad_out_78_80', 'pad_out_72_80', 'one_tile_per_view')

B, F, W, W4 = CONV_F32_EMU_BF16X6, CONV_F32_EMU_F16X3, CONV_WINOGRAD, CONV_WINOGRAD | CONV_WINOGRAD4
W42T, W42S, W4OUT = W | CONV_WINOGRAD42, W | CONV_WINOGRAD42S, W4 | CONV_WINOGRAD4_OUT
# the Winograd rows of CONV_TILES: family -> (pixel tile width, height, columns), and what the C ABI reports for the family:
# (rnr_conv_algorithm, rnr_conv_winograd_tile); WINO_KIND: the one kind a family is instantiated for where that is not 0.
WINO_TILES = {'wino80': (16, 4, 80), 'wino4': (32, 16, 64), 'wino': (16, 8, 64), 'wino2': (16, 16, 128), 'wino2t': (16, 8, 64),
              'wino42t': (32, 16, 64), 'wino42s': (32, 16, 64), 'wino80f4': (16, 16, 80)}
FAMILY = {'wino80': (3, 2), 'wino4': (4, 4), 'wino': (1, 2), 'wino2': (2, 2), 'wino2t': (2, 2),
          'wino42t': (2, 4), 'wino42s': (2, 4), 'wino80f4': (3, 4)}
WINO_KIND = {'wino2': 1, 'wino42s': 1, 'wino2t': 2, 'wino42t': 2}


def _case(kind, N, H, W_, cins, c_out, flags, family, tile, split, feats=(), tracer=False):
    algo, m = FAMILY.get(family, (0, 0))
    return dict(kind=kind, N=N, H=H, W=W_, cins=list(cins), c_out=c_out, flags=flags, family=family, tile=tile, split=split,
                algo=algo, m=m, feats=tuple(feats), tracer=tracer,
                id='k%d-%dx%dx%d-%s-%d-f%d' % (kind, N, H, W_, '+'.join(str(c) for c in cins), c_out, flags))


# kind, N, H, W, [C per source], c_out, flags, family, (tile width, height, columns), split depth, features, tracer
CASES = [
    # ---- gather (conv_mfma_kernel): maps no halo tile fits (width no multiple of 16, or a height no tile divides); the row by
    # column count: <= 64 -> 256 x 64, 65 ... 80 -> 256 x 96, wider (wide_columns) -> 128 x 128
    _case(0, 2, 24, 24, [40], 24, 0, 'gather', (256, 1, 64), 6),
    _case(0, 1, 12, 24, [16], 78, 0, 'gather', (256, 1, 96), 2, ['pad_out_78_80']),
    _case(0, 1, 12, 24, [16], 96, 0, 'gather', (128, 1, 128), 2),
    _case(1, 5, 8, 8, [16], 16, 0, 'gather', (256, 1, 64), 4, ['tiles_straddle_views'], tracer=True),     # 80 rows of five views in one tile
    _case(1, 2, 8, 8, [16], 78, 0, 'gather', (256, 1, 96), 4),
    _case(1, 2, 8, 8, [16], 96, 0, 'gather', (128, 1, 128), 4),
    _case(2, 3, 4, 4, [64], 16, 0, 'gather', (256, 1, 64), 4, ['tiles_straddle_views']),
    _case(2, 2, 4, 4, [16], 78, 0, 'gather', (256, 1, 96), 1),
    _case(2, 2, 4, 4, [16], 96, 0, 'gather', (128, 1, 128), 1),
    # ---- halo, exact fp32 (conv_halo_kernel).  32 x 8 x 64: narrow columns and MORE than RNR_CFG0_SMALL_MAX = 1024 tiles
    _case(0, 2, 264, 512, [16], 20, 0, 'halo', (32, 8, 64), 1),
    _case(2, 1, 264, 256, [16], 16, 0, 'halo', (32, 8, 64), 1),
    # 32 x 8 x 80: 65 ... 80 columns, any tile count
    _case(0, 2, 32, 64, [20], 78, 0, 'halo', (32, 8, 80), 2, ['pad_in_20_32', 'pad_out_78_80', 'splitk_direct'], tracer=True),
    _case(0, 1, 344, 192, [16], 78, 0, 'halo', (32, 8, 80), 1, ['pad_out_78_80'], tracer=True),      # 258 tiles: unsplit, maskable
    _case(2, 1, 8, 32, [32], 78, 0, 'halo', (32, 8, 80), 2, ['splitk_direct', 'one_tile_high']),
    # 32 x 8 x 128: wide columns and >= RNR_NATIVE_BIG_MIN = 512 tiles (the stride-2 convolution is wide whatever its columns)
    _case(0, 1, 256, 512, [16], 96, 0, 'halo', (32, 8, 128), 1),
    _case(1, 2, 512, 512, [16], 16, 0, 'halo', (32, 8, 128), 1),
    _case(2, 1, 64, 512, [16], 96, 0, 'halo', (32, 8, 128), 1),
    # 32 x 4 x 128: wide columns, fewer than 512 tiles 8 rows high (or a height 8 does not divide), not `few`, and for the 3x3
    # convolution more than RNR_CFG4_MAX = 512 tiles 4 rows high
    _case(0, 1, 1028, 64, [16], 96, 0, 'halo', (32, 4, 128), 1),
    _case(1, 2, 64, 128, [32], 16, 0, 'halo', (32, 4, 128), 2, ['splitk_direct']),
    _case(2, 2, 32, 64, [32], 128, 0, 'halo', (32, 4, 128), 2, ['splitk_direct']),
    # 32 x 4 x 64: narrow columns and at most 1024 tiles 8 rows high (kinds 0, 2), or the 3x3 convolution at <= 512 wide tiles
    _case(0, 1, 64, 64, [112], 64, 0, 'halo', (32, 4, 64), 7, ['splitk_direct']),
    _case(0, 1, 1032, 32, [16], 32, 0, 'halo', (32, 4, 64), 1),                     # 258 tiles: unsplit, maskable
    _case(0, 2, 8, 32, [32], 32, 0, 'halo', (32, 4, 64), 2, ['splitk_direct']),
    _case(0, 2, 64, 128, [32], 128, 0, 'halo', (32, 4, 64), 2, ['splitk_direct']),  # through RNR_CFG4_MAX: 128 tiles of 32 x 4 x 128
    _case(2, 1, 8, 32, [32], 32, 0, 'halo', (32, 4, 64), 2, ['splitk_direct']),
    # 32 x 2 x 64: wide columns and `few` tiles 4 rows high (< 128; stride 2: < 32)
    _case(0, 2, 4, 32, [32], 96, 0, 'halo', (32, 2, 64), 2, ['splitk_direct']),
    _case(1, 1, 8, 64, [16], 16, 0, 'halo', (32, 2, 64), 1),
    _case(2, 1, 4, 32, [16], 96, 0, 'halo', (32, 2, 64), 1),
    # 16 x 8 x 128: maps 16 (48, ...) pixels wide with at least 128 (stride 2: 32) tiles
    _case(0, 2, 512, 16, [16], 16, 0, 'halo', (16, 8, 128), 1),
    _case(1, 1, 512, 32, [16], 16, 0, 'halo', (16, 8, 128), 1),
    _case(2, 1, 256, 16, [16], 16, 0, 'halo', (16, 8, 128), 1),
    # 16 x 4 x 64: the same maps with fewer tiles
    _case(0, 1, 8, 16, [32], 32, 0, 'halo', (16, 4, 64), 2, ['splitk_direct']),
    _case(0, 1, 16, 16, [16, 32], 128, 0, 'halo', (16, 4, 64), 3, ['two_sources_unequal', 'splitk_direct'], tracer=True),
    _case(1, 1, 16, 32, [16], 16, 0, 'halo', (16, 4, 64), 1),
    _case(2, 1, 8, 16, [16], 16, 0, 'halo', (16, 4, 64), 1),
]
# ---- halo, emulated fp32 (conv_halo_emu_kernel), every row in both formats: narrow columns -> 32 x 8 x 64 / x 96 (kinds 0, 2);
# wide columns -> the tallest of 32 x 8 / 4 / 2 x 128 that divides the height (2: stride 2 only, Ho % 4 != 0 with > 80
# columns); maps 16 pixels wide -> 16 x 8 x 128
for _f in (B, F):
    CASES += [
        _case(0, 2, 8, 32, [32], 32, _f, 'emu', (32, 8, 64), 2, ['one_tile_high', 'splitk_direct'], tracer=True),
        _case(2, 1, 8, 32, [16], 16, _f, 'emu', (32, 8, 64), 1),
        _case(0, 1, 16, 32, [20], 78, _f, 'emu', (32, 8, 96), 2, ['pad_in_20_32', 'pad_out_78_80', 'splitk_direct']),
        _case(2, 1, 8, 32, [16], 78, _f, 'emu', (32, 8, 96), 1),
        _case(0, 1, 8, 64, [16], 96, _f, 'emu', (32, 8, 128), 1),
        _case(1, 2, 16, 64, [16, 32], 16, _f, 'emu', (32, 8, 128), 3, ['two_sources_unequal', 'splitk_direct']),
        _case(2, 1, 8, 32, [16], 96, _f, 'emu', (32, 8, 128), 1),
        _case(0, 1, 4, 32, [16], 96, _f, 'emu', (32, 4, 128), 1),
        _case(1, 1, 8, 64, [16], 16, _f, 'emu', (32, 4, 128), 1),
        _case(2, 1, 4, 32, [16], 96, _f, 'emu', (32, 4, 128), 1),
        _case(1, 1, 4, 64, [16], 96, _f, 'emu', (32, 2, 128), 1),
        _case(0, 1, 8, 16, [16], 16, _f, 'emu', (16, 8, 128), 1, ['one_tile_high']),
        _case(1, 1, 16, 32, [16], 16, _f, 'emu', (16, 8, 128), 1),
        _case(2, 1, 8, 16, [16], 16, _f, 'emu', (16, 8, 128), 1),
    ]
# ---- the Winograd kernels: 256 workgroups unsplit (F(2x2, 2x2): 200), split-K slices of at least 4 chunks
CASES += [
    _case(0, 4, 64, 64, [16], 72, W, 'wino80', (16, 4, 80), 1, ['pad_out_72_80'], tracer=True),          # 4 x 16 x 4 = 256 tiles
    _case(0, 16, 64, 64, [16], 128, W4, 'wino4', (32, 16, 64), 1, tracer=True),                          # 16 x 8 x 2 column tiles = 256
    _case(0, 64, 16, 32, [16], 256, W4, 'wino4', (32, 16, 64), 1, ['one_tile_per_view', 'one_tile_high']),
    _case(0, 2, 64, 64, [128], 512, W4, 'wino4', (32, 16, 64), 2, ['splitk_wino4'], tracer=True),        # 128 workgroups, 8 chunks
    _case(0, 2, 64, 128, [20], 128, W, 'wino', (16, 8, 64), 1, ['pad_in_20_32'], tracer=True),           # 2 x 64 x 2 = 256
    _case(0, 64, 8, 16, [16], 256, W, 'wino', (16, 8, 64), 1, ['one_tile_per_view', 'one_tile_high']),
    _case(0, 2, 32, 32, [128], 512, W, 'wino', (16, 8, 64), 2, ['splitk_wino'], tracer=True),            # 128 workgroups, 8 chunks
    _case(1, 4, 256, 256, [16], 128, W, 'wino2', (16, 16, 128), 1),                                      # 4 x 64 = 256
    _case(1, 50, 32, 32, [16], 512, W, 'wino2', (16, 16, 128), 1, ['one_tile_per_view', 'one_tile_high'], tracer=True),  # 50 x 4 = 200
    _case(1, 2, 128, 128, [128], 512, W, 'wino2', (16, 16, 128), 2, ['splitk_wino2'], tracer=True),      # 128 workgroups, 8 chunks
    _case(2, 13, 32, 64, [16, 32], 64, W, 'wino2t', (16, 8, 64), 1, ['two_sources_unequal'], tracer=True),       # 13 x 16 = 208
    _case(2, 1, 64, 64, [80, 48], 256, W, 'wino2t', (16, 8, 64), 2, ['two_sources_unequal', 'splitk_wino2'], tracer=True),   # 128 workgroups; slice 1 straddles the concat
    # F(4x4, 2x2) transposed: one parity class of 32 x 16 input pixels, 256 workgroups (tiles x column tiles x 4 classes)
    _case(2, 16, 32, 64, [16, 32], 64, W42T, 'wino42t', (32, 16, 64), 1, ['two_sources_unequal'], tracer=True),      # 16 x 4 tiles x 4 classes = 256
    _case(2, 64, 16, 32, [16], 64, W42T, 'wino42t', (32, 16, 64), 1, ['one_tile_per_view', 'one_tile_high'], tracer=True),
    _case(2, 64, 16, 32, [16, 16], 64, W42T, 'wino42t', (32, 16, 64), 1),                    # the value sweep's case (C)
    # F(4x4, 2x2) stride 2: 32 x 16 output pixels
    _case(1, 64, 32, 64, [16], 256, W42S, 'wino42s', (32, 16, 64), 1, ['one_tile_per_view', 'one_tile_high'], tracer=True),   # 64 x 4 column tiles = 256; value sweep (C)
    _case(1, 32, 64, 128, [16, 32], 128, W42S, 'wino42s', (32, 16, 64), 1, ['two_sources_unequal'], tracer=True),            # 32 x 4 tiles x 2 = 256
    # F(4x4, 3x3) of the out layer: 256 tiles of 16 x 16 output pixels, maskable
    _case(0, 256, 16, 16, [16, 32], 78, W4OUT, 'wino80f4', (16, 16, 80), 1, ['one_tile_per_view', 'two_sources_unequal', 'pad_out_78_80'], tracer=True),
    _case(0, 4, 128, 128, [20], 78, W4OUT, 'wino80f4', (16, 16, 80), 1, ['pad_in_20_32', 'pad_out_78_80'], tracer=True),
    _case(0, 256, 16, 16, [16, 16], 78, W4OUT, 'wino80f4', (16, 16, 80), 1),                 # the value sweep's case (B)
]

# (c) ReLU and NaN: one 3x3 shape every family runs — direct, F(2x2, 3x3), F(4x4, 3x3), both emulation formats
RELU_NAN_SHAPE = (0, 16, 64, 64, [16], 128)
RELU_NAN_FLAGS = ((0, 0, 0), (W, 1, 2), (W4, 4, 4), (B, 0, 0), (F, 0, 0))   # (flags, algorithm and m the planner must report)


def desc(c):
    """rnr_conv_desc of a case."""
    from rnr_amd.testing import conv_desc
    return conv_desc(c['kind'], c['cins'], c['c_out'], c['flags'])


def split_depth(L, c):
    """The split-K depth of a case's plan, from the workspace the host planner of library handle `L` asks for: 256 bytes
    unsplit, otherwise one float32 slab of the padded output per slice."""
    d = desc(c)
    ws = L.rnr_conv_workspace_bytes(ctypes.byref(d), c['N'], c['H'], c['W'])
    oh, ow = out_hw(c['kind'], c['H'], c['W'])
    return 1 if ws == 256 else ws // (c['N'] * oh * ow * d.c_out_pad * 4)


def out_hw(kind, H, W_):
    return (H, W_) if kind == 0 else ((H // 2, W_ // 2) if kind == 1 else (2 * H, 2 * W_))


def mask_tile(c):
    """(tile width, height) of the MASKED launch of a case (rnr_conv_tile_count describes that launch): the out layer's
    Winograd kernels take the mask on their own 16 x 4 resp. 16 x 16 tiles, every other Winograd plan runs the direct kernels
    when masked."""
    if c['family'] in ('halo', 'emu', 'wino80', 'wino80f4'):
        return c['tile'][:2]
    return direct_row(c['kind'], c['N'], c['H'], c['W'], c['cins'], c['c_out'], 0)['tile'][:2]
