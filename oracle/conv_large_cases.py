"""ORACLE (test infrastructure): the convolutions at buffer sizes beyond 2 GiB and 4 GiB — the case table, the periodic exact
inputs and the expectation of a whole launch from one small float64 convolution.  tests/test_gpu_conv_large.py runs the table
on the GPU, tests/test_conv_large_cpu.py proves on the CPU what that module rests on.

WHY.  Every kernel but the gather kernel reads a source view through a buffer resource of 0x7fffffff bytes with a 32-bit BYTE
offset (conv_stage.inc: buffer_rsrc, halo_load); an access outside the range is dropped, not faulted — a silent zero.  Outputs
go through a 64-bit tile base.  The case table of oracle/conv_guard_cases.py is built from the smallest shapes; this one puts
the same launchers where the offsets are large.

THE TABLE, in the id style of conv_guard_cases.CASES (`bytes`: device memory the test holds at once, see case_bytes).

  View-count cases (VIEW_CASES), one per launcher family — gather, halo, the three 16-bit formats of conv_halo_emu_kernel
  (bf16x6, f16x3, f16), wino, wino80, wino2, wino2t, wino4, wino42t, wino42s, wino80f4.  The larger of the input and output
  buffers holds at least one whole view beyond byte 2^32 (and so the 2^31 boundary too): N = ceil(2^32 / view bytes) + 1.  The
  channel counts are the smallest the family takes (16 inputs; 16 / 64 / 80 / 128 columns) and the larger buffer's views are
  512^2 or 1024^2, whichever needs fewer bytes (view_count_shape; the CPU twin recomputes every row).  The gather row is the
  exception in shape: the gather kernel gets the maps no halo tile fits, so its views are 1020^2 (1020 = 17 * 60: no multiple
  of 16) on R = 60.
    two sources     the F(4x4, 3x3) row reads a skip concat of 16 + 16 channels
    fused           the halo row also runs rnr_conv2d_fused with BatchNorm: scale / shift, and through rnr_conv2d the sums
    masked          the out-layer row wino80 also runs rnr_conv2d_masked on a checkerboard of its 16 x 4 tiles
    split-K         NOT REACHABLE at this size, so there is no such row: direct_choice and wino_splitk split only grids below
                    257 resp. 256 workgroups of one K slice.  256 workgroups cover at most 256 * 512 GEMM rows (the largest
                    tile is 32 x 16 pixels), i.e. at most 4 * 131072 input pixels (stride 2) — a 2^32-byte buffer over them
                    needs 2048 channels in one source, and a source view past 2^31 bytes 4096 (4 x and 8 x what
                    exact_conv_case can keep exact, c_in <= 512; the CPU twin holds the arithmetic).  This holds for the
                    DEFAULT tuning only: the thresholds are read from the environment (RNR_SPLITK_BELOW, RNR_WINO_MIN_WGS,
                    ...) once per process, and the 512 channels are the limit of the test's generator, not of the library
                    — a caller with thousands of channels, or with the thresholds raised, reaches split-K slabs beyond
                    4 GiB, which no test here runs.  The split-K rows of
                    conv_guard_cases stay the test of the slab arithmetic, which is size_t throughout (splitk_reduce_kernel).

  Single-view cases (SINGLE_CASES): N = 1, 3x3, c_out = 16 — the offsets INSIDE one source view.
    (a) 2048 x 2048 x 128   exactly 2^29 floats = 2^31 bytes: the last dword of the view ends at byte 2^31
    (b) 2048 x 2560 x 128   2.5 GiB: the rows from 1638 on lie beyond 2 GiB
    (c) 2048 x 2016 x 256   just under 2^30 floats (R = 32: 2016 = 63 * 32)
    (d) 2048 x 2048 x 256   exactly 2^30 floats
    (e) 2048 x 2560 x 16 + 128   two sources, only source 1 crosses 2 GiB
    (f) (b) with RNR_CONV_F32_EMU_BF16X6 and with RNR_CONV_F16
  A source view of 2^31 bytes or more is a "big view" (plan_conv): the gather kernel, which addresses with size_t, runs it —
  `family` names that — and a 16-bit-format call has no kernel there: family 'refused', the call must fail before any launch
  with a message that names the view's bytes.  big_view() restates the rule.  halo_crossing() is the boundary arithmetic of
  the halo kernels on such a view: which pixels' dwords reach the end of the resource's range, which output rows read them.
  The bound is the one the hardware decided (profiles/conv_large.txt): with the planner's earlier bound of 2^30 ELEMENTS the
  halo kernel ran (a), (b), (c) and (e); all four were wrong from exactly the row — in (b) from the very pixel — that the
  'inclusive' reading of halo_crossing names: the range check is per dword and on the dword's END, so of a view of exactly
  2^31 bytes the last dword alone is lost.  (a)'s base block is drawn with SALT so that this one dword shows: the CPU twin
  holds that zeroing it changes outputs.

PERIODIC EXACT INPUTS.  A case's data is a base block from oracle.conv64.exact_conv_case: P = 2 views of R x R pixels, R a
multiple of every pixel-tile and Winograd-patch dimension of the row and even (R = 64: every tile is at most 32 x 16 pixels,
output pixels for the stride-2 kind, input pixels of a parity class for the transposed one).  The device input is the block
repeated over rows, columns and views (view n = block n mod P; the per-view scale and shift rows repeat with it).  The
convolution of such a map is known from the float64 convolution of the 3R x 3R map tile(base, 3, 3) alone: in output
coordinates, with output period p = R (3x3), R / 2 (stride 2), 2R (transposed), the first block of the large map is the
first block of the small one, the last block the last, and every block in between the middle block — per axis, since the
windows reach one input pixel (3x3, transposed) or two (stride 2: 2 o - 1 .. 2 o + 2) beyond the block, well inside the
neighbouring block, and the border rule (ReflectionPad2d(1), zero border) sees the same pixels at both sizes.
expect_index(kind, size, R) is that gather index.
"""
import zlib

import numpy as np
import torch

from oracle import conv64 as o64
from oracle import conv_guard_cases as cg
from oracle.conv_guard_cases import pad16

P_VIEWS = 2
CONV_F16 = 256                          # RNR_CONV_F16 of include/rnr_hip.h (tests/test_conv_large_cpu.py holds it against rnr_amd._lib's)
B, F, W, W4, W42T, W42S, W4OUT = cg.B, cg.F, cg.W, cg.W4, cg.W42T, cg.W42S, cg.W4OUT
FORMATS_16BIT = cg.EMU_FORMATS | CONV_F16
VIEW_BYTES_MAX = 1 << 31                # plan_conv: a source view of this many bytes or more is a big view
RSRC_BYTES = 0x7fffffff                 # buffer_rsrc of conv_stage.inc


def big_view(c):
    """plan_conv's rule: the larger source view of the case, H * W * c_in_pad * 4 bytes, reaches VIEW_BYTES_MAX."""
    return c['H'] * c['W'] * max(pad16(x) for x in c['cins']) * 4 >= VIEW_BYTES_MAX


def case_bytes(kind, N, H, W_, cins, c_out, outputs=1):
    """Device bytes a test of the case holds at once: the sources, `outputs` out_raw buffers (2 for the masked row) and three
    output views of working memory for the comparison (expectation, difference, float64 of a view at the bounded families)."""
    oh, ow = cg.out_hw(kind, H, W_)
    out_view = oh * ow * pad16(c_out) * 4
    return N * H * W_ * sum(pad16(x) for x in cins) * 4 + outputs * N * out_view + 3 * max(out_view, 1 << 28)


def _case(kind, N, H, W_, cins, c_out, flags, family, tile, R=64, also=(), group='views'):
    c = cg._case(kind, N, H, W_, cins, c_out, flags, family, tile, 1)
    if family == 'refused':
        c['algo'], c['m'] = -1, -1
    c.update(R=R, also=tuple(also), group=group, id=('L-' if group == 'views' else 'S-') + c['id'],
             bytes=case_bytes(kind, N, H, W_, cins, c_out, 2 if 'masked' in also else 1))
    return c


def view_count_shape(kind, cins, c_out):
    """(N, H) of a view-count row: square input maps of H pixels such that the LARGER of the input and output views is 512^2 or
    1024^2 pixels, N = ceil(2^32 / bytes of that view) + 1 views, and of the candidates the one whose buffers hold the fewest
    bytes (ties: fewer views)."""
    best = None
    for H in (256, 512, 1024, 2048):
        oh = cg.out_hw(kind, H, H)[0]
        in_view, out_view = H * H * max(pad16(x) for x in cins) * 4, oh * oh * pad16(c_out) * 4
        if (H if in_view >= out_view else oh) not in (512, 1024):
            continue
        N = -(-2 ** 32 // max(in_view, out_view)) + 1
        total = N * (H * H * sum(pad16(x) for x in cins) * 4 + out_view)
        if best is None or (total, N) < best[:2]:
            best = (total, N, H)
    return best[1], best[2]


def _vcase(kind, cins, c_out, flags, family, tile, also=()):
    N, H = view_count_shape(kind, cins, c_out)
    return _case(kind, N, H, H, cins, c_out, flags, family, tile, also=also)


# kind, [C per source], c_out, flags, family, (tile width, height, columns); N and the map size follow from view_count_shape
VIEW_CASES = [
    _case(0, 66, 1020, 1020, [16], 16, 0, 'gather', (256, 1, 64), R=60),       # 66 views of 63.5 MiB, in and out
    _vcase(0, [16], 16, 0, 'halo', (32, 8, 64), also=('fused',)),              # 257 views of 512^2 x 16: 16 MiB, in and out
    _vcase(0, [16], 16, B, 'emu', (32, 8, 64)),
    _vcase(0, [16], 16, F, 'emu', (32, 8, 64)),
    _vcase(0, [16], 16, CONV_F16, 'emu', (32, 8, 64)),
    _vcase(0, [16], 64, W, 'wino', (16, 8, 64)),                               # 65 output views of 512^2 x 64: 64 MiB
    _vcase(0, [16], 80, W, 'wino80', (16, 4, 80), also=('masked',)),           # 53 output views of 512^2 x 80: 80 MiB
    _vcase(1, [16], 128, W, 'wino2', (16, 16, 128)),                           # 33 output views of 512^2 x 128 (input 1024^2)
    _vcase(2, [16], 64, W, 'wino2t', (16, 8, 64)),                             # 65 output views of 512^2 x 64 (input 256^2)
    _vcase(0, [16, 16], 64, W4, 'wino4', (32, 16, 64)),                        # the skip concat
    _vcase(2, [16], 64, W42T, 'wino42t', (32, 16, 64)),
    _vcase(1, [16], 64, W42S, 'wino42s', (32, 16, 64)),                        # 257 views: 512^2 x 16 in, 256^2 x 64 out, 16 MiB each
    _vcase(0, [16], 80, W4OUT, 'wino80f4', (16, 16, 80)),
]
_S = dict(group='single')
SINGLE_CASES = [
    _case(0, 1, 2048, 2048, [128], 16, 0, 'gather', (256, 1, 64), **_S),                    # (a)
    _case(0, 1, 2048, 2560, [128], 16, 0, 'gather', (256, 1, 64), **_S),                    # (b)
    _case(0, 1, 2048, 2016, [256], 16, 0, 'gather', (256, 1, 64), R=32, **_S),              # (c)
    _case(0, 1, 2048, 2048, [256], 16, 0, 'gather', (256, 1, 64), **_S),                    # (d)
    _case(0, 1, 2048, 2560, [16, 128], 16, 0, 'gather', (256, 1, 64), **_S),                # (e)
    _case(0, 1, 2048, 2560, [128], 16, B, 'refused', None, **_S),                           # (f)
    _case(0, 1, 2048, 2560, [128], 16, CONV_F16, 'refused', None, **_S),                    # (f)
]
SINGLE_LETTER = dict(zip((c['id'] for c in SINGLE_CASES), 'abcdeff'))
# added to the id a base block is seeded from: (a) must show the loss of the LAST dword of its view alone
SALT = {SINGLE_CASES[0]['id']: '+SALT'}
CASES = VIEW_CASES + SINGLE_CASES

# the value classes of tests/test_gpu_conv_exact_sweep.py: (A) bitwise, (B) F(4x4, 3x3): 4 x the emulation's worst ratio,
# (C) F(4x4, 2x2): 1e-4 of the output peak
VALUE_CLASS = {'gather': 'A', 'halo': 'A', 'emu': 'A', 'wino': 'A', 'wino80': 'A', 'wino2': 'A', 'wino2t': 'A',
               'wino4': 'B', 'wino80f4': 'B', 'wino42t': 'C', 'wino42s': 'C'}


def out_period(kind, R):
    return R if kind == 0 else (R // 2 if kind == 1 else 2 * R)


def expect_index(kind, size, R):
    """int64 [output size]: for every output coordinate of a map of `size` = k R (k >= 2) input pixels along one axis, the
    output coordinate of the 3R map tile(base, 3) that holds the same value (module docstring)."""
    assert size % R == 0 and size >= 2 * R and R % 2 == 0
    p = out_period(kind, R)
    o = torch.arange(out_period(kind, size))
    blocks = size // R
    b = o // p
    return o % p + p * torch.where(b == 0, 0, torch.where(b == blocks - 1, 2, 1))


def base_inputs(c, R=None):
    """The base block of a case, seeded from its id: (srcs, weight) of exact_conv_case for P_VIEWS views of R x R pixels."""
    R = R or c['R']
    rng = np.random.default_rng(zlib.crc32((c['id'] + SALT.get(c['id'], '')).encode()))
    return o64.exact_conv_case(rng, c['kind'], P_VIEWS, R, R, c['cins'], c['c_out'])


def repeat_sources(srcs, ky, kx, views=None):
    """The sources with every view's map repeated ky x kx times (and, with `views`, view n = base view n mod P)."""
    out = []
    for raw, sc, sh, act in srcs:
        raw = raw.repeat(1, 1, ky, kx)
        if views is not None:
            pick = torch.arange(views) % raw.shape[0]
            raw, sc, sh = raw[pick], sc[pick], sh[pick]
        out.append((raw, sc, sh, act))
    return out


def small_reference(c, R=None):
    """(srcs3, weight, ref): the base block repeated 3 x 3, its float64 convolution ref [P, c_out, 3p, 3p]."""
    srcs, w = base_inputs(c, R)
    srcs3 = repeat_sources(srcs, 3, 3)
    return srcs3, w, o64.conv64(c['kind'], srcs3, w)


def gather_expected(small, kind, H, W_, R, views=None):
    """small [P, C, 3p, 3p] -> [views or P, C, OH, OW]: the expectation of the large map by expect_index on both axes."""
    iy, ix = expect_index(kind, H, R), expect_index(kind, W_, R)
    big = small[:, :, iy][:, :, :, ix]
    return big if views is None else big[torch.arange(views) % small.shape[0]]


def halo_crossing(c):
    """The boundary arithmetic of the halo kernels on a single-view case (3x3).  Dword (channel) k of pixel p (index inside
    the view) of a source of C padded channels sits at byte (p * C + k) * 4 of the resource; the resource's range is 0x7fffffff
    bytes and the hardware answers a dword outside it with zero.  Which dwords that is depends on how the range check treats
    the END of a dword:
      'inclusive'   a dword is lost when it ends beyond byte 0x7fffffff, i.e. begins at 2^31 - 4 or later
      'exclusive'   only a dword that BEGINS at byte 2^31 or later is lost
    For each reading: the first output row that reads a lost dword, or None when none is lost — the first input row with a
    pixel whose LAST dword is lost, minus one: a 3x3 window reads the rows y - 1 .. y + 1, so every output row from there to
    the last is wrong.  (The hardware: 'inclusive'.)"""
    assert c['kind'] == 0 and c['N'] == 1
    H, W_ = c['H'], c['W']
    res = {}
    for name, limit in (('inclusive', RSRC_BYTES - 4), ('exclusive', (1 << 31) - 1)):
        first = None
        for C in (pad16(x) for x in c['cins']):
            # the last dword of pixel p begins at (p * C + C - 1) * 4: the first pixel where that lies beyond `limit`
            p = max(0, -(-(limit + 1 - (C - 1) * 4) // (C * 4)))
            if p < H * W_:
                row = p // W_
                first = row if first is None else min(first, row)
        res[name] = None if first is None else max(first - 1, 0)
    return res
