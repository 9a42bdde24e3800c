"""-m gpu: the VALUES an unmasked convolution launch computes, for every kernel plan — one id per row of the plan table
oracle/conv_guard_cases.CASES (every launcher of CONV_TILES x kind x emulation format, the split-K rows and the slice that
straddles the concat included), on the EXACT inputs of oracle.conv64.exact_conv_case, against the float64 convolution
oracle.conv64.conv64.  tests/test_conv_exact_cpu.py proves on the CPU what this module rests on: that the inputs are exact on
every case used, that every case lands on the row it names, and that the two sweeps below cover every reachable launcher.

(A) BITWISE — the rows whose Winograd tile is not 4: gather, halo, emu (both formats), wino, wino80, wino2, wino2t.
    Integer activations in [-3, 3], scales in {1/2, 1, 2}, shifts multiples of 1/2, weights multiples of 2^-3: every product
    is a multiple of 2^-4 and every partial sum fits float32's significand, so any summation order, the F(2x2, 3x3) and
    F(2x2, 2x2) transforms (the data transforms only add, the weight transforms divide by 2 and 4), the bf16x6 / f16x3 operand
    splits and the sums of split-K slabs all give conv64(...).float() exactly.  out_raw — prefilled with a NaN whose payload is
    the element index — is compared with it as int32: no tolerance appears anywhere in (A).  A transposed tap order, a swapped
    phase or parity class, a halo staged from the wrong row fail, and the message names the workgroup tile and the position
    inside it.
    The activation of a source is NONE or ReLU, as exact_conv_case draws it: LeakyReLU's 0.2 is not dyadic, so that
    activation stays with the Gaussian tests (test_gpu_unet.py, test_gpu_conv_guard.py).

(B) BOUNDED PER ELEMENT — the F(4x4, 3x3) kernels conv_wino4_kernel (the three wino4 rows of the table) and
    conv_wino80f4_kernel (the row k0-256x16x16-16+16-78-f88, the smallest case of tests/test_gpu_conv_wino80f4.py).
    Their weight transform divides by 81/64, 243/128, ... : no choice of inputs makes them exact.  On exact inputs the
    float64 reference is exact, so the whole error is the kernel's, and the magnitude map A = conv64(|input|, |w|) is known
    per element:
        |got - ref| <= c * EPS * A,   EPS = 2^-24,   and got == 0 exactly where A == 0.
    c is not chosen: it is 4 x the worst |err| / (EPS * A) of oracle.conv64.wino4_f32 on the SAME inputs, a float32 numpy
    emulation of the algorithm (U = G g G^T in float64 rounded once; input transform, accumulation two channels per step and
    output transform in float32) — what float32 arithmetic alone costs F(4x4, 3x3) on these points.  The kernels accumulate in
    MFMA steps of another width and add split-K slabs, a different draw of the same rounding process; the factor 4 covers that.

(C) F(4x4, 2x2) — conv_wino42p_kernel (family wino42t, the row k2-64x16x32-16+16-64-f40) and conv_wino42s_kernel (wino42s,
    k1-64x32x64-16-256-f136), the first case of each kernel's own test module, on exact inputs at the existing gate of 1e-4 of
    the output peak; the ratio |err| / (EPS * A) is recorded, no new bound.

(B) and (C) select their rows BY ID: the 4x emulation bound and the figures below were measured on exactly these cases.  The
table's other five F(4x4, .) rows (NOT_VALUE_SWEPT: the guard-sweep rows of wino42t, wino42s and wino80f4) get no value test
here — a bound for them would rest on numbers nobody has measured; their values are held by the Gaussian tests of the kernels'
own modules, and the CPU twin holds that every row is in (A), (B), (C) or that list.

Worst |err| / (EPS * A) per case (profiles/conv_exact_sweep.txt has the same table with a reading of it); the emulation on the
CPU, the kernels on an MI355X:
    kernel                 case                           emulation   allowed (4 x)   measured   max error of the peak
    conv_wino4_kernel      k0-16x64x64-16-128-f24         12.1        48.6            13.8       7.69e-07
    conv_wino4_kernel      k0-64x16x32-16-256-f24         12.1        48.3            14.5       7.02e-07
    conv_wino4_kernel      k0-2x64x64-128-512-f24         6.56        26.2            7.11       1.29e-06     (split-K)
    conv_wino80f4_kernel   k0-256x16x16-16+16-78-f88      8.45        33.8            10.5       7.94e-07
    conv_wino42p_kernel    k2-64x16x32-16+16-64-f40       -           -               108        1.04e-06     (gate: 1e-4 of the peak)
    conv_wino42s_kernel    k1-64x32x64-16-256-f136        -           -               18         1.28e-06     (gate: 1e-4 of the peak)
"""
import ctypes
import functools
import zlib

import numpy as np
import pytest
import torch

from oracle import conv64 as o64
from oracle import conv_guard_cases as cg
from rnr_amd import _lib
from rnr_amd.testing import conv_desc, pad16, run_conv, run_conv_fused
from test_gpu_conv_mask_sweep import nhwc_padded, prefill

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24
ALL_CASES = cg.CASES


def _rows(family, *ids):
    rows = [c for c in cg.CASES if c['family'] == family and c['id'] in ids]
    assert len(rows) == len(ids), 'the plan table has lost a %s row this sweep selects: %s' % (family, ids)
    return rows


# (A) every row of the table but the F(4x4, .) ones
BITWISE_CASES = [c for c in cg.CASES if c['m'] != 4]
# (B) the wino4 rows (unsplit, one tile per view, split-K) and the smallest case of tests/test_gpu_conv_wino80f4.py
F4_CASES = [c for c in cg.CASES if c['family'] == 'wino4'] + _rows('wino80f4', 'k0-256x16x16-16+16-78-f88')
# (C) the first case of tests/test_gpu_conv_wino42p.py and of tests/test_gpu_conv_wino42s.py
F42_CASES = _rows('wino42t', 'k2-64x16x32-16+16-64-f40') + _rows('wino42s', 'k1-64x32x64-16-256-f136')
# the F(4x4, .) rows without a value test here (module docstring): the guard sweep's other rows of the three newest kernels
NOT_VALUE_SWEPT = {'wino42t': ('k2-16x32x64-16+32-64-f40', 'k2-64x16x32-16-64-f40'), 'wino42s': ('k1-32x64x128-16+32-128-f136',),
                   'wino80f4': ('k0-256x16x16-16+32-78-f88', 'k0-4x128x128-20-78-f88')}


def exact_inputs(c):
    """The exact inputs of a case, seeded from its id: the same here and in tests/test_conv_exact_cpu.py."""
    rng = np.random.default_rng(zlib.crc32(c['id'].encode()))
    return o64.exact_conv_case(rng, c['kind'], c['N'], c['H'], c['W'], c['cins'], c['c_out'])


@functools.lru_cache(maxsize=4)
def _reference(cid):
    c = next(x for x in ALL_CASES if x['id'] == cid)
    srcs, w = exact_inputs(c)
    return srcs, w, o64.conv64(c['kind'], srcs, w)


def locate(c, n, y, x, col):
    """Where output element (view, y, x, column) sits in the launch of case `c`, in words: the workgroup's pixel tile and the
    position inside it — in the GEMM row space the tiles are counted in (output pixels; for the transposed convolution the
    input pixel y // 2, x // 2 of output parity class (y % 2, x % 2)) — the Winograd patch and the position inside it, the
    column tile and the column inside it."""
    tw, th, bn = c['tile']
    oh, ow = cg.out_hw(c['kind'], c['H'], c['W'])
    s = ''
    gy, gx, gh, gw = y, x, oh, ow
    if c['kind'] == 2:
        s = 'parity class (%d, %d), class pixel (%d, %d): ' % (y % 2, x % 2, y // 2, x // 2)
        gy, gx, gh, gw = y // 2, x // 2, c['H'], c['W']
    if c['family'] == 'gather':
        row = (n * gh + gy) * gw + gx
        s += 'gather tile %d (of %d GEMM rows), row %d inside it' % (row // tw, tw, row % tw)
    else:
        s += 'tile (row %d, column %d) of %d x %d pixels in view %d, position (%d, %d) inside it' % (
            gy // th, gx // tw, tw, th, n, gy % th, gx % tw)
        m = c['m']
        if m:
            s += '; F(%dx%d) patch (%d, %d) of the tile, output (%d, %d) of the patch' % (
                m, m, gy % th // m, gx % tw // m, gy % m, gx % m)
            if c['kind'] == 1:
                s += ' (every output sums the four input parity phases)'
    return s + '; column tile %d, column %d inside it' % (col // bn, col % bn)


def spread(c, bad):
    """One line on HOW the failing elements `bad` (rows of (view, y, x, column)) are spread: over the views, the output
    parity classes (transposed convolution), the workgroup tiles and the positions inside a tile — a wrong tile decode fails
    whole tiles, a wrong halo or tap the same positions of every tile, a swapped parity class one class only."""
    tw, th, _ = c['tile']
    n, y, x = bad[:, 0], bad[:, 1], bad[:, 2]
    s = '%d of %d views' % (n.unique().numel(), c['N'])
    if c['kind'] == 2:
        s += '; parity classes (y %% 2, x %% 2) %s' % [(int(p) // 2, int(p) % 2) for p in (y % 2 * 2 + x % 2).unique()]
        y, x = y // 2, x // 2
    gh, gw = (c['H'], c['W']) if c['kind'] == 2 else cg.out_hw(c['kind'], c['H'], c['W'])
    if c['family'] == 'gather':
        row = (n * gh + y) * gw + x
        return s + '; %d of %d gather tiles, %d of %d rows inside a tile' % (
            (row // tw).unique().numel(), -(-(c['N'] * gh * gw) // tw), (row % tw).unique().numel(), min(tw, c['N'] * gh * gw))
    tiles = ((n * (gh // th) + y // th) * (gw // tw) + x // tw).unique().numel()
    inside = ((y % th) * tw + x % tw).unique()
    s += '; %d of %d tiles, %d of %d positions inside a tile' % (tiles, c['N'] * (gh // th) * (gw // tw), inside.numel(), th * tw)
    if inside.numel() <= 8:
        s += ' %s' % [(int(p) // tw, int(p) % tw) for p in inside]
    return s


def launches(c, srcs, w):
    """rnr_conv2d once and rnr_conv2d_fused with BatchNorm twice on one sync buffer, both on an out_raw prefilled with the NaN
    index pattern: (out_raw of the legacy entry as int32, the fused entry's as int32).  Checks what holds for every plan: the
    algorithm and the split depth the case names, a sync buffer left at zero, padding columns +0.0, fused == legacy bitwise."""
    L = _lib.load()
    d = conv_desc(c['kind'], c['cins'], c['c_out'], c['flags'])
    assert L.rnr_conv_algorithm(ctypes.byref(d), c['N'], c['H'], c['W']) == c['algo']
    assert cg.split_depth(L, c) == c['split']
    co, cp = c['c_out'], pad16(c['c_out'])
    oh, ow = cg.out_hw(c['kind'], c['H'], c['W'])
    fill = prefill(c['N'], oh, ow, cp)
    args = (c['kind'], srcs, w, co, c['N'], c['H'], c['W'])
    legacy = run_conv(*args, flags=c['flags'], out=fill)[0].view(torch.int32)
    g = torch.Generator().manual_seed(co)
    gamma, beta = torch.rand(co, generator=g) + 0.5, torch.randn(co, generator=g)
    fused, _, _, sync = run_conv_fused(*args, gamma, beta, flags=c['flags'], repeats=2, out=fill)
    fused = fused.view(torch.int32)
    assert int(sync.to(torch.int32).abs().sum()) == 0, 'sync buffer not left at zero'
    if cp > co:
        assert int(legacy[..., co:].abs().max()) == 0, 'padding columns of out_raw are not +0.0'
    bad = (fused != legacy).nonzero()
    assert bad.shape[0] == 0, ('rnr_conv2d_fused differs from rnr_conv2d in %d elements, first (view, y, x, column) %s: %s' % (
        bad.shape[0], bad[0].tolist(), locate(c, *bad[0].tolist())))
    return legacy


# ---- (A) bitwise ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('c', BITWISE_CASES, ids=[c['id'] for c in BITWISE_CASES])
def test_exact_inputs_bitwise(c):
    """out_raw[..., :c_out] of rnr_conv2d and of rnr_conv2d_fused, as int32, equals conv64(...).float() as int32."""
    srcs, w, ref = _reference(c['id'])
    want = (nhwc_padded(ref, pad16(c['c_out'])) + 0.0).view(torch.int32)        # (+ 0.0: a sum that came out as -0.0 becomes +0.0)
    got = launches(c, srcs, w)
    bad = (got != want).nonzero()
    if bad.shape[0]:
        gf, wf = got.view(torch.float32), want.view(torch.float32)
        head = bad[:4096]                                                       # the first failing pixels, one element of each
        show = [head[(head[:, :3] == p).all(dim=1)][0] for p in head[:, :3].unique(dim=0)[:3]]
        first = ['(view, y, x, column) %s: got %r, want %r — %s' % (b.tolist(), gf[tuple(b)].item(), wf[tuple(b)].item(),
                                                                   locate(c, *b.tolist())) for b in show]
        pytest.fail('%s %s: %d of %d elements differ from the float64 convolution (%s); the first pixels:\n  %s' % (
            c['family'], c['tile'], bad.shape[0], got.numel(), spread(c, bad), '\n  '.join(first)))


# ---- (B), (C) the F(4x4, .) kernels -----------------------------------------------------------------------------------------

def ratio_map(out_nchw, ref, A):
    """|out - ref| / (EPS * A) per element (0 where A == 0) and the worst of it."""
    err = (out_nchw.double() - ref).abs()
    r = torch.where(A > 0, err / (EPS * A.clamp_min(1e-300)), torch.zeros_like(err))
    return r, float(r.max())


def emulation_ratio(c):
    """Worst |err| / (EPS * A) of the float32 emulation wino4_f32 on the exact inputs of an F(4x4, 3x3) case."""
    srcs, w, ref = _reference(c['id'])
    emu = o64.wino4_f32(o64.conv_input(srcs), w)
    return ratio_map(emu, ref, o64.magnitude64(c['kind'], srcs, w))[1]


def kernel_ratio(c):
    srcs, w, ref = _reference(c['id'])
    got = launches(c, srcs, w).view(torch.float32)
    assert bool(torch.isfinite(got).all()), 'out_raw kept prefill (NaN) elements'
    out = got[..., :c['c_out']].permute(0, 3, 1, 2)
    A = o64.magnitude64(c['kind'], srcs, w)
    assert bool((out[A == 0] == 0).all()), 'an output whose every product is zero is not exactly 0'
    r, worst = ratio_map(out, ref, A)
    at = [int(v) for v in (r == r.max()).nonzero()[0]]                          # (view, column, y, x)
    where = (at[0], at[2], at[3], at[1])
    peak = float((out.double() - ref).abs().max() / ref.abs().max())
    return worst, where, peak


@pytest.mark.parametrize('c', F4_CASES, ids=[c['id'] for c in F4_CASES])
def test_f4x4_3x3_exact_inputs_per_element_bound(c):
    """|got - ref| <= 4 * (the emulation's worst ratio on these inputs) * EPS * A for every element (module docstring, (B))."""
    L = _lib.load()
    d = conv_desc(c['kind'], c['cins'], c['c_out'], c['flags'])
    assert L.rnr_conv_winograd_tile(ctypes.byref(d), c['N'], c['H'], c['W']) == 4
    emu = emulation_ratio(c)
    worst, where, peak = kernel_ratio(c)
    print('\nF4 %s %s: emulation %.3g, allowed %.3g, measured %.3g (max error %.3g of the peak)' % (
        c['family'], c['id'], emu, 4 * emu, worst, peak))
    assert worst <= 4 * emu, ('worst |err| / (EPS * A) = %.3g > 4 x %.3g at (view, y, x, column) %s: %s' % (
        worst, emu, where, locate(c, *where)))


@pytest.mark.parametrize('c', F42_CASES, ids=[c['id'] for c in F42_CASES])
def test_f4x4_2x2_exact_inputs_at_the_existing_gate(c):
    """Exact inputs through conv_wino42p_kernel / conv_wino42s_kernel: max |err| < 1e-4 of the output peak (the gate of the
    kernels' own modules); |err| / (EPS * A) is printed for the record."""
    L = _lib.load()
    d = conv_desc(c['kind'], c['cins'], c['c_out'], c['flags'])
    assert L.rnr_conv_winograd_tile(ctypes.byref(d), c['N'], c['H'], c['W']) == 4
    worst, where, peak = kernel_ratio(c)
    print('\nF42 %s %s: measured %.3g (max error %.3g of the peak) at %s' % (c['family'], c['id'], worst, peak, where))
    assert peak < 1e-4, peak
