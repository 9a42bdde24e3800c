"""-m gpu: the convolution entry points that take a TILE MASK (rnr_conv_active_tiles, rnr_conv2d_masked, rnr_conv2d_fused with
a mask) or carry the RAY-RENDERER EPILOGUE (rnr_conv2d_ray), kernel by kernel, against the float64 restatements of
oracle/conv64.py — one row per tile plan that takes a mask (MASKED_CASES; tests/test_conv_mask_cpu.py checks on the CPU that
every row lands on the tile it names).

What a masked launch is held to:
  * out_raw is prefilled with a per-element int32 pattern that is a NaN, and everything is compared as int32: a dead tile
    keeps its pattern bit for bit, a live tile equals the all-ones launch bit for bit, a forgotten store is non-finite;
  * masks are NOT derived from an alpha map: all ones, all zeros, checkerboard, Bernoulli(0.5), only the first / only the last
    tile of every view — a wrong tile index -> (view, y0, x0) mapping in a kernel's early-out moves a tile border;
  * EXACT inputs (oracle.conv64.exact_conv_case): small dyadic values whose convolution is exact in float32 in any summation
    order, through the Winograd transforms and the bf16x6 / f16x3 splits.  Live tiles equal conv64(...).float() BITWISE: no
    tolerance, no second run of the code under test — a tile that reads its halo from the wrong view, row or column fails.

The ray epilogue.  image[n,c,y,x] = sum_r (tanh(y_r) + 1) * w_r with y_r = conv[3r+c] + bias[3r+c], R = c_out / 3 rays.  With
y_r exact in float32 (exact inputs, dyadic bias) the kernel differs from float64 by, per term and with EPS = 2^-24:
    fast_tanh_plus1f     <= 30 EPS absolute on tanh + 1 in [0, 2] (exp2 and rcp at 1 ulp: the figure tests/test_gpu_shade_sweep.py
                         holds rnr_ray_render to), plus EPS |y_r| for the argument (one float32 rounding of conv + bias when the
                         sum is not exact; d tanh / dy <= 1),
    the product          one rounding, <= EPS * 2 |w_r|,
    the sum over r       R - 1 sequential float32 additions of terms <= 2 |w_r|: <= (R - 1) EPS * 2 sum_r |w_r|, taken as 2 R EPS,
hence  |image - image64| <= EPS * (30 + max_r |y_r| + 2 R) * sum_r |w_r|   (RAY_BOUND).  Pixels whose ray_w row is all zero
give exactly 0.0.  With Gaussian inputs the convolution itself carries the direct kernels' 1e-4 * peak (test_conv_vs_torch);
tanh is 1-Lipschitz, so that adds sum_r |w_r| * 1e-4 * peak(conv64) — and nothing when the reference is the epilogue formula
applied to the GPU's own rnr_conv2d output.

Measured on an MI355X, worst error / bound per case (N, H, W, c_out); (e) exact inputs, (f) Gaussian inputs against conv64,
(f') against the GPU's own convolution, (g) test_ray_epilogue_saturation:
    case            (e)     (f)       (f')    (g) saturated bias columns
    1x8x32-66       0.036   0.00035   0.027   0.012
    1x8x32-72       0.028   0.00041   0.026   0.012
    1x8x32-78       0.024   0.00038   0.029   0.013
    2x16x96-66      0.047   0.00047   0.038   0.02
    2x16x96-72      0.043   0.00044   0.037   0.018
    2x16x96-78      0.036   0.00064   0.037   0.023
    3x96x320-66     0.045   0.00064   0.064   0.033
    3x96x320-72     0.055   0.00069   0.063   0.031
    3x96x320-78     0.046   0.00059   0.048   0.023
(f) is small because its bound is dominated by the 1e-4 * peak the convolution is allowed; (e), (f') and (g) show that the
derived budget has a factor of 15 or more in hand (its terms are worst cases: 30 EPS for the tanh, every addition of the
sequential sum rounding the same way).
"""
import ctypes
import functools
from collections import namedtuple

import numpy as np
import pytest
import torch

from oracle import conv64 as o64
from rnr_amd import _lib
from rnr_amd.testing import conv_active_tiles, conv_desc, run_conv, run_conv_fused, run_conv_ray

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24
WINO, BF16X6, F16X3 = _lib.CONV_WINOGRAD, _lib.CONV_F32_EMU_BF16X6, _lib.CONV_F32_EMU_F16X3

MaskCase = namedtuple('MaskCase', 'id N H W cins c_out flags th tw tol')
# every tile plan plan_conv gives a masked launch (all 3x3; at the default tuning).  tol: what the project holds that kernel
# family to against a float64 convolution, as a fraction of the output peak (test_conv_vs_torch / test_conv_f32_emulation: 1e-4,
# test_conv_winograd_vs_torch: 3e-5).  Base map 3 x 96 x 320 = 360 tiles of 32 x 8: no grid below 257 workgroups (those split K
# and take no mask).  All rows landed on the tile named here as first written (test_conv_mask_cpu.py::test_plan_geometry).
MASKED_CASES = [
    #         id             N  H   W    cins      c_out flags th tw  tol
    MaskCase('wino80',       3, 96, 320, [16, 16], 78,  WINO, 4, 16, 3e-5),      # conv_wino80_kernel: 1440 tiles of 16 x 4
    MaskCase('wino80_72',    4, 64, 64,  [20],     72,  WINO, 4, 16, 3e-5),      # 256 tiles: the smallest grid it takes, 72 live columns
    MaskCase('halo80',       3, 96, 320, [16, 16], 78,  0,    8, 32, 1e-4),      # 32 x 8 x 80
    MaskCase('halo64_4',     3, 96, 320, [20],     48,  0,    4, 32, 1e-4),      # 32 x 4 x 64 (<= 1024 tiles of 32 x 8), 48 live columns
    MaskCase('halo64_8',     9, 96, 320, [16],     16,  0,    8, 32, 1e-4),      # 32 x 8 x 64 (1080 tiles), 16 columns of 64
    MaskCase('halo128_4',    3, 96, 320, [16],     128, 0,    4, 32, 1e-4),      # 32 x 4 x 128 (720 tiles: over the 512 of the next row)
    MaskCase('halo128_8',    3, 96, 320, [16],     256, 0,    8, 32, 1e-4),      # 32 x 8 x 128, two column tiles (720 workgroups >= 512)
    MaskCase('halo64_cfg4',  2, 96, 320, [16],     128, 0,    4, 32, 1e-4),      # 32 x 4 x 64, two column tiles (480 tiles <= 512)
    MaskCase('halo64_2',     1, 64, 160, [16],     128, 0,    2, 32, 1e-4),      # 32 x 2 x 64, two column tiles (80 tiles of 32 x 4 < 128)
] + [MaskCase('%s_%s' % (name, fmt), 3, 96, 320, cins, c_out, _lib.EMU_FLAGS[fmt], 8, 32, 1e-4)
     for name, cins, c_out in (('emu96', [16, 16], 78), ('emu64', [20], 48), ('emu128', [16], 128))      # conv_halo_emu_kernel, 32 x 8
     for fmt in ('bf16x6', 'f16x3')]

# shapes plan_conv must refuse a mask for: kind, N, H, W, cins, c_out
REFUSED_CASES = [
    (1, 1, 64, 64, [16], 128),          # 4x4 stride 2
    (2, 1, 64, 64, [16], 128),          # transposed
    (0, 1, 64, 16, [16], 128),          # a map 16 pixels wide: the 16-wide tiles
    (0, 1, 24, 48, [16], 128),          # no halo tile fits: the gather kernel
    (0, 1, 64, 64, [64], 64),           # a grid that splits K
]

RayCase = namedtuple('RayCase', 'N H W cins c_out')
RAY_CASES = [RayCase(N, H, W, cins, c_out) for N, H, W in ((1, 8, 32), (2, 16, 96), (3, 96, 320))
             for cins, c_out in (([16, 16], 66), ([20], 72), ([16, 16], 78))]
ray_id = lambda c: '%dx%dx%d-%d' % (c.N, c.H, c.W, c.c_out)


def _seed(*key):
    return sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31)


def gaussian_case(kind, N, H, W, cins, c_out):
    """The inputs of test_gpu_unet.py::test_conv_vs_torch."""
    g = torch.Generator().manual_seed(kind * 100 + H + c_out)
    srcs = []
    for j, C in enumerate(cins):
        raw = torch.randn(N, C, H, W, generator=g)
        sc = torch.rand(N, C, generator=g) + 0.5 if j == 0 else None
        sh = torch.randn(N, C, generator=g) * 0.3
        srcs.append((raw, sc, sh, 1 if j == 0 else 2))
    cin = sum(cins)
    k = 3 if kind == 0 else 4
    w = torch.randn(c_out, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    return srcs, w


def exact_case(N, H, W, cins, c_out):
    """The exact inputs of a shape: the same in the CPU module (exactness property) and here."""
    return o64.exact_conv_case(np.random.default_rng(_seed(N, H, W, sum(cins), c_out)), 0, N, H, W, cins, c_out)


def nhwc_padded(ref_nchw, c_pad, dtype=torch.float32):
    """conv64's [N,C,H,W] -> out_raw's layout [N,H,W,c_pad] with zero padding columns."""
    N, C, H, W = ref_nchw.shape
    out = torch.zeros(N, H, W, c_pad, dtype=dtype)
    out[..., :C] = ref_nchw.permute(0, 2, 3, 1).to(dtype)
    return out


def prefill(N, H, W, c_pad):
    """int32 [N,H,W,c_pad]: a quiet NaN whose payload is the element index."""
    idx = torch.arange(N * H * W * c_pad, dtype=torch.int64)
    return (0x7fc00000 | (idx & 0x3fffff)).to(torch.int32).reshape(N, H, W, c_pad)


def named_masks(c):
    """Tile masks [N, H/th, W/tw] that no alpha map produced."""
    ty, tx = c.H // c.th, c.W // c.tw
    yy, xx = torch.meshgrid(torch.arange(ty), torch.arange(tx), indexing='ij')
    checker = (((yy + xx) % 2) == 1).to(torch.uint8)
    first, last = torch.zeros(ty, tx, dtype=torch.uint8), torch.zeros(ty, tx, dtype=torch.uint8)
    first[0, 0] = 1
    last[-1, -1] = 1
    per_view = lambda m: m[None].repeat(c.N, 1, 1)
    bern = (torch.rand(c.N, ty, tx, generator=torch.Generator().manual_seed(_seed(c.N, ty, tx))) < 0.5).to(torch.uint8)
    return {'zeros': torch.zeros(c.N, ty, tx, dtype=torch.uint8), 'checkerboard': per_view(checker), 'bernoulli': bern,
            'first': per_view(first), 'last': per_view(last)}


def pixels_of(mask, th, tw):
    """tile mask [N, ty, tx] -> bool [N, H, W, 1]"""
    return mask.bool().repeat_interleave(th, dim=1).repeat_interleave(tw, dim=2)[..., None]


def launch(entry, c, srcs, w, tile_mask, out, masked=True):
    """One launch of case `c` through 'masked' (rnr_conv2d_masked) or 'fused' (rnr_conv2d_fused without BatchNorm); a NULL mask
    when tile_mask is None.  Returns out_raw as int32; the fused entry's sync buffer must come back all zero."""
    tm = None if tile_mask is None else tile_mask.reshape(-1)
    if entry == 'masked':
        got = run_conv(0, srcs, w, c.c_out, c.N, c.H, c.W, flags=c.flags, tile_mask=tm, out=out, masked=masked)[0]
    else:
        got, _, _, sync = run_conv_fused(0, srcs, w, c.c_out, c.N, c.H, c.W, flags=c.flags, tile_mask=tm, out=out)
        assert int(sync.to(torch.int32).abs().sum()) == 0, 'sync buffer not left at zero'
    return got.view(torch.int32)


# ---- (a) rnr_conv_active_tiles ----------------------------------------------------------------------------------------------

def _geometries():
    seen = {}
    for c in MASKED_CASES:
        seen.setdefault((c.th, c.tw, c.N, c.H, c.W), c)
    return list(seen.values())


def alpha_map(c):
    """alpha [N,H,W] float32 and the liveness the construction implies [N, ty, tx].  The first view (the upper half of the map when
    there is one view only): exactly one pixel > 0 in every tile, cycling through the four corners and an interior pixel.  A
    middle view, when there are three: all zero.  The last view (the lower half of a single view): zero except its very last
    pixel, and a handful of tiles that hold only -1.0, only -0.0 (inactive) or one 1.2e-38 (active: the smallest normal
    float32 is 1.18e-38).  Views in between: one pixel in a Bernoulli(0.3) choice of tiles."""
    N, H, W, th, tw = c.N, c.H, c.W, c.th, c.tw
    ty, tx = H // th, W // tw
    a = np.zeros((N, H, W), np.float32)
    live = np.zeros((N, ty, tx), bool)
    spots = [(0, 0), (0, tw - 1), (th - 1, 0), (th - 1, tw - 1), (th // 2, tw // 2)]
    one_view = N == 1
    first_rows = ty // 2 if one_view else ty            # tile rows of the 'one pixel per tile' region
    k = 0
    for j in range(first_rows):
        for i in range(tx):
            dy, dx = spots[k % 5]
            a[0, j * th + dy, i * tw + dx] = 0.25 + k
            live[0, j, i] = True
            k += 1
    rng = np.random.default_rng(_seed(N, H, W, th, tw))
    for n in range(2, N - 1):                           # views between the all-zero one and the last
        for j in range(ty):
            for i in range(tx):
                if rng.random() < 0.3:
                    a[n, j * th + rng.integers(th), i * tw + rng.integers(tw)] = 1.0
                    live[n, j, i] = True
    last, j0 = N - 1, (first_rows if one_view else 0)   # the 'last view' region: tile rows j0 ... ty - 1 of view N - 1
    a[last, H - 1, W - 1] = 1.0
    live[last, ty - 1, tx - 1] = True
    free = [(j, i) for j in range(j0, ty) for i in range(tx) if (j, i) != (ty - 1, tx - 1)]
    picks = [free[p] for p in rng.permutation(len(free))[:12]]
    for p, (j, i) in enumerate(picks):
        tile = a[last, j * th:(j + 1) * th, i * tw:(i + 1) * tw]
        if p % 4 == 0:
            tile[:] = -1.0
        elif p % 4 == 1:
            tile[:] = -0.0
        elif p % 4 == 2:
            tile[:] = 0.0
            tile[rng.integers(th), rng.integers(tw)] = -1.0
        else:
            tile[rng.integers(th), rng.integers(tw)] = 1.2e-38
            live[last, j, i] = True
    return a, live


@pytest.mark.parametrize('c', _geometries(), ids=lambda c: '%dx%d-%dx%dx%d' % (c.th, c.tw, c.N, c.H, c.W))
def test_active_tiles_equal_tile_mask64(c):
    """rnr_conv_active_tiles == tile_mask64 exactly on the alpha maps of alpha_map(): every entry 0 or 1, in (view, tile row,
    tile column) order, and not one byte written past the last tile (64 guard bytes keep their 0xAA)."""
    alpha, live = alpha_map(c)
    want = o64.tile_mask64(torch.from_numpy(alpha), c.th, c.tw)
    assert torch.equal(want, torch.from_numpy(live.reshape(-1)).to(torch.uint8)), 'tile_mask64 disagrees with the construction'
    assert np.isfinite(alpha).all() and not ((alpha != 0) & (np.abs(alpha) < 1.17549435e-38)).any()     # no NaN, no denormals
    tiles = c.N * (c.H // c.th) * (c.W // c.tw)
    buf = conv_active_tiles(conv_desc(0, c.cins, c.c_out, c.flags), alpha, c.N, c.H, c.W, guard=64, fill=0xAA)
    assert buf.numel() == tiles + 64
    got = buf[:tiles]
    assert int(got.max()) <= 1, 'entries other than 0 and 1'
    wrong = (got != want).nonzero().reshape(-1)
    assert wrong.numel() == 0, ('tiles differ', wrong[:8].tolist())
    assert bool((buf[tiles:] == 0xAA).all()), 'bytes behind the mask were written'


# ---- (b) masked launches, Gaussian inputs -----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _gaussian(cid):
    c = next(x for x in MASKED_CASES if x.id == cid)
    srcs, w = gaussian_case(0, c.N, c.H, c.W, c.cins, c.c_out)
    return srcs, w, o64.conv64(0, srcs, w).permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize('entry', ['masked', 'fused'])
@pytest.mark.parametrize('c', MASKED_CASES, ids=lambda c: c.id)
def test_masked_launch_gaussian(c, entry):
    """A masked launch through rnr_conv2d_masked / rnr_conv2d_fused(bn = NULL, tile_mask): the all-ones mask matches conv64 to
    the family's tolerance with exactly zero padding columns and equals the NULL-mask launch of the same entry point bitwise
    (every family here takes a mask, so the masked plan picks the same kernel); under every other mask live tiles — all
    c_out_pad columns, across column tiles — equal the all-ones launch bitwise and dead tiles still hold the prefill pattern;
    the all-zeros launch succeeds and touches nothing."""
    srcs, w, ref = _gaussian(c.id)
    cp = (c.c_out + 15) // 16 * 16
    fill = prefill(c.N, c.H, c.W, cp)
    ones = torch.ones(c.N, c.H // c.th, c.W // c.tw, dtype=torch.uint8)
    full = launch(entry, c, srcs, w, ones, fill)
    full_f = full.view(torch.float32)
    assert torch.isfinite(full_f).all(), 'a live tile kept prefill (NaN) elements'
    peak = float(ref.abs().max())
    err = float((full_f[..., :c.c_out].double() - ref).abs().max())
    print('%s %s: max error %.3g = %.3g of the peak (tolerance %.0e)' % (c.id, entry, err, err / peak, c.tol))
    assert err < c.tol * peak, (err, peak)
    assert cp == c.c_out or int(full[..., c.c_out:].abs().max()) == 0, 'padding columns are not +0.0'
    null = launch(entry, c, srcs, w, None, fill)
    assert torch.equal(null, full), 'all-ones mask and NULL mask differ'
    for name, mask in named_masks(c).items():
        got = launch(entry, c, srcs, w, mask, fill)
        want = torch.where(pixels_of(mask, c.th, c.tw), full, fill)
        bad = (got != want).nonzero()
        assert bad.shape[0] == 0, (name, '%d elements differ, first (n, y, x, column):' % bad.shape[0], bad[:4].tolist())
    assert torch.equal(fill, prefill(c.N, c.H, c.W, cp))


# ---- (c) masked launches, exact inputs --------------------------------------------------------------------------------------

@pytest.mark.parametrize('entry', ['masked', 'fused'])
@pytest.mark.parametrize('c', MASKED_CASES, ids=lambda c: c.id)
def test_masked_launch_exact_inputs_bitwise(c, entry):
    """Exact inputs (module docstring) under the Bernoulli mask: live tiles equal conv64(...).float() BITWISE (padding columns
    +0.0), dead tiles the prefill.  Nothing here depends on another run of the code under test."""
    srcs, w = exact_case(c.N, c.H, c.W, c.cins, c.c_out)
    cp = (c.c_out + 15) // 16 * 16
    ref = nhwc_padded(o64.conv64(0, srcs, w), cp) + 0.0            # (+ 0.0: a float64 sum that came out as -0.0 becomes +0.0)
    fill = prefill(c.N, c.H, c.W, cp)
    mask = named_masks(c)['bernoulli']
    assert 0.3 < float(mask.float().mean()) < 0.7
    got = launch(entry, c, srcs, w, mask, fill)
    want = torch.where(pixels_of(mask, c.th, c.tw), ref.view(torch.int32), fill)
    bad = (got != want).nonzero()
    assert bad.shape[0] == 0, ('%d elements differ, first (n, y, x, column):' % bad.shape[0], bad[:4].tolist(),
                               [(got[tuple(b)].item(), want[tuple(b)].item()) for b in bad[:4]])


# ---- (d) refusals (host-side argument checks: nothing is launched) ----------------------------------------------------------

@pytest.mark.parametrize('kind,N,H,W,cins,c_out', REFUSED_CASES)
def test_mask_is_refused_where_the_plan_has_no_maskable_tiles(kind, N, H, W, cins, c_out):
    L = _lib.load()
    d = conv_desc(kind, cins, c_out)
    assert L.rnr_conv_tile_count(ctypes.byref(d), N, H, W) == 0
    srcs = [(torch.zeros(N, C, H, W), None, None, 0) for C in cins]
    k = 3 if kind == 0 else 4
    w = torch.zeros((sum(cins), c_out, 4, 4) if kind == 2 else (c_out, sum(cins), k, k))
    with pytest.raises(_lib.RnrError, match='maskable'):
        run_conv(kind, srcs, w, c_out, N, H, W, tile_mask=torch.ones(N * H * W, dtype=torch.uint8))
    with pytest.raises(_lib.RnrError, match='maskable'):
        conv_active_tiles(d, torch.ones(N, H, W), N, H, W)


def test_mask_with_statistics_is_refused():
    """Skipped tiles would falsify batch statistics: a mask together with stats != NULL (rnr_conv2d_masked) or with a BatchNorm
    (rnr_conv2d_fused) is an error, and the fused entry's sync buffer is still all zero afterwards."""
    c = MASKED_CASES[2]
    srcs, w, _ = _gaussian(c.id)
    ones = torch.ones(c.N * (c.H // c.th) * (c.W // c.tw), dtype=torch.uint8)
    with pytest.raises(_lib.RnrError, match='statistics'):
        run_conv(0, srcs, w, c.c_out, c.N, c.H, c.W, tile_mask=ones, with_stats=True)
    sync = []
    with pytest.raises(_lib.RnrError, match='statistics'):
        run_conv_fused(0, srcs, w, c.c_out, c.N, c.H, c.W, torch.ones(c.c_out), torch.zeros(c.c_out), tile_mask=ones, sync_out=sync)
    assert len(sync) == 1 and sync[0].numel() > 0 and int(sync[0].max()) == 0


# ---- the ray epilogue -------------------------------------------------------------------------------------------------------

def ray_weights(c, rng, zero_rows=0.3):
    """ray_w [N,H,W,c_out_pad]: uniform in [-1, 1], about 30 % of the pixels with an all-zero row, columns >= c_out zero (as
    rnr_ray_weights leaves them)."""
    cp = (c.c_out + 15) // 16 * 16
    w = rng.uniform(-1.0, 1.0, size=(c.N, c.H, c.W, cp)).astype(np.float32)
    w[rng.random((c.N, c.H, c.W)) < zero_rows] = 0.0
    w[..., c.c_out:] = 0.0
    return torch.from_numpy(w)


def dyadic_bias(c, rng, length=None):
    """bias [c_out_pad] (rnr_conv2d_ray's contract): multiples of 2^-4 in [-2, 2]; the padding entries hold values too — they
    must not matter."""
    cp = (c.c_out + 15) // 16 * 16
    return torch.from_numpy((rng.integers(-32, 33, size=cp if length is None else length) / 16.0).astype(np.float32))


def ray_bound(y64, ray_w, c_out):
    """RAY_BOUND of the module docstring per output [N,3,H,W], from y = conv + bias [N,H,W,>=c_out] in float64."""
    R = c_out // 3
    ya = y64[..., :3 * R].abs().reshape(*y64.shape[:3], R, 3).amax(dim=3)
    ws = ray_w[..., :3 * R].double().abs().reshape(*ray_w.shape[:3], R, 3).sum(dim=3)
    return (EPS * (30.0 + ya + 2 * R) * ws).permute(0, 3, 1, 2), ws.permute(0, 3, 1, 2)


def check_image(tag, image, conv_nhwc64, bias, ray_w, c, extra=0.0):
    """image against ray_epilogue64 of the given convolution within RAY_BOUND (+ extra * sum |w|); all-zero rows give exactly
    0.0; prints the worst error / bound."""
    assert torch.isfinite(image).all(), 'non-finite pixels (or pixels the kernel never wrote)'
    ref = o64.ray_epilogue64(conv_nhwc64, bias, ray_w, c.c_out)
    y = conv_nhwc64[..., :c.c_out].double() + bias[:c.c_out].double()
    bound, ws = ray_bound(y, ray_w, c.c_out)
    bound = bound + extra * ws
    err = (image.double() - ref).abs()
    zero = ws == 0
    assert bool(zero.any()) and bool((image[zero] == 0).all()), 'a pixel without ray weights is not exactly 0'
    ratio = float((err[~zero] / bound[~zero]).max())
    print('%s %s: worst error / bound = %.2g (max error %.3g)' % (tag, ray_id(c), ratio, float(err.max())))
    assert ratio <= 1.0, (tag, ratio)
    return ratio


@pytest.mark.parametrize('c', RAY_CASES, ids=ray_id)
def test_ray_epilogue_exact_inputs(c):
    """(e) exact convolution inputs and a dyadic bias: y = conv + bias is exact in float32, the image is within RAY_BOUND of
    ray_epilogue64(conv64)."""
    rng = np.random.default_rng(_seed(c.N, c.H, c.c_out, 5))
    srcs, w = exact_case(c.N, c.H, c.W, c.cins, c.c_out)
    ray_w, bias = ray_weights(c, rng), dyadic_bias(c, rng)
    image = run_conv_ray(srcs, w, c.c_out, c.N, c.H, c.W, ray_w, bias)
    conv = o64.conv64(0, srcs, w).permute(0, 2, 3, 1)
    assert torch.equal((conv + bias[:c.c_out].double()).float().double(), conv + bias[:c.c_out].double())      # y exact in float32
    check_image('(e)', image, conv, bias, ray_w, c)


@pytest.mark.parametrize('c', RAY_CASES, ids=ray_id)
def test_ray_epilogue_gaussian_inputs(c):
    """(f) Gaussian inputs: against ray_epilogue64(conv64) within RAY_BOUND + sum |w| * 1e-4 * peak(conv64), and against
    ray_epilogue64 of the GPU's own rnr_conv2d output (the direct kernel of the same plan: the convolution error cancels) within
    RAY_BOUND alone."""
    rng = np.random.default_rng(_seed(c.N, c.H, c.c_out, 6))
    srcs, w = gaussian_case(0, c.N, c.H, c.W, c.cins, c.c_out)
    ray_w = ray_weights(c, rng)
    bias = torch.from_numpy(rng.normal(0.0, 0.5, size=ray_w.shape[-1]).astype(np.float32))
    bias[c.c_out:] = float('nan')                       # bias [c_out_pad]: the padding entries reach no output
    image = run_conv_ray(srcs, w, c.c_out, c.N, c.H, c.W, ray_w, bias)
    conv = o64.conv64(0, srcs, w).permute(0, 2, 3, 1)
    check_image('(f)', image, conv, bias, ray_w, c, extra=1e-4 * float(conv.abs().max()))
    own = run_conv(0, srcs, w, c.c_out, c.N, c.H, c.W)[0]
    check_image("(f')", image, own.double(), bias, ray_w, c)


@pytest.mark.parametrize('c', RAY_CASES, ids=ray_id)
def test_ray_epilogue_saturation(c):
    """(g) one ray's three bias columns at +90, another's at -90 (exact inputs): tanh + 1 comes out as exactly 2 and exactly 0 —
    with weights on those two rays only the image is 2 * w of the first, bit for bit — and with all weights the image is finite
    and within RAY_BOUND."""
    rng = np.random.default_rng(_seed(c.N, c.H, c.c_out, 7))
    srcs, w = exact_case(c.N, c.H, c.W, c.cins, c.c_out)
    ray_w, bias = ray_weights(c, rng), dyadic_bias(c, rng)
    R = c.c_out // 3
    hi, lo = 1, R - 1                                   # rays: columns 3 .. 5 and the last three live columns
    bias[3 * hi:3 * hi + 3] = 90.0
    bias[3 * lo:3 * lo + 3] = -90.0
    conv = o64.conv64(0, srcs, w).permute(0, 2, 3, 1)
    assert float(conv.abs().max()) < 80.0               # |y| >= 10 on the six columns: beyond where float32 tanh + 1 leaves {0, 2}
    image = run_conv_ray(srcs, w, c.c_out, c.N, c.H, c.W, ray_w, bias)
    check_image('(g)', image, conv, bias, ray_w, c)
    only = torch.zeros_like(ray_w)
    only[..., 3 * hi:3 * hi + 3] = ray_w[..., 3 * hi:3 * hi + 3]
    only[..., 3 * lo:3 * lo + 3] = ray_w[..., 3 * lo:3 * lo + 3]
    image = run_conv_ray(srcs, w, c.c_out, c.N, c.H, c.W, only, bias)
    want = (2.0 * ray_w[..., 3 * hi:3 * hi + 3]).permute(0, 3, 1, 2) + 0.0
    assert torch.equal(image.view(torch.int32), want.contiguous().view(torch.int32))


@pytest.mark.parametrize('c', RAY_CASES, ids=ray_id)
def test_ray_epilogue_with_a_tile_mask(c):
    """(h) the mask of a ray launch is laid out for the direct plan's 32 x 8 tiles whatever Winograd flags the descriptor of
    the call carries: built by rnr_conv_active_tiles from the descriptor WITHOUT the flag, passed to a call WITH it.  Dead
    tiles are +0.0, live tiles equal the unmasked launch bitwise.  Where rnr_conv_tile_count reports 0 (grids below 257
    workgroups: plan_conv decides `maskable` before it pins the ray launch to one K slice) the masked call must be refused —
    the two answers agree — and the unmasked call still runs (test_ray_epilogue_gaussian_inputs)."""
    L = _lib.load()
    rng = np.random.default_rng(_seed(c.N, c.H, c.c_out, 8))
    srcs, w = gaussian_case(0, c.N, c.H, c.W, c.cins, c.c_out)
    ray_w = ray_weights(c, rng)
    bias = torch.from_numpy(rng.normal(0.0, 0.5, size=ray_w.shape[-1]).astype(np.float32))
    plain = conv_desc(0, c.cins, c.c_out)
    tiles = L.rnr_conv_tile_count(ctypes.byref(plain), c.N, c.H, c.W)
    ty, tx = c.H // 8, c.W // 32
    if (c.N, c.H, c.W) == (3, 96, 320):
        assert tiles == c.N * ty * tx                   # the one size with >= 257 direct tiles
    if tiles == 0:
        with pytest.raises(_lib.RnrError, match='maskable'):
            run_conv_ray(srcs, w, c.c_out, c.N, c.H, c.W, ray_w, bias, flags=WINO, tile_mask=torch.ones(c.N * ty * tx, dtype=torch.uint8))
        return
    assert tiles == c.N * ty * tx
    live = torch.from_numpy(rng.random((c.N, ty, tx)) < 0.5)
    alpha = (pixels_of(live, 8, 32)[..., 0] & torch.from_numpy(rng.random((c.N, c.H, c.W)) < 0.05)).float()
    buf = conv_active_tiles(plain, alpha, c.N, c.H, c.W, guard=0)
    mask = o64.tile_mask64(alpha, 8, 32)
    assert torch.equal(buf, mask) and 0.2 < float(mask.float().mean()) < 0.8
    full = run_conv_ray(srcs, w, c.c_out, c.N, c.H, c.W, ray_w, bias, flags=WINO)
    assert torch.equal(full, run_conv_ray(srcs, w, c.c_out, c.N, c.H, c.W, ray_w, bias)), 'the Winograd flag is not ignored'
    got = run_conv_ray(srcs, w, c.c_out, c.N, c.H, c.W, ray_w, bias, flags=WINO, tile_mask=buf)
    pix = pixels_of(mask.reshape(c.N, ty, tx), 8, 32)[..., 0][:, None]          # [N,1,H,W]
    want = torch.where(pix, full.view(torch.int32), torch.zeros((), dtype=torch.int32))
    bad = (got.view(torch.int32) != want).nonzero()
    assert bad.shape[0] == 0, ('%d pixels differ, first (n, c, y, x):' % bad.shape[0], bad[:4].tolist())


@pytest.mark.parametrize('what,kind,W,cins,c_out,flags', [
    ('c_out = 64: the 64-column plan', 0, 64, [16], 64, 0),
    ('c_out = 77 is not 3 x rays', 0, 64, [16], 77, 0),
    ('a map 48 pixels wide: the gather kernel', 0, 48, [16], 78, 0),
    ('emulated operands', 0, 64, [16], 78, F16X3),
    ('emulated operands', 0, 64, [16], 78, BF16X6),
    ('4x4 stride 2', 1, 64, [16], 78, 0),
])
def test_ray_epilogue_refusals(what, kind, W, cins, c_out, flags):
    """(i) everything but the exact-fp32 3x3 convolution on the 80-column plan with c_out = 3 x rays is refused (host side)."""
    N, H = 1, 64
    cp = (c_out + 15) // 16 * 16
    srcs = [(torch.zeros(N, C, H, W), None, None, 0) for C in cins]
    k = 3 if kind == 0 else 4
    with pytest.raises(_lib.RnrError, match='80-column'):
        run_conv_ray(srcs, torch.zeros(c_out, sum(cins), k, k), c_out, N, H, W, torch.zeros(N, H, W, cp), torch.zeros(cp),
                     flags=flags, kind=kind)
