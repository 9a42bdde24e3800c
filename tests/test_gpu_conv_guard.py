"""-m gpu: WHERE the convolution kernels touch memory.  Every kernel of conv.hip / conv_wino*.inc addresses its operands through
descriptors without bounds, so an index slip neither faults nor — next to fresh, zero-padded allocations — changes a value.

  (a) guard sweep   every case of oracle/conv_guard_cases.py (every launcher of CONV_TILES) with every device operand carved out
                    of a sentinel-filled allocation of its own at the weakest alignment the header grants, out_raw / workspace /
                    the packed weight prefilled with the sentinel NaN: guards intact, output finite and BITWISE the unguarded
                    run's, statistics / scale / shift at the bound of test_conv_fused_equals_separate_launches, sync zero.  No
                    float64 reference here: tests/test_gpu_conv_exact_sweep.py compares the values of these cases with a
                    float64 convolution, bit for bit (the F(4x4, .) rows it selects: within a bound; it lists the rest).  For
                    the wino80f4 rows, whose masked launch runs the same kernel, live tiles are bitwise the unmasked launch's.
  (b) NaN tracer    one NaN in `raw`: it must surface in every output whose window contains it and may surface only where
                    rnr_hip.h ("Non-finite inputs") allows for the Winograd tile that runs — a pure index property, the
                    sharpest probe of halo staging, reflection and tile decode; everything outside is bitwise the clean run.
  (c) ReLU and NaN  a NaN under RNR_ACT_RELU surfaces in all five kernel families (rnr_conv_src in rnr_hip.h).
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import conv_guard_cases as cg
from oracle.conv64 import nan_may, nan_must
from rnr_amd import _lib
from rnr_amd.testing import SENTINEL, conv_desc, pad16, run_conv, run_conv_fused, run_conv_ray

pytestmark = pytest.mark.gpu
IDS = [c['id'] for c in cg.CASES]


def bits(t):
    return t.contiguous().view(torch.int32)


def assert_intact(tag, report, want):
    assert set(want) <= set(report), '%s: operands not guarded: %s' % (tag, sorted(set(want) - set(report)))
    for name, off in report.items():
        assert off is None, '%s: guard of operand %s damaged, first byte at payload offset %d' % (tag, name, off)


def gaussian_inputs(c, act=None):
    """As test_conv_vs_torch: scale / shift on the first source, shift only on the second, activations 1 and 2 (act: the same
    activation, scale and shift on every source)."""
    g = torch.Generator().manual_seed(c['kind'] * 100 + c['H'] + c['c_out'] + 7 * c['N'])
    N, H, W = c['N'], c['H'], c['W']
    srcs = []
    for j, C in enumerate(c['cins']):
        raw = torch.randn(N, C, H, W, generator=g)
        sc = torch.rand(N, C, generator=g) + 0.5 if (j == 0 or act is not None) else None
        sh = torch.randn(N, C, generator=g) * 0.3
        srcs.append((raw, sc, sh, act if act is not None else (1 if j == 0 else 2)))
    cin, k = sum(c['cins']), (3 if c['kind'] == 0 else 4)
    shape = (cin, c['c_out'], 4, 4) if c['kind'] == 2 else (c['c_out'], cin, k, k)
    w = torch.randn(shape, generator=g) / (cin * k * k / (4 if c['kind'] == 2 else 1)) ** 0.5
    gamma, beta = torch.rand(c['c_out'], generator=g) + 0.5, torch.randn(c['c_out'], generator=g)
    return srcs, w, gamma, beta


def check_out(tag, out, c_out):
    assert bool(torch.isfinite(out).all()), '%s: out_raw not finite (a sentinel was read, or an element never written)' % tag
    if out.shape[-1] > c_out:
        assert float(out[..., c_out:].abs().max()) == 0.0, '%s: padding columns of out_raw not 0' % tag


SRC_NAMES = lambda c: [n for j in range(len(c['cins'])) for n in ('src%d.data' % j, 'src%d.shift' % j)] + ['src0.scale']


@pytest.mark.parametrize('c', cg.CASES, ids=IDS)
def test_guard_sweep(c):
    srcs, w, gamma, beta = gaussian_inputs(c)
    args = (c['kind'], srcs, w, c['c_out'], c['N'], c['H'], c['W'])
    co, cp = c['c_out'], pad16(c['c_out'])
    L = _lib.load()
    d = cg.desc(c)
    assert L.rnr_conv_algorithm(ctypes.byref(d), c['N'], c['H'], c['W']) == c['algo']
    assert L.rnr_conv_winograd_tile(ctypes.byref(d), c['N'], c['H'], c['W']) == c['m']

    # rnr_conv2d with statistics
    out_u, st_u = run_conv(*args, flags=c['flags'])
    out_g, st_g, rep = run_conv(*args, flags=c['flags'], guard=True)
    assert_intact('rnr_conv2d', rep, SRC_NAMES(c) + ['weight', 'packed', 'out_raw', 'stats', 'workspace'])
    check_out('rnr_conv2d', out_g, co)
    assert torch.equal(bits(out_g), bits(out_u)), 'rnr_conv2d: guarded and unguarded out_raw differ'
    assert bool(torch.isfinite(st_g).all())
    for k in (0, 1):
        atol = 1e-9 * float(st_u[..., k].abs().max())       # float64 atomics of varying order: ~2^-53 of the largest partial per addition
        assert torch.allclose(st_g[:, :co, k], st_u[:, :co, k], rtol=1e-6, atol=atol), 'rnr_conv2d: stats differ'
    if cp > co:
        assert float(st_g[:, co:].abs().max()) == 0.0, 'rnr_conv2d: statistics of the padding columns not 0'

    # rnr_conv2d_fused with BatchNorm, twice on one sync buffer
    out_fu, sc_u, sh_u, sy_u = run_conv_fused(*args, gamma, beta, flags=c['flags'], repeats=2)
    out_fg, sc_g, sh_g, sy_g, rep = run_conv_fused(*args, gamma, beta, flags=c['flags'], repeats=2, guard=True)
    assert_intact('rnr_conv2d_fused', rep, SRC_NAMES(c) + ['weight', 'packed', 'out_raw', 'workspace', 'sync', 'scale', 'shift',
                                                            'gamma', 'beta'])
    check_out('rnr_conv2d_fused', out_fg, co)
    assert torch.equal(bits(out_fg), bits(out_fu)) and torch.equal(bits(out_fg), bits(out_u)), 'rnr_conv2d_fused: out_raw differs'
    assert bool(torch.isfinite(sc_g).all()) and bool(torch.isfinite(sh_g).all()), 'scale / shift not finite'
    assert torch.allclose(sc_g[:, :co], sc_u[:, :co], rtol=1e-6, atol=1e-7)
    assert torch.allclose(sh_g[:, :co], sh_u[:, :co], rtol=1e-5, atol=1e-6)
    if cp > co:
        assert float(sc_g[:, co:].abs().max()) == 0.0 and float(sh_g[:, co:].abs().max()) == 0.0
    assert int(sy_g.max()) == 0 and int(sy_u.max()) == 0, 'sync buffer not returned to zero'

    # rnr_conv2d_masked with a mixed mask, where the masked launch takes one
    tiles = L.rnr_conv_tile_count(ctypes.byref(d), c['N'], c['H'], c['W'])
    rng = np.random.default_rng(c['H'] * 131 + c['W'])
    assert tiles or c['family'] not in ('wino80', 'wino80f4'), 'the out layer\'s Winograd plans take a tile mask'
    if tiles:
        tw, th = cg.mask_tile(c)
        mask = (rng.random(tiles) < 0.5).astype(np.uint8)
        if tiles > 1:
            mask[0], mask[-1] = 1, 0
        mask_t = torch.from_numpy(mask)
        out_mu, _ = run_conv(*args, flags=c['flags'], tile_mask=mask_t)
        out_mg, _, rep = run_conv(*args, flags=c['flags'], tile_mask=mask_t, guard=True)
        assert_intact('rnr_conv2d_masked', rep, SRC_NAMES(c) + ['weight', 'packed', 'out_raw', 'workspace', 'tile_mask'])
        live = torch.from_numpy(mask.astype(bool)).reshape(c['N'], c['H'] // th, 1, c['W'] // tw, 1)
        live = live.expand(-1, -1, th, -1, tw).reshape(c['N'], c['H'], c['W'])
        check_out('rnr_conv2d_masked', out_mg[live], co)
        assert torch.equal(bits(out_mg[live]), bits(out_mu[live])), 'rnr_conv2d_masked: guarded and unguarded differ'
        if c['family'] == 'wino80f4':               # the masked launch runs the same kernel (the other Winograd plans: a direct one)
            assert torch.equal(bits(out_mg[live]), bits(out_u[live])), 'rnr_conv2d_masked: live tiles differ from the unmasked launch'
        assert bool((bits(out_mg[~live]) == SENTINEL).all()), 'rnr_conv2d_masked: a masked-off tile was written'

    # rnr_conv2d_ray on the 80-column direct plan
    if c['family'] == 'halo' and c['tile'] == (32, 8, 80) and c['kind'] == 0 and co % 3 == 0:
        rw = rng.uniform(-1.0, 1.0, size=(c['N'], c['H'], c['W'], cp)).astype(np.float32)
        rw[rng.random((c['N'], c['H'], c['W'])) < 0.3] = 0.0
        rw[..., co:] = 0.0
        rw, bias = torch.from_numpy(rw), torch.from_numpy(rng.normal(0.0, 0.5, size=cp).astype(np.float32))
        for mk in ([None] + ([mask_t] if tiles else [])):
            img_u = run_conv_ray(srcs, w, co, c['N'], c['H'], c['W'], rw, bias, tile_mask=mk)
            img_g, rep = run_conv_ray(srcs, w, co, c['N'], c['H'], c['W'], rw, bias, tile_mask=mk, guard=True)
            assert_intact('rnr_conv2d_ray', rep, SRC_NAMES(c) + ['weight', 'packed', 'ray_w', 'bias', 'image'] +
                          (['tile_mask'] if mk is not None else []))
            assert bool(torch.isfinite(img_g).all()), 'rnr_conv2d_ray: image not finite'
            assert torch.equal(bits(img_g), bits(img_u)), 'rnr_conv2d_ray: guarded and unguarded image differ'


# ---- (b) NaN tracer ----

def tracer_positions(c):
    """(view, row, column, source, channel) of the tracer runs: the four corners, a pixel on each edge, both sides of a tile
    boundary in x and in y, an interior pixel, a pixel of the last view; channel 0, the last live channel, a channel of the
    second source in turn."""
    N, H, W = c['N'], c['H'], c['W']
    up = 2 if c['kind'] == 1 else 1                 # the tiles are counted in the GEMM row space: output pixels for stride 2
    tw, th = c['tile'][0] * up, c['tile'][1] * up
    xb = tw if (c['family'] != 'gather' and W > tw) else W // 2
    yb = th if (c['family'] != 'gather' and H > th) else H // 2
    where = [(0, 0, 0), (0, 0, W - 1), (0, H - 1, 0), (0, H - 1, W - 1),
             (0, 0, W // 2), (0, H - 1, W // 2 - 1), (0, H // 2, 0), (0, H // 2 - 1, W - 1),
             (0, H // 2, xb - 1), (0, H // 2, xb), (0, yb - 1, W // 2), (0, yb, W // 2),
             (0, min(H - 2, H // 2 + 1), max(1, W // 2 - 1)), (N - 1, H // 2, W // 2)]
    last = len(c['cins']) - 1
    chans = [(0, 0), (last, c['cins'][last] - 1), (last, 0)]
    return [(n, i, j) + chans[k % 3] for k, (n, i, j) in enumerate(where)]


TRACER = [c for c in cg.CASES if c['tracer']]


@pytest.mark.parametrize('c', TRACER, ids=[c['id'] for c in TRACER])
def test_nan_tracer(c):
    srcs, w, _, _ = gaussian_inputs(c, act=0)
    assert bool((w != 0).all())
    co = c['c_out']
    clean, _ = run_conv(c['kind'], srcs, w, co, c['N'], c['H'], c['W'], flags=c['flags'], with_stats=False)
    assert bool(torch.isfinite(clean).all())
    for n, i, j, s, ch in tracer_positions(c):
        raw = srcs[s][0].clone()
        raw[n, ch, i, j] = float('nan')
        poisoned = list(srcs)
        poisoned[s] = (raw,) + srcs[s][1:]
        out, _ = run_conv(c['kind'], poisoned, w, co, c['N'], c['H'], c['W'], flags=c['flags'], with_stats=False)
        tag = 'NaN at view %d pixel (%d, %d) source %d channel %d' % (n, i, j, s, ch)
        must = torch.from_numpy(nan_must(c['kind'], c['H'], c['W'], i, j))
        may = torch.from_numpy(nan_may(c['kind'], c['m'], c['H'], c['W'], i, j))
        assert bool((may | ~must).all())
        nan = torch.isnan(out[..., :co])
        assert bool(nan[n][must].all()), '%s: %d of %d outputs whose window holds it are not NaN in every live column' % (
            tag, int((~nan[n][must].all(dim=-1)).sum()), int(must.sum()))
        reach = torch.zeros(out.shape[:3], dtype=torch.bool)
        reach[n] = may
        stray = nan.any(dim=-1) & ~reach
        assert not bool(stray.any()), '%s: NaN outside the footprint, first at (view, y, x) = %s' % (
            tag, tuple(int(v) for v in stray.nonzero()[0]))
        same = bits(out[..., :co])[~reach] == bits(clean[..., :co])[~reach]
        assert bool(same.all()), '%s: %d outputs outside the footprint differ from the clean run' % (tag, int((~same).sum()))


# ---- (c) ReLU and NaN ----

def test_relu_propagates_nan_in_every_kernel_family():
    """max(v, 0 * v): both operands are NaN, so the NaN survives whatever v_max_f32 does with ONE NaN operand — in the direct,
    F(2x2, 3x3), F(4x4, 3x3) and both emulated kernels alike (UNetPlan's check_finite = 'first' relies on it)."""
    kind, N, H, W, cins, co = cg.RELU_NAN_SHAPE
    c = dict(kind=kind, N=N, H=H, W=W, cins=cins, c_out=co)
    srcs, w, _, _ = gaussian_inputs(c, act=2)
    n, i, j, ch = 1, 31, 32, 5
    raw = srcs[0][0].clone()
    raw[n, ch, i, j] = float('nan')
    srcs = [(raw,) + srcs[0][1:]]
    must = torch.from_numpy(nan_must(kind, H, W, i, j))
    verdict = {}
    L = _lib.load()
    for flags, algo, m in cg.RELU_NAN_FLAGS:
        d = conv_desc(kind, cins, co, flags)
        assert L.rnr_conv_algorithm(ctypes.byref(d), N, H, W) == algo and L.rnr_conv_winograd_tile(ctypes.byref(d), N, H, W) == m
        out, _ = run_conv(kind, srcs, w, co, N, H, W, flags=flags, with_stats=False)
        nan = torch.isnan(out[n][must][:, :co])
        verdict[flags] = 'all' if bool(nan.all()) else ('none' if not bool(nan.any()) else 'some')
        may = torch.from_numpy(nan_may(kind, m, H, W, i, j))
        assert not bool(torch.isnan(out[n][~may]).any()) and not bool(torch.isnan(out[:n]).any())
    assert set(verdict.values()) == {'all'}, 'flags -> NaN at the window outputs: %s' % verdict
