"""-m gpu: WHERE conv_wino42s_kernel (F(4x4, 2x2), 4x4 stride-2 convolution) touches memory — the guard-band sweep and the NaN
tracer of tests/test_gpu_conv_guard.py on the cases of this kernel, built with oracle/conv_guard_cases.py's case constructor."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import conv_guard_cases as cg
from oracle.conv64 import nan_must
from rnr_amd import _lib
from rnr_amd.testing import conv_desc, pad16, run_conv, run_conv_fused
from test_gpu_conv_guard import SRC_NAMES, assert_intact, bits, check_out, gaussian_inputs, tracer_positions

pytestmark = pytest.mark.gpu
W42S = cg.CONV_WINOGRAD | 128       # RNR_CONV_WINOGRAD42S


def _case(*a, **k):
    c = cg._case(*a, **k)
    c['algo'] = 2               # rnr_conv_algorithm's code of both 2x2-tap Winograd forms; these cases run tile 4
    return c


CASES = [
    _case(1, 64, 32, 64, [16], 256, W42S, 'wino42s', (32, 16, 64), 1, ['one_tile_per_view', 'one_tile_high'], tracer=True),   # 64 x 4 column tiles = 256
    _case(1, 32, 64, 128, [16, 32], 128, W42S, 'wino42s', (32, 16, 64), 1, ['two_sources_unequal'], tracer=True),            # 32 x 4 tiles x 2 = 256
]


def reflect1(i, n):
    i = -i if i < 0 else i
    return 2 * n - 2 - i if i >= n else i


def may1(n, i, p):
    """F(4x4, 2x2), input parity phase p of an axis of n input rows: phase image D_p[r] = pad(in)[2 r - p] = in[reflect1(2 r - p)];
    tile t (outputs 4 t .. 4 t + 3) reads D_p[4 t .. 4 t + 4]: all four outputs of every tile one of whose five rows is input row i."""
    on = n // 2
    assert on % 4 == 0
    o = np.zeros(on, bool)
    for t in range(on // 4):
        if any(reflect1(2 * (4 * t + k) - p, n) == i for k in range(5)):
            o[4 * t:4 * t + 4] = True
    return o


def nan_may5(H, W, i, j):
    m = np.zeros((H // 2, W // 2), bool)
    for py in range(2):
        for px in range(2):
            m |= np.outer(may1(H, i, py), may1(W, j, px))
    return m


def test_may_footprint_holds_the_window():
    for i, j in ((0, 0), (31, 63), (15, 31), (16, 32), (3, 4), (1, 1), (30, 62), (7, 8), (8, 7)):
        assert bool((nan_may5(32, 64, i, j) | ~nan_must(1, 32, 64, i, j)).all())


@pytest.mark.parametrize('c', CASES, ids=[c['id'] for c in CASES])
def test_guard_sweep(c):
    """test_gpu_conv_guard.test_guard_sweep for this kernel: no element outside an operand is written, none of the sentinel-filled
    surroundings (or of the sentinel-prefilled packed weight / out_raw) is read."""
    srcs, w, gamma, beta = gaussian_inputs(c)
    args = (c['kind'], srcs, w, c['c_out'], c['N'], c['H'], c['W'])
    co = c['c_out']
    d = conv_desc(c['kind'], c['cins'], co, c['flags'])
    L = _lib.load()
    assert L.rnr_conv_algorithm(ctypes.byref(d), c['N'], c['H'], c['W']) == 2 and L.rnr_conv_winograd_tile(ctypes.byref(d), c['N'], c['H'], c['W']) == 4
    out_u, st_u = run_conv(*args, flags=c['flags'])
    out_g, st_g, rep = run_conv(*args, flags=c['flags'], guard=True)
    assert_intact('rnr_conv2d', rep, SRC_NAMES(c) + ['weight', 'packed', 'out_raw', 'stats', 'workspace'])
    check_out('rnr_conv2d', out_g, co)
    assert torch.equal(bits(out_g), bits(out_u)), 'rnr_conv2d: guarded and unguarded out_raw differ'
    assert bool(torch.isfinite(st_g).all())
    for k in (0, 1):
        atol = 1e-9 * float(st_u[..., k].abs().max())
        assert torch.allclose(st_g[:, :co, k], st_u[:, :co, k], rtol=1e-6, atol=atol), 'rnr_conv2d: stats differ'
    out_fu, sc_u, sh_u, sy_u = run_conv_fused(*args, gamma, beta, flags=c['flags'], repeats=2)
    out_fg, sc_g, sh_g, sy_g, rep = run_conv_fused(*args, gamma, beta, flags=c['flags'], repeats=2, guard=True)
    assert_intact('rnr_conv2d_fused', rep, SRC_NAMES(c) + ['weight', 'packed', 'out_raw', 'workspace', 'sync', 'scale', 'shift',
                                                            'gamma', 'beta'])
    check_out('rnr_conv2d_fused', out_fg, co)
    assert torch.equal(bits(out_fg), bits(out_fu)) and torch.equal(bits(out_fg), bits(out_u)), 'rnr_conv2d_fused: out_raw differs'
    assert bool(torch.isfinite(sc_g).all()) and bool(torch.isfinite(sh_g).all()), 'scale / shift not finite'
    assert torch.allclose(sc_g[:, :co], sc_u[:, :co], rtol=1e-6, atol=1e-7)
    assert torch.allclose(sh_g[:, :co], sh_u[:, :co], rtol=1e-5, atol=1e-6)
    assert int(sy_g.max()) == 0 and int(sy_u.max()) == 0, 'sync buffer not returned to zero'


@pytest.mark.parametrize('c', CASES, ids=[c['id'] for c in CASES])
def test_nan_tracer(c):
    """One NaN in `raw`: it surfaces in every output whose window holds it and only inside the 4 x 4 tiles whose 5 x 5 patch of
    some phase image holds it; everything else is bitwise the clean run (an index property of staging, reflection and tile decode)."""
    srcs, w, _, _ = gaussian_inputs(c, act=0)
    co = c['c_out']
    clean, _ = run_conv(1, srcs, w, co, c['N'], c['H'], c['W'], flags=c['flags'], with_stats=False)
    assert bool(torch.isfinite(clean).all())
    for n, i, j, s, ch in tracer_positions(c):
        raw = srcs[s][0].clone()
        raw[n, ch, i, j] = float('nan')
        poisoned = list(srcs)
        poisoned[s] = (raw,) + srcs[s][1:]
        out, _ = run_conv(1, poisoned, w, co, c['N'], c['H'], c['W'], flags=c['flags'], with_stats=False)
        tag = 'NaN at view %d pixel (%d, %d) source %d channel %d' % (n, i, j, s, ch)
        must = torch.from_numpy(nan_must(1, c['H'], c['W'], i, j))
        may = torch.from_numpy(nan_may5(c['H'], c['W'], i, j))
        nan = torch.isnan(out[..., :co])
        assert bool(nan[n][must].all()), '%s: outputs whose window holds it are not NaN in every live column' % tag
        reach = torch.zeros(out.shape[:3], dtype=torch.bool)
        reach[n] = may
        stray = nan.any(dim=-1) & ~reach
        assert not bool(stray.any()), '%s: NaN outside the footprint, first at (view, y, x) = %s' % (
            tag, tuple(int(v) for v in stray.nonzero()[0]))
        same = bits(out[..., :co])[~reach] == bits(clean[..., :co])[~reach]
        assert bool(same.all()), '%s: %d outputs outside the footprint differ from the clean run' % (tag, int((~same).sum()))
