"""CPU: the four-phase F(4x4, 2x2) form of the 4x4 stride-2 convolution that conv_wino42s_kernel evaluates
(relightable-nr_amd/csrc/conv_wino42s.inc) in float64, and where the planner takes the kernel (rnr_conv_algorithm 2 with
rnr_conv_winograd_tile 4 under RNR_CONV_WINOGRAD42S; host code only)."""
import ctypes

import numpy as np

from rnr_amd import _lib
from rnr_amd.testing import conv_desc
from test_conv_wino42p_cpu import AT, BT, g_matrix

# N, H, W (input), [C per source], c_out of tests/test_gpu_conv_wino42s.py: exactly 256 workgroups each
GPU_SHAPES = ((64, 32, 64, (16,), 256), (32, 64, 128, (16, 16), 128), (16, 64, 256, (32,), 128), (4, 256, 512, (16,), 64))


def reflect1(i, n):
    i = -i if i < 0 else i
    return 2 * n - 2 - i if i >= n else i


def f42s(x, w):
    """x [H, W], w [4, 4] -> [H / 2, W / 2]: out = sum over the four input parity phases p of the 2x2-tap correlation of the
    phase image D_p[r][c] = x[reflect1(2 r - py)][reflect1(2 c - px)] with the taps g_p[a][b] = w[2 a + 1 - py][2 b + 1 - px],
    each 4 x 4 output tile as A^T [(G g G^T) .* (B^T d B)] A of its 5 x 5 patch of D_p."""
    H, W = x.shape
    Ho, Wo = H // 2, W // 2
    G = g_matrix()
    out = np.zeros((Ho, Wo))
    for py in range(2):
        for px in range(2):
            rows = [reflect1(2 * r - py, H) for r in range(Ho + 1)]
            cols = [reflect1(2 * c - px, W) for c in range(Wo + 1)]
            D = x[np.ix_(rows, cols)]
            g = np.array([[w[2 * a + 1 - py, 2 * b + 1 - px] for b in range(2)] for a in range(2)])
            U = G @ g @ G.T
            for ty in range(Ho // 4):
                for tx in range(Wo // 4):
                    d = D[4 * ty:4 * ty + 5, 4 * tx:4 * tx + 5]
                    out[4 * ty:4 * ty + 4, 4 * tx:4 * tx + 4] += AT @ (U * (BT @ d @ BT.T)) @ AT.T
    return out


def direct(x, w):
    H, W = x.shape
    p = np.pad(x, 1, mode='reflect')
    return np.array([[(p[2 * y:2 * y + 4, 2 * c:2 * c + 4] * w).sum() for c in range(W // 2)] for y in range(H // 2)])


def test_four_phase_form_equals_the_reflected_stride2_convolution():
    rng = np.random.default_rng(421)
    for shape in ((8, 8), (16, 8)):
        for _ in range(20):
            x, w = rng.normal(size=shape), rng.normal(size=(4, 4))
            assert np.abs(f42s(x, w) - direct(x, w)).max() < 1e-12


def test_planner_takes_the_kernel_only_with_its_flag_on_tiling_maps():
    L = _lib.load()
    W, W42, W42S = _lib.CONV_WINOGRAD, _lib.CONV_WINOGRAD | _lib.CONV_WINOGRAD42, _lib.CONV_WINOGRAD | _lib.CONV_WINOGRAD42S
    assert _lib.CONV_WINOGRAD42S == 128
    code = lambda cins, co, fl, n, h, w, kind=1: L.rnr_conv_algorithm(ctypes.byref(conv_desc(kind, cins, co, fl)), n, h, w)
    tile = lambda cins, co, fl, n, h, w, kind=1: L.rnr_conv_winograd_tile(ctypes.byref(conv_desc(kind, cins, co, fl)), n, h, w)
    both = lambda *a, **k: (code(*a, **k), tile(*a, **k))
    # the U-Net's stride-2 layers at 16 views: L3, L5, L7, L9 tile; L11 (16 x 16 output) does not
    for h, cin, co in ((512, 64, 128), (256, 128, 256), (128, 256, 512), (64, 512, 512)):
        assert both((cin,), co, W42S, 16, h, h) == (2, 4)
        assert both((cin,), co, W, 16, h, h) == (2, 2) and both((cin,), co, W42, 16, h, h) == (2, 2)       # without the flag; with the transposed one's
        assert both((cin,), co, 0, 16, h, h) == (0, 0)
    assert both((512,), 512, W42S, 16, 32, 32) == both((512,), 512, W, 16, 32, 32) and tile((512,), 512, W42S, 16, 32, 32) != 4
    assert both((64,), 128, W42S, 1, 512, 512) == (2, 4) and tile((128,), 256, W42S, 1, 256, 256) != 4      # one view per call: L3 only
    for n, h, w, cins, co in GPU_SHAPES:
        assert both(cins, co, W42S, n, h, w) == (2, 4)
        assert both(cins, co, W42S, n - 1, h, w) == both(cins, co, W, n - 1, h, w) and tile(cins, co, W42S, n - 1, h, w) != 4
    n, h, w, cins, co = GPU_SHAPES[0]
    assert both(cins, 64, W42S, 256, h, w, kind=0) == both(cins, 64, W, 256, h, w, kind=0)                  # other kinds ignore it
    assert both(cins, 64, W42S, 256, h // 2, w // 2, kind=2) == both(cins, 64, W, 256, h // 2, w // 2, kind=2)
    assert tile(cins, 64, W42S, 256, h, w, kind=0) != 4 and tile(cins, 64, W42S, 256, h // 2, w // 2, kind=2) != 4
    for pad_co in (48, 80):                                                                                 # columns no multiple of 64
        assert both(cins, pad_co, W42S, 512, h, w) == both(cins, pad_co, W, 512, h, w) and tile(cins, pad_co, W42S, 512, h, w) != 4
    assert both(cins, 64, W42S, 512, 32, 96) == both(cins, 64, W, 512, 32, 96) and tile(cins, 64, W42S, 512, 32, 96) != 4    # Wo = 48
    assert both(cins, 64, W42S, 512, 48, 64) == both(cins, 64, W, 512, 48, 64) and tile(cins, 64, W42S, 512, 48, 64) != 4    # Ho = 24
    assert tile((1024, 16), 64, W42S, 256, 32, 64) != 4 and tile((1008, 16), 64, W42S, 256, 32, 64) == 4    # the BatchNorm table of 1024 channels
    for cins, co in (((16,), 64), ((16, 16), 128), ((512,), 512)):
        steps = sum(cins) // 2
        base = L.rnr_packed_weight_floats(ctypes.byref(conv_desc(1, cins, co, W)))
        assert L.rnr_packed_weight_floats(ctypes.byref(conv_desc(1, cins, co, W42S))) == base + (co // 64) * (4 * steps + 2) * 3200
        assert L.rnr_packed_weight_floats(ctypes.byref(conv_desc(1, cins, co, W42))) == base
    assert L.rnr_packed_weight_floats(ctypes.byref(conv_desc(1, (16,), 48, W42S))) == \
        L.rnr_packed_weight_floats(ctypes.byref(conv_desc(1, (16,), 48, W)))
    n, h, w, cins, co = GPU_SHAPES[1]
    assert L.rnr_conv_workspace_bytes(ctypes.byref(conv_desc(1, cins, co, W42S)), n, h, w) == 256           # never split over K
    assert L.rnr_conv_tile_count(ctypes.byref(conv_desc(1, cins, co, W42S)), n, h, w) == 0                  # takes no tile mask


def test_lowered_grid_threshold_takes_the_kernel_at_small_grids():
    """RNR_WINO42S_MIN_WGS is read once per process, so the lowered threshold is checked in a process of its own (host code only):
    with 1, a single view of one tile takes F(4x4, 2x2); with 2, its one workgroup is too few."""
    import os
    import subprocess
    import sys
    code = ("import ctypes, sys\n"
            "from rnr_amd import _lib\n"
            "from rnr_amd.testing import conv_desc\n"
            "d = conv_desc(1, (16,), 64, _lib.CONV_WINOGRAD | _lib.CONV_WINOGRAD42S)\n"
            "print(_lib.load().rnr_conv_winograd_tile(ctypes.byref(d), 1, 32, 64))\n")
    here = os.path.dirname(os.path.abspath(__file__))
    path = os.pathsep.join([os.path.join(os.path.dirname(here), 'relightable-nr_amd')] + sys.path)
    for min_wgs, want in (('1', 4), ('2', None)):
        env = dict(os.environ, RNR_WINO42S_MIN_WGS=min_wgs, PYTHONPATH=path)
        out = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        got = int(out.stdout.strip().splitlines()[-1])
        assert (got == 4) if want == 4 else (got != 4), (min_wgs, got)
