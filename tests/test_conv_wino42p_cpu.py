"""CPU: the F(4x4, 2x2) transform matrices of conv_wino42p_kernel (relightable-nr_amd/csrc/conv_wino42p.inc) in float64, and
where the planner takes the kernel (rnr_conv_algorithm 2 with rnr_conv_winograd_tile 4; host code only)."""
import ctypes

import numpy as np

from rnr_amd import _lib
from rnr_amd.testing import conv_desc

A, B = 0.75, 2.0            # the finite interpolation points are (0, A, -A, B); the fifth is infinity
# the rows the kernel's w42_bt / w42_at evaluate, and pack_weight_wino42p_kernel's G
BT = np.array([[A * A * B, -A * A, -B, 1.0, 0.0],
               [0.0, -A * B, A - B, 1.0, 0.0],
               [0.0, A * B, -(A + B), 1.0, 0.0],
               [0.0, -A * A, 0.0, 1.0, 0.0],
               [0.0, A * A * B, -A * A, -B, 1.0]])
AT = np.array([[1.0, 1.0, 1.0, 1.0, 0.0],
               [0.0, A, -A, B, 0.0],
               [0.0, A * A, A * A, B * B, 0.0],
               [0.0, A ** 3, -A ** 3, B ** 3, 1.0]])


def g_matrix():
    pts = [0.0, A, -A, B]
    G = np.zeros((5, 2))
    for j in range(4):
        den = np.prod([pts[j] - pts[k] for k in range(4) if k != j])
        G[j] = [1.0 / den, pts[j] / den]
    G[4] = [0.0, 1.0]
    return G


def test_transform_matrices_reproduce_a_2x2_tap_correlation():
    """Y = A^T [(G g G^T) .* (B^T d B)] A equals the 4 x 4 outputs of the 2x2-tap correlation of a 5 x 5 patch, and the 1-D form
    the 4 outputs of a 2-tap correlation of 5 values, to 1e-12 on random data."""
    G = g_matrix()
    rng = np.random.default_rng(42)
    for _ in range(200):
        d, g = rng.normal(size=(5, 5)), rng.normal(size=(2, 2))
        y = AT @ ((G @ g @ G.T) * (BT @ d @ BT.T)) @ AT.T
        ref = np.array([[sum(d[i + p, j + q] * g[p, q] for p in range(2) for q in range(2)) for j in range(4)] for i in range(4)])
        assert np.abs(y - ref).max() < 1e-12
        y1 = AT @ ((G @ g[0]) * (BT @ d[0]))
        assert np.abs(y1 - np.array([d[0, i] * g[0, 0] + d[0, i + 1] * g[0, 1] for i in range(4)])).max() < 1e-12


def test_planner_takes_f4x4_2x2_only_with_its_flag_on_tiling_maps():
    """RNR_CONV_WINOGRAD42: transposed layers whose class map tiles into 32 x 16, with 64 k columns, at most 1024 input channels
    and a grid of 256 workgroups (tiles x column tiles x 4 classes) report Winograd tile 4 under algorithm 2 (the code of both
    2x2-tap forms); everything else, and every other flag set, reports what it reported before; the 25-plane image sits behind
    the F(2x2, 2x2) one."""
    L = _lib.load()
    W, W4, W42 = _lib.CONV_WINOGRAD, _lib.CONV_WINOGRAD | _lib.CONV_WINOGRAD4, _lib.CONV_WINOGRAD | _lib.CONV_WINOGRAD42
    code = lambda cins, co, fl, n, h, w, kind=2: L.rnr_conv_algorithm(ctypes.byref(conv_desc(kind, cins, co, fl)), n, h, w)
    tile = lambda cins, co, fl, n, h, w, kind=2: L.rnr_conv_winograd_tile(ctypes.byref(conv_desc(kind, cins, co, fl)), n, h, w)
    # 'f42' stands for "F(4x4, 2x2) runs": algorithm code 2 with Winograd tile 4
    algo = lambda *a, **k: 'f42' if (code(*a, **k), tile(*a, **k)) == (2, 4) else code(*a, **k)
    assert tile((64,), 64, W4, 16, 128, 128, kind=0) == 4 and tile((64,), 64, W, 16, 128, 128, kind=0) == 2 and tile((64,), 64, 0, 16, 128, 128, kind=0) == 0
    assert tile((16, 16), 64, W, 64, 16, 32) == 2 and L.rnr_conv_winograd_tile(None, 1, 16, 16) == -1
    # the U-Net's transposed layers at 16 views: L14, L16, L18, L20 tile, L12 (16 x 16) does not
    for h, cins, co in ((32, (512, 512), 512), (64, (512, 512), 256), (128, (256, 256), 128), (256, (128, 128), 64)):
        assert algo(cins, co, W42, 16, h, h) == 'f42'
        assert algo(cins, co, W, 16, h, h) == 2 and algo(cins, co, W4, 16, h, h) == 2 and algo(cins, co, 0, 16, h, h) == 0
    assert algo((512,), 512, W42, 16, 16, 16) == 2
    # the sizes of tests/test_gpu_conv_wino42p.py: exactly 256 workgroups each
    for n, h, w, cins, co in ((64, 16, 32, (16, 16), 64), (16, 32, 64, (32, 16), 64), (32, 16, 32, (16, 16), 128),
                              (2, 64, 128, (16, 16), 128)):
        assert algo(cins, co, W42, n, h, w) == 'f42'
        assert algo(cins, co, W42, n - 1, h, w) == algo(cins, co, W, n - 1, h, w) != 'f42'       # 252 / 240 / 248 / 128 workgroups: as without the flag
    assert algo((16, 16), 64, W42, 64, 16, 48) == 2                     # width no multiple of 32
    assert algo((16, 16), 64, W42, 64, 24, 32) == 2                     # height no multiple of 16
    assert algo((1024, 16), 64, W42, 64, 16, 32) == 2                   # over the BatchNorm table of 1024 channels
    assert algo((16,), 64, W42, 64, 32, 64, kind=0) == 1 and algo((16,), 128, W42, 4, 256, 256, kind=1) == 2      # other kinds ignore it
    for cins, co in (((16, 16), 64), ((128, 128), 128)):
        steps = sum(cins) // 2
        w2 = L.rnr_packed_weight_floats(ctypes.byref(conv_desc(2, cins, co, W)))
        assert L.rnr_packed_weight_floats(ctypes.byref(conv_desc(2, cins, co, W42))) == w2 + (co // 64) * (steps + 2) * 12800
        assert L.rnr_packed_weight_floats(ctypes.byref(conv_desc(2, cins, co, W4))) == w2
    assert L.rnr_packed_weight_floats(ctypes.byref(conv_desc(2, (16,), 48, W42))) == \
        L.rnr_packed_weight_floats(ctypes.byref(conv_desc(2, (16,), 48, W)))
    assert L.rnr_conv_workspace_bytes(ctypes.byref(conv_desc(2, (16, 16), 64, W42)), 64, 16, 32) == 256        # never split over K
    assert L.rnr_conv_tile_count(ctypes.byref(conv_desc(2, (16, 16), 64, W42)), 64, 16, 32) == 0               # takes no tile mask


def test_lowered_grid_threshold_takes_the_kernel_at_small_grids():
    """RNR_WINO42_MIN_WGS is read once per process, so the lowered threshold is checked in a process of its own (host code only):
    with 1, a single view of one tile per class takes F(4x4, 2x2); with 5, its four workgroups are too few."""
    import os
    import subprocess
    import sys
    code = ("import ctypes, sys\n"
            "from rnr_amd import _lib\n"
            "from rnr_amd.testing import conv_desc\n"
            "d = conv_desc(2, (16, 16), 64, _lib.CONV_WINOGRAD | _lib.CONV_WINOGRAD42)\n"
            "print(_lib.load().rnr_conv_winograd_tile(ctypes.byref(d), 1, 16, 32))\n")
    here = os.path.dirname(os.path.abspath(__file__))
    path = os.pathsep.join([os.path.join(os.path.dirname(here), 'relightable-nr_amd')] + sys.path)
    for min_wgs, want in (('1', 4), ('5', None)):
        env = dict(os.environ, RNR_WINO42_MIN_WGS=min_wgs, PYTHONPATH=path)
        out = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        got = int(out.stdout.strip().splitlines()[-1])
        assert (got == 4) if want == 4 else (got != 4), (min_wgs, got)
