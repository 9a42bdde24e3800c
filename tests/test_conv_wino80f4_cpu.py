"""CPU: where the planner takes conv_wino80f4_kernel (relightable-nr_amd/csrc/conv_wino80f4.inc: F(4x4, 3x3) for the 80-column
out layer, RNR_CONV_WINOGRAD4_OUT) — rnr_conv_algorithm 3 with rnr_conv_winograd_tile 4 — and what its packed image adds (host
code only)."""
import ctypes
import os
import subprocess
import sys

from rnr_amd import _lib
from rnr_amd.testing import conv_desc

W = _lib.CONV_WINOGRAD
W4 = W | _lib.CONV_WINOGRAD4                      # what callers passed before the flag existed
OUT = W4 | _lib.CONV_WINOGRAD4_OUT
STEP_FLOATS = 36 * 4 * 80                         # one K step of the image: 36 planes x 4 input channels x 80 columns
LOOKAHEAD = 1                                     # zero K steps behind the last one (W8F_BDIST)


def _plan(cins, c_out, flags, n, h, w):
    L, d = _lib.load(), conv_desc(0, cins, c_out, flags)
    return L.rnr_conv_algorithm(ctypes.byref(d), n, h, w), L.rnr_conv_winograd_tile(ctypes.byref(d), n, h, w)


def test_planner_takes_the_kernel_only_with_its_flag_on_tiling_maps_that_fill_the_chip():
    L = _lib.load()
    assert _lib.CONV_WINOGRAD4_OUT == 64
    # with the flag: 256 tiles of 16 x 16 each
    for n, h, w, cins in ((4, 128, 128, (64, 64)), (16, 64, 64, (112,))):
        assert _plan(cins, 78, OUT, n, h, w) == (3, 4)
        assert _plan(cins, 78, W | _lib.CONV_WINOGRAD4_OUT, n, h, w) == (3, 4)      # RNR_CONV_WINOGRAD4 is not needed
        # without it: the out layer's F(2x2, 3x3) kernel, as before
        assert _plan(cins, 78, W4, n, h, w) == (3, 2) and _plan(cins, 78, W, n, h, w) == (3, 2)
        assert _plan(cins, 78, 0, n, h, w) == (0, 0)
        d = conv_desc(0, cins, 78, OUT)
        assert L.rnr_conv_tile_count(ctypes.byref(d), n, h, w) == n * (h // 16) * (w // 16)
        assert L.rnr_conv_tile_count(ctypes.byref(conv_desc(0, cins, 78, W4)), n, h, w) == n * (h // 4) * (w // 16)
        assert L.rnr_conv_workspace_bytes(ctypes.byref(d), n, h, w) == 256          # never split over K
    # the benchmark's out layer, 16 views and one view of 512^2
    assert _plan((64, 64), 78, OUT, 16, 512, 512) == (3, 4) and _plan((64, 64), 78, OUT, 1, 512, 512) == (3, 4)
    # a grid below the minimum (128 tiles), and a map 16 does not divide in height but 4 does: F(2x2, 3x3)
    assert _plan((64, 64), 78, OUT, 2, 128, 128) == (3, 2)
    assert _plan((64, 64), 78, OUT, 16, 68, 64) == (3, 2) and _plan((112,), 78, OUT, 16, 68, 64) == (3, 2)
    assert L.rnr_conv_tile_count(ctypes.byref(conv_desc(0, (64, 64), 78, OUT)), 16, 68, 64) == 16 * 17 * 4
    # where conv_wino80_kernel does not qualify either (32 tiles of 16 x 4): direct
    assert _plan((64,), 78, OUT, 1, 32, 64) == (0, 0)
    # more input channels than the BatchNorm table holds: F(2x2, 3x3)
    assert _plan((1024, 16), 78, OUT, 4, 128, 128) == (3, 2)
    # other column counts and kinds ignore the flag
    assert _plan((64,), 64, OUT, 16, 128, 128) == (4, 4) and _plan((64,), 64, W | _lib.CONV_WINOGRAD4_OUT, 16, 128, 128) == (1, 2)
    d1 = conv_desc(1, (64,), 78, W | _lib.CONV_WINOGRAD4_OUT)
    assert L.rnr_conv_algorithm(ctypes.byref(d1), 16, 128, 128) == L.rnr_conv_algorithm(ctypes.byref(conv_desc(1, (64,), 78, W)), 16, 128, 128)


def test_packed_weight_grows_by_the_36_plane_image_behind_the_fallback_images():
    """The F(4x4, 3x3) image of the out layer sits behind the direct and the F(2x2, 3x3) images, which keep their sizes and
    places (the packed buffer serves the fall-back kernels); every image starts on a multiple of 4 floats (dwordx4 loads)."""
    L = _lib.load()
    size = lambda cins, co, fl, kind=0: L.rnr_packed_weight_floats(ctypes.byref(conv_desc(kind, cins, co, fl)))
    for cins in ((64, 64), (112,), (16,), (20,)):
        cin_pad = sum((c + 15) // 16 * 16 for c in cins)
        direct, fallback = size(cins, 78, 0), size(cins, 78, W)
        assert size(cins, 78, W4) == fallback                       # 80 columns never had an RNR_CONV_WINOGRAD4 image
        grown = size(cins, 78, OUT)
        assert grown == fallback + (cin_pad // 4 + LOOKAHEAD) * STEP_FLOATS
        assert grown == size(cins, 78, W | _lib.CONV_WINOGRAD4_OUT)
        assert direct % 4 == 0 and fallback % 4 == 0 and grown % 4 == 0
    # 64 columns, other kinds: nothing added
    assert size((64,), 64, OUT) == size((64,), 64, W4)
    assert size((64,), 78, W | _lib.CONV_WINOGRAD4_OUT, kind=2) == size((64,), 78, W, kind=2)


def test_lowered_grid_threshold_takes_the_kernel_at_small_grids():
    """RNR_WINO80F4_MIN_WGS is read once per process, so the lowered threshold is checked in a process of its own (host code
    only): with 1, one view of one tile takes F(4x4, 3x3); with 5, four tiles are too few."""
    code = ("import ctypes, sys\n"
            "from rnr_amd import _lib\n"
            "from rnr_amd.testing import conv_desc\n"
            "d = conv_desc(0, (16,), 78, _lib.CONV_WINOGRAD | _lib.CONV_WINOGRAD4_OUT)\n"
            "L = _lib.load()\n"
            "print(L.rnr_conv_winograd_tile(ctypes.byref(d), 1, 32, 32), L.rnr_conv_tile_count(ctypes.byref(d), 1, 32, 32))\n")
    here = os.path.dirname(os.path.abspath(__file__))
    path = os.pathsep.join([os.path.join(os.path.dirname(here), 'relightable-nr_amd')] + sys.path)
    for min_wgs, want in (('1', (4, 4)), ('5', None)):
        env = dict(os.environ, RNR_WINO80F4_MIN_WGS=min_wgs, RNR_WINO_MIN_WGS='1', PYTHONPATH=path)
        out = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        got = tuple(int(v) for v in out.stdout.strip().splitlines()[-1].split())
        if want:
            assert got == want, (min_wgs, got)
        else:
            assert got == (2, 16), (min_wgs, got)       # conv_wino80_kernel's 16 x 4 tiles
