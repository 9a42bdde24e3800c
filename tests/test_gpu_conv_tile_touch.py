"""-m gpu: the next-tile touch of the one-workgroup-per-CU Winograd kernels conv_wino42p_kernel, conv_wino42s_kernel and
conv_wino80f4_kernel (W42_PREFETCH / W8F_PREFETCH, csrc/conv_wino42_body.inc, csrc/conv_wino80f4.inc): behind its K loop workgroup
b touches the first staged image of block b + 256's tile.  Every other conv test launches exactly 256 workgroups, where no block
has a successor; the launches here have more, through rnr_amd.testing.run_conv_fused.

Touch changes nothing: one launch of 2N views (512 workgroups: blocks 0 - 255 touch, their successors cover every tile position
of a view, first and last tile rows and columns included) against two launches of N views (256 workgroups each, nobody touches):
out_raw bitwise equal view for view; scale / shift of the big launch against oracle/bn64.py on the output it wrote, at the bound
tests/test_gpu_bn_sweep.py derives.  The stride-2 case has a 16-channel source, so the second touched dword clamps to the
pixel's last; the transposed and the out-layer case have two sources, of which the touch reads source 0.
Ragged successor: a launch of more than 256, fewer than 512 workgroups whose count is no multiple of 8, so only some blocks have a
successor and block_coords' remainder branch decodes it; out_raw within 1e-4 of the peak of oracle/conv64.py, sync
buffer back to zero.

A kernel whose touch is compiled out (its macro at 0) passes the same tests; what they pin is that a build with the touch on
computes what one without computes."""
import ctypes

import pytest
import torch

from oracle import bn64
from oracle.conv64 import conv64
from rnr_amd import _lib
from rnr_amd.testing import conv_desc, run_conv_fused
from test_gpu_bn_sweep import EPS, assert_affine

pytestmark = pytest.mark.gpu
WINO = _lib.CONV_WINOGRAD
FLAGS = {'s2': WINO | _lib.CONV_WINOGRAD42S, 'tr': WINO | _lib.CONV_WINOGRAD42, 'out': WINO | _lib.CONV_WINOGRAD4 | _lib.CONV_WINOGRAD4_OUT}
KIND = {'s2': 1, 'tr': 2, 'out': 0}
ALGO = {'s2': 2, 'tr': 2, 'out': 3}         # rnr_conv_algorithm's code of the kernel under test; all three run Winograd tile 4

# name: N (the big launch), H, W (input), C per source, c_out, workgroups of the big launch
BIG = {
    's2': (8, 256, 512, (16,), 64, 512),            # 64 tiles of 32 x 16 outputs per view
    'tr': (32, 32, 64, (16, 16), 64, 512),          # 4 tiles x 4 parity classes per view
    'out': (2, 256, 256, (16, 16), 78, 512),        # 256 tiles of 16 x 16 per view
}
RAGGED = {
    's2': (29, 96, 192, (16,), 64, 261),            # 9 tiles per view
    'tr': (23, 48, 32, (16, 16), 64, 276),          # 3 tile rows x 4 classes per view
    'out': (29, 48, 48, (16, 16), 78, 261),         # 9 tiles per view
}
_cache = {}


def make_inputs(name, N, H, W, cins, c_out):
    g = torch.Generator().manual_seed(1010 + 7 * N + H + W + c_out + sum(cins) + KIND[name])
    srcs = []
    for j, C in enumerate(cins):
        raw = torch.randn(N, C, H, W, generator=g)
        srcs.append((raw, torch.rand(N, C, generator=g) + 0.5, torch.randn(N, C, generator=g) * 0.3, 1 if j == 0 else 2))
    cin = sum(cins)
    k = 3 if name == 'out' else 4
    shape = (cin, c_out, 4, 4) if name == 'tr' else (c_out, cin, k, k)
    w = torch.randn(shape, generator=g) / (cin * (4 if name == 'tr' else k * k)) ** 0.5
    gamma, beta = torch.rand(c_out, generator=g) + 0.5, torch.randn(c_out, generator=g)
    return srcs, w, gamma, beta


def assert_kernel(name, N, H, W, cins, c_out, wgs):
    """The planner gives the launch to the kernel under test, with `wgs` workgroups of one tile each."""
    L, d = _lib.load(), conv_desc(KIND[name], cins, c_out, FLAGS[name])
    assert L.rnr_conv_algorithm(ctypes.byref(d), N, H, W) == ALGO[name]
    assert L.rnr_conv_winograd_tile(ctypes.byref(d), N, H, W) == 4
    Ho, Wo = (H // 2, W // 2) if name == 's2' else (H, W)
    tiles = N * (Ho // 16) * (Wo // 16) if name == 'out' else N * (Ho // 16) * (Wo // 32) * (4 if name == 'tr' else 1)
    assert tiles * ((c_out + 63) // 64 if name != 'out' else 1) == wgs


def views(srcs, lo, hi):
    return [(raw[lo:hi], sc[lo:hi], sh[lo:hi], act) for raw, sc, sh, act in srcs]


def big_launch(name):
    """The 512-workgroup launch of a kernel, once: inputs and what it wrote."""
    if name not in _cache:
        N, H, W, cins, c_out, _ = BIG[name]
        srcs, w, gamma, beta = make_inputs(name, N, H, W, cins, c_out)
        _cache[name] = (srcs, w, gamma, beta, run_conv_fused(KIND[name], srcs, w, c_out, N, H, W, gamma, beta, flags=FLAGS[name]))
    return _cache[name]


@pytest.mark.parametrize('name', ['s2', 'tr', 'out'])
def test_touching_launch_equals_two_launches_that_do_not_touch(name):
    N, H, W, cins, c_out, wgs = BIG[name]
    assert_kernel(name, N, H, W, cins, c_out, wgs)
    assert_kernel(name, N // 2, H, W, cins, c_out, 256)
    srcs, w, gamma, beta, (out, _, _, sync) = big_launch(name)
    assert bool(torch.isfinite(out).all()) and int(sync.to(torch.int32).abs().sum()) == 0
    for half in range(2):
        lo, hi = half * (N // 2), (half + 1) * (N // 2)
        part, _, _, psync = run_conv_fused(KIND[name], views(srcs, lo, hi), w, c_out, N // 2, H, W, gamma, beta, flags=FLAGS[name])
        assert int(psync.to(torch.int32).abs().sum()) == 0
        same = (out[lo:hi].view(torch.int32) == part.view(torch.int32)).flatten(1).all(dim=1)
        assert bool(same.all()), 'views %s of the 512-workgroup launch differ from the 256-workgroup launch' % (
            [lo + i for i in range(N // 2) if not bool(same[i])],)


@pytest.mark.parametrize('name', ['s2', 'tr', 'out'])
def test_touching_launch_batchnorm_vs_bn64(name):
    c_out = BIG[name][4]
    _, _, gamma, beta, (out, scale, shift, _) = big_launch(name)
    ref = bn64.per_view(out, c_out, gamma, beta, EPS)
    assert_affine(scale, shift, ref, beta, c_out, 'tile touch, %s %s' % (name, BIG[name]))


@pytest.mark.parametrize('name', ['s2', 'tr', 'out'])
def test_ragged_grid_some_blocks_have_a_successor(name):
    N, H, W, cins, c_out, wgs = RAGGED[name]
    assert 256 < wgs < 512 and wgs % 8 != 0
    assert_kernel(name, N, H, W, cins, c_out, wgs)
    srcs, w, gamma, beta = make_inputs(name, N, H, W, cins, c_out)
    out, _, _, sync = run_conv_fused(KIND[name], srcs, w, c_out, N, H, W, gamma, beta, flags=FLAGS[name], repeats=2)
    ref = conv64(KIND[name], srcs, w).permute(0, 2, 3, 1).contiguous()
    assert int(sync.to(torch.int32).abs().sum()) == 0, 'sync buffer not returned to zero'
    peak = float(ref.abs().max())
    err = float((out[..., :c_out].double() - ref).abs().max())
    print('tile touch, ragged %s %s: max error %.3g of the peak' % (name, RAGGED[name], err / peak))
    assert bool(torch.isfinite(out).all()) and err < 1e-4 * peak, (err, peak)
