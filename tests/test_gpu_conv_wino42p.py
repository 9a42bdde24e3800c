"""-m gpu: conv_wino42p_kernel (Winograd F(4x4, 2x2) for ConvTranspose2d 4x4 s2 p1, RNR_CONV_WINOGRAD42; one output parity class
of 32 x 16 input pixels x 64 columns per 12-wave workgroup) through rnr_conv2d_fused against oracle/conv64.py and oracle/bn64.py.

Shapes: the smallest that reach the kernel.  The planner takes it from 256 workgroups (tiles x column tiles x 4 classes) on, and
its thresholds are read once per process, so a case gets there by its view count (the lowered threshold, RNR_WINO42_MIN_WGS, is
exercised in a process of its own by tests/test_conv_wino42p_cpu.py): one tile per
class and view (every border of the map inside one tile), two tiles in each direction (shared and clamped input rows / columns
at all four borders), 2 views, 16 + 16 and 32 + 16 input channels (one chunk per source; uneven concat), 64 and 128 columns, with
and without the producer's BatchNorm + LeakyReLU.
Bounds: out_raw within 1e-4 of the output peak of the float64 convolution (the bound of the F(4x4, 3x3) sweep); scale /
shift against bn64 on the output the launch wrote, at the bound tests/test_gpu_bn_sweep.py derives (assert_affine)."""
import ctypes

import pytest
import torch

from oracle import bn64
from oracle.conv64 import conv64
from rnr_amd import _lib
from rnr_amd.testing import conv_desc, run_conv, run_conv_fused
from test_gpu_bn_sweep import EPS, assert_affine

pytestmark = pytest.mark.gpu
W2, W42 = _lib.CONV_WINOGRAD, _lib.CONV_WINOGRAD | _lib.CONV_WINOGRAD42

CASES = [
    # N, H, W (input), [C per source], c_out, producer BatchNorm + LeakyReLU on the sources
    (64, 16, 32, [16, 16], 64, True),       # exactly one workgroup tile per class and view
    (16, 32, 64, [32, 16], 64, True),       # two tiles in each direction, uneven concat
    (32, 16, 32, [16, 16], 128, False),     # two column tiles, raw sources
    (2, 64, 128, [16, 16], 128, True),      # 2 views of 4 x 4 tiles
    (8, 32, 64, [32, 16], 128, False),      # two tiles in each direction x two column tiles, uneven concat
]
_cache = {}


def make_inputs(N, H, W, cins, c_out, affine):
    g = torch.Generator().manual_seed(4200 + 7 * N + H + W + c_out + sum(cins))
    srcs = []
    for C in cins:
        raw = torch.randn(N, C, H, W, generator=g)
        if affine:
            srcs.append((raw, torch.rand(N, C, generator=g) + 0.5, torch.randn(N, C, generator=g) * 0.3, 1))
        else:
            srcs.append((raw, None, None, 0))
    cin = sum(cins)
    w = torch.randn(cin, c_out, 4, 4, generator=g) / (cin * 4) ** 0.5
    gamma, beta = torch.rand(c_out, generator=g) + 0.5, torch.randn(c_out, generator=g)
    return srcs, w, gamma, beta


def run_case(case):
    """One fused run (twice on one sync buffer) and the float64 reference per case, shared by the tests below."""
    if case not in _cache:
        N, H, W, cins, c_out, affine = case
        srcs, w, gamma, beta = make_inputs(N, H, W, cins, c_out, affine)
        got = run_conv_fused(2, srcs, w, c_out, N, H, W, gamma, beta, flags=W42, repeats=2)
        ref = conv64(2, srcs, w).permute(0, 2, 3, 1).contiguous()
        _cache[case] = (srcs, w, gamma, beta, got, ref)
    return _cache[case]


IDS = ['%dx%dx%d-%s-%d-%s' % (c[0], c[1], c[2], '+'.join(map(str, c[3])), c[4], 'bn' if c[5] else 'raw') for c in CASES]


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_f4x4_2x2_output_vs_float64(case):
    N, H, W, cins, c_out, _ = case
    L, d = _lib.load(), conv_desc(2, cins, c_out, W42)
    assert L.rnr_conv_algorithm(ctypes.byref(d), N, H, W) == 2 and L.rnr_conv_winograd_tile(ctypes.byref(d), N, H, W) == 4
    _, _, _, _, (out, _, _, sync), ref = run_case(tuple(case[:3]) + (tuple(cins),) + tuple(case[4:]))
    assert tuple(out.shape) == (N, 2 * H, 2 * W, c_out) and bool(torch.isfinite(out).all())
    assert int(sync.to(torch.int32).abs().sum()) == 0, 'sync buffer not returned to zero'
    peak = float(ref.abs().max())
    err = float((out.double() - ref).abs().max())
    rms = float((out.double() - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())
    print('F(4x4, 2x2) %s: max error %.3g of the peak, rms error %.3g of the rms' % (case, err / peak, rms))
    assert err < 1e-4 * peak, (err, peak)


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_f4x4_2x2_batchnorm_vs_bn64(case):
    N, H, W, cins, c_out, _ = case
    _, _, gamma, beta, (out, scale, shift, _), _ = run_case(tuple(case[:3]) + (tuple(cins),) + tuple(case[4:]))
    ref = bn64.per_view(out, c_out, gamma, beta, EPS)
    assert_affine(scale, shift, ref, beta, c_out, 'conv_wino42p_kernel %s' % (case,))


def test_f4x4_2x2_legacy_entry_point_equals_fused():
    """rnr_conv2d (statistics into the caller's buffer, no arrival counters) writes the same out_raw as rnr_conv2d_fused."""
    case = CASES[1]
    N, H, W, cins, c_out, _ = case
    srcs, w, _, _, (out_f, _, _, _), _ = run_case(tuple(case[:3]) + (tuple(cins),) + tuple(case[4:]))
    out, stats = run_conv(2, srcs, w, c_out, N, H, W, flags=W42)
    assert torch.equal(out.view(torch.int32), out_f.view(torch.int32))
    s1 = out.double().sum(dim=(1, 2))
    assert torch.allclose(stats[:, :c_out, 0], s1, rtol=1e-9, atol=1e-9 * float(out.double().abs().sum(dim=(1, 2)).max()))


@pytest.mark.parametrize('N,H,W', [(13, 32, 80), (40, 24, 32)])
def test_map_off_the_tile_runs_the_old_kernel_bit_for_bit(N, H, W):
    """A class map that is no multiple of 32 x 16 reports F(2x2, 2x2) (algorithm 2, Winograd tile 2) and equals the run without the flag bit for bit: scale /
    shift too (the same kernel, the same statistics up to the order of the float64 atomics)."""
    cins, c_out = [32, 16], 64
    L = _lib.load()
    assert L.rnr_conv_algorithm(ctypes.byref(conv_desc(2, cins, c_out, W42)), N, H, W) == 2
    assert L.rnr_conv_winograd_tile(ctypes.byref(conv_desc(2, cins, c_out, W42)), N, H, W) == 2
    assert L.rnr_conv_algorithm(ctypes.byref(conv_desc(2, cins, c_out, W2)), N, H, W) == 2
    srcs, w, gamma, beta = make_inputs(N, H, W, cins, c_out, True)
    a = run_conv_fused(2, srcs, w, c_out, N, H, W, gamma, beta, flags=W42)
    b = run_conv_fused(2, srcs, w, c_out, N, H, W, gamma, beta, flags=W2)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
    assert torch.allclose(a[1], b[1], rtol=1e-6, atol=1e-7) and torch.allclose(a[2], b[2], rtol=1e-5, atol=1e-6)


def test_columns_off_the_tile_keep_the_old_plan():
    """72 live columns: the 80 padded columns are no multiple of 64, so the flag changes nothing about the plan."""
    N, H, W, cins, c_out = 8, 32, 64, [16], 72
    L = _lib.load()
    q = lambda f, fl: f(ctypes.byref(conv_desc(2, cins, c_out, fl)), N, H, W)
    assert q(L.rnr_conv_algorithm, W42) == q(L.rnr_conv_algorithm, W2)
    assert q(L.rnr_conv_winograd_tile, W42) == q(L.rnr_conv_winograd_tile, W2) != 4
