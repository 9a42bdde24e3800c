"""-m gpu: conv_wino42s_kernel (Winograd F(4x4, 2x2) for ReflectionPad2d(1) + Conv2d 4x4 s2, RNR_CONV_WINOGRAD42S; 32 x 16 output
pixels x 64 columns per 12-wave workgroup) through rnr_conv2d_fused against oracle/conv64.py and oracle/bn64.py.

Shapes: the smallest that reach the kernel at the default threshold of 256 workgroups (the lowered threshold is exercised in a
process of its own by tests/test_conv_wino42s_cpu.py).
Bounds: out_raw within 1e-4 of the output peak of the float64 convolution; scale / shift against bn64 on the
output the launch wrote, at the bound tests/test_gpu_bn_sweep.py derives (assert_affine).

Measured (MI355X), max error of the peak / rms error of the rms: see profiles/r09_wino42s_ab.txt."""
import ctypes

import pytest
import torch

from oracle import bn64
from oracle.conv64 import conv64
from rnr_amd import _lib
from rnr_amd.testing import conv_desc, run_conv, run_conv_fused
from test_gpu_bn_sweep import EPS, assert_affine

pytestmark = pytest.mark.gpu
W2, W42S = _lib.CONV_WINOGRAD, _lib.CONV_WINOGRAD | _lib.CONV_WINOGRAD42S

CASES = [
    # N, H, W (input), (C per source), c_out, producer BatchNorm + LeakyReLU on the sources
    (64, 32, 64, (16,), 256, True),         # one tile per view: all four reflected borders in one tile; four column tiles
    (32, 64, 128, (16, 16), 128, True),     # two tiles each way, two sources
    (16, 64, 256, (32,), 128, False),       # two chunks per phase, raw source
    (4, 256, 512, (16,), 64, True),         # interior tiles, 8 x 8 per view
]
_cache = {}


def make_inputs(N, H, W, cins, c_out, affine):
    g = torch.Generator().manual_seed(4210 + 7 * N + H + W + c_out + sum(cins))
    srcs = []
    for C in cins:
        raw = torch.randn(N, C, H, W, generator=g)
        if affine:
            srcs.append((raw, torch.rand(N, C, generator=g) + 0.5, torch.randn(N, C, generator=g) * 0.3, 1))
        else:
            srcs.append((raw, None, None, 0))
    cin = sum(cins)
    w = torch.randn(c_out, cin, 4, 4, generator=g) / (cin * 16) ** 0.5
    gamma, beta = torch.rand(c_out, generator=g) + 0.5, torch.randn(c_out, generator=g)
    return srcs, w, gamma, beta


def run_case(case):
    """One fused run (twice on one sync buffer) and the float64 reference per case, shared by the tests below."""
    if case not in _cache:
        N, H, W, cins, c_out, affine = case
        srcs, w, gamma, beta = make_inputs(N, H, W, cins, c_out, affine)
        got = run_conv_fused(1, srcs, w, c_out, N, H, W, gamma, beta, flags=W42S, repeats=2)
        ref = conv64(1, srcs, w).permute(0, 2, 3, 1).contiguous()
        _cache[case] = (srcs, w, gamma, beta, got, ref)
    return _cache[case]


IDS = ['%dx%dx%d-%s-%d-%s' % (c[0], c[1], c[2], '+'.join(map(str, c[3])), c[4], 'bn' if c[5] else 'raw') for c in CASES]


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_f4x4_2x2_stride2_output_vs_float64(case):
    N, H, W, cins, c_out, _ = case
    L, d = _lib.load(), conv_desc(1, cins, c_out, W42S)
    assert L.rnr_conv_algorithm(ctypes.byref(d), N, H, W) == 2 and L.rnr_conv_winograd_tile(ctypes.byref(d), N, H, W) == 4
    _, _, _, _, (out, _, _, sync), ref = run_case(case)
    assert tuple(out.shape) == (N, H // 2, W // 2, c_out) and bool(torch.isfinite(out).all())
    assert int(sync.to(torch.int32).abs().sum()) == 0, 'sync buffer not returned to zero'
    peak = float(ref.abs().max())
    err = float((out.double() - ref).abs().max())
    rms = float((out.double() - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())
    print('F(4x4, 2x2) stride 2 %s: max error %.3g of the peak, rms error %.3g of the rms' % (case, err / peak, rms))
    assert err < 1e-4 * peak, (err, peak)


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_f4x4_2x2_stride2_batchnorm_vs_bn64(case):
    c_out = case[4]
    _, _, gamma, beta, (out, scale, shift, _), _ = run_case(case)
    ref = bn64.per_view(out, c_out, gamma, beta, EPS)
    assert_affine(scale, shift, ref, beta, c_out, 'conv_wino42s_kernel %s' % (case,))


def test_f4x4_2x2_stride2_legacy_entry_point_equals_fused():
    """rnr_conv2d (statistics into the caller's buffer, no arrival counters) writes the same out_raw as rnr_conv2d_fused."""
    case = CASES[1]
    N, H, W, cins, c_out, _ = case
    srcs, w, _, _, (out_f, _, _, _), _ = run_case(case)
    out, stats = run_conv(1, srcs, w, c_out, N, H, W, flags=W42S)
    assert torch.equal(out.view(torch.int32), out_f.view(torch.int32))
    s1 = out.double().sum(dim=(1, 2))
    assert torch.allclose(stats[:, :c_out, 0], s1, rtol=1e-9, atol=1e-9 * float(out.double().abs().sum(dim=(1, 2)).max()))


@pytest.mark.parametrize('N,H,W,tile', [(50, 32, 96, 2), (40, 48, 64, 0)])
def test_map_off_the_tile_runs_the_old_kernel_bit_for_bit(N, H, W, tile):
    """An output map that is no multiple of 32 x 16 reports what the descriptor without the flag reports and equals that run bit
    for bit, scale / shift too (the same kernel, the same statistics up to the order of the float64 atomics).  Wo = 48 tiles into
    the 16 x 16 pixels of F(2x2, 2x2): algorithm 2, Winograd tile 2.  Ho = 24 does not — no height that 16 does not divide can,
    the old kernel's tile being 16 rows high as well — so that map runs the direct kernels (algorithm 0, tile 0) with or without
    the flag."""
    cins, c_out = (16,), 512
    L = _lib.load()
    q = lambda f, fl: f(ctypes.byref(conv_desc(1, cins, c_out, fl)), N, H, W)
    assert q(L.rnr_conv_winograd_tile, W42S) == q(L.rnr_conv_winograd_tile, W2) == tile
    assert q(L.rnr_conv_algorithm, W42S) == q(L.rnr_conv_algorithm, W2) == tile
    srcs, w, gamma, beta = make_inputs(N, H, W, cins, c_out, True)
    a = run_conv_fused(1, srcs, w, c_out, N, H, W, gamma, beta, flags=W42S)
    b = run_conv_fused(1, srcs, w, c_out, N, H, W, gamma, beta, flags=W2)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
    assert torch.allclose(a[1], b[1], rtol=1e-6, atol=1e-7) and torch.allclose(a[2], b[2], rtol=1e-5, atol=1e-6)
