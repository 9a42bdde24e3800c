"""-m gpu: conv_wino80f4_kernel (Winograd F(4x4, 3x3) for the 80-column out layer, RNR_CONV_WINOGRAD4_OUT; 16 x 16 output pixels x
80 columns per 12-wave workgroup) through rnr_conv2d_fused / rnr_conv2d_masked against oracle/conv64.py.

Shapes: the smallest that reach the kernel — the planner takes it from 256 workgroups on and reads its thresholds once per
process, so every case has exactly 256 tiles of 16 x 16 (the lowered threshold is exercised in a process of its own by
tests/test_conv_wino80f4_cpu.py).
Bounds: out_raw within 1e-4 of the output peak of the float64 convolution (the project's gate for every Winograd kernel); scale /
shift of the same launch against the float64 statistics at the tolerances of test_gpu_unet.test_conv_winograd_f4x4_vs_torch.
Where the kernel touches memory: the wino80f4 rows of oracle/conv_guard_cases.py, run by tests/test_gpu_conv_guard.py."""
import ctypes

import numpy as np
import pytest
import torch

from oracle.conv64 import conv64
from rnr_amd import _lib
from rnr_amd.testing import SENTINEL, conv_active_tiles, conv_desc, run_conv, run_conv_fused
from test_gpu_conv_guard import bits

pytestmark = pytest.mark.gpu
W4 = _lib.CONV_WINOGRAD | _lib.CONV_WINOGRAD4             # conv_wino80_kernel (F(2x2, 3x3)) on 80 columns
OUT = W4 | _lib.CONV_WINOGRAD4_OUT

CASES = [
    # N, H, W, [C per source], c_out
    (256, 16, 16, (16, 16), 78),        # one tile per view: every halo pixel reflected on all four borders
    (4, 128, 128, (64, 64), 78),        # skip concat, two sources with their own scale / shift / activation
    (16, 64, 64, (108,), 78),           # 7 chunks, 4 padding input channels
    (32, 32, 64, (32, 96), 78),         # non-square, unequal sources
    (16, 64, 64, (64,), 72),            # 72 live columns: columns 72 ... 79 stay exactly zero
]
IDS = ['%dx%dx%d-%s-%d' % (c[0], c[1], c[2], '+'.join(map(str, c[3])), c[4]) for c in CASES]
_cache = {}


def make_inputs(N, H, W, cins, c_out):
    g = torch.Generator().manual_seed(8000 + 7 * N + H + W + c_out + sum(cins))
    srcs = []
    for j, C in enumerate(cins):
        raw = torch.randn(N, C, H, W, generator=g)
        srcs.append((raw, torch.rand(N, C, generator=g) + 0.5, torch.randn(N, C, generator=g) * 0.3, 1 if j == 0 else 2))
    cin = sum(cins)
    w = torch.randn(c_out, cin, 3, 3, generator=g) / (cin * 9) ** 0.5
    gamma, beta = torch.rand(c_out, generator=g) + 0.5, torch.randn(c_out, generator=g)
    return srcs, w, gamma, beta


def run_case(case):
    """Per case, once: the fused launch alone and twice on one sync buffer, and the float64 reference."""
    if case not in _cache:
        N, H, W, cins, c_out = case
        srcs, w, gamma, beta = make_inputs(*case)
        first = run_conv_fused(0, srcs, w, c_out, N, H, W, gamma, beta, flags=OUT)
        second = run_conv_fused(0, srcs, w, c_out, N, H, W, gamma, beta, flags=OUT, repeats=2)
        ref = conv64(0, srcs, w).permute(0, 2, 3, 1).contiguous()
        _cache[case] = (srcs, w, gamma, beta, first, second, ref)
    return _cache[case]


def errors(out, ref, c_out):
    d = out[..., :c_out].double() - ref
    return float(d.abs().max() / ref.abs().max()), float(d.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_f4x4_out_layer_output_vs_float64(case):
    N, H, W, cins, c_out = case
    L, d = _lib.load(), conv_desc(0, cins, c_out, OUT)
    assert L.rnr_conv_algorithm(ctypes.byref(d), N, H, W) == 3 and L.rnr_conv_winograd_tile(ctypes.byref(d), N, H, W) == 4
    assert L.rnr_conv_tile_count(ctypes.byref(d), N, H, W) == 256
    srcs, w, gamma, beta, first, (out, _, _, sync), ref = run_case(case)
    assert tuple(out.shape) == (N, H, W, 80) and bool(torch.isfinite(out).all())
    assert float(out[..., c_out:].abs().max()) == 0.0, 'padding columns not exactly zero'
    assert int(sync.to(torch.int32).abs().sum()) == 0 and int(first[3].to(torch.int32).abs().sum()) == 0, 'sync buffer not returned to zero'
    e_max, e_rms = errors(out, ref, c_out)
    # conv_wino80_kernel (F(2x2, 3x3)) on the same inputs, for the record
    old = run_conv_fused(0, srcs, w, c_out, N, H, W, gamma, beta, flags=W4)[0]
    o_max, o_rms = errors(old, ref, c_out)
    print('\nconv_wino80f4_kernel %s: max error %.3g of the peak, rms error %.3g of the rms   (conv_wino80_kernel: %.3g, %.3g)' % (
        case, e_max, e_rms, o_max, o_rms))
    assert e_max < 1e-4, e_max


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_f4x4_out_layer_batchnorm_vs_float64_statistics(case):
    N, H, W, cins, c_out = case
    _, _, gamma, beta, _, (_, scale, shift, _), ref = run_case(case)
    mean, var = ref.mean(dim=(1, 2)), ref.var(dim=(1, 2), unbiased=False)
    sc_ref = gamma.double()[None] / torch.sqrt(var + 1e-5)
    sh_ref = beta.double()[None] - mean * sc_ref
    assert torch.allclose(scale[:, :c_out].double(), sc_ref, rtol=5e-5, atol=1e-6)
    assert torch.allclose(shift[:, :c_out].double(), sh_ref, rtol=5e-5, atol=5e-5)
    assert float(scale[:, c_out:].abs().max()) == 0.0 and float(shift[:, c_out:].abs().max()) == 0.0


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_f4x4_out_layer_second_launch_is_bit_identical(case):
    _, _, _, _, first, second, _ = run_case(case)
    assert torch.equal(bits(first[0]), bits(second[0])), 'out_raw of the second launch differs from the first'
    assert torch.equal(bits(first[1]), bits(second[1])) and torch.equal(bits(first[2]), bits(second[2])), 'scale / shift differ'


def test_flag_without_its_companion_is_refused():
    srcs, w, gamma, beta = make_inputs(1, 16, 16, (16,), 78)
    with pytest.raises(RuntimeError, match='WINOGRAD4_OUT'):
        run_conv_fused(0, srcs, w, 78, 1, 16, 16, gamma, beta, flags=_lib.CONV_WINOGRAD4_OUT)


def test_masked_launch_writes_live_tiles_only():
    """rnr_conv2d_masked with a seeded random mask (about half the 16 x 16 tiles off): live tiles bit-identical to the unmasked
    launch, skipped tiles leave a sentinel-filled out_raw untouched."""
    case = CASES[1]
    N, H, W, cins, c_out = case
    srcs, w, _, _, first, _, _ = run_case(case)
    d = conv_desc(0, cins, c_out, OUT)
    tiles = _lib.load().rnr_conv_tile_count(ctypes.byref(d), N, H, W)
    assert tiles == N * (H // 16) * (W // 16)
    rng = np.random.default_rng(80)
    mask = (rng.random(tiles) < 0.5).astype(np.uint8)
    mask[0], mask[-1] = 1, 0
    prefill = torch.full((N, H, W, 80), SENTINEL, dtype=torch.int32)
    out, _ = run_conv(0, srcs, w, c_out, N, H, W, flags=OUT, tile_mask=torch.from_numpy(mask), out=prefill)
    live = torch.from_numpy(mask.astype(bool)).reshape(N, H // 16, 1, W // 16, 1).expand(-1, -1, 16, -1, 16).reshape(N, H, W)
    assert 0.3 < float(live.float().mean()) < 0.7
    assert torch.equal(bits(out[live]), bits(first[0][live])), 'live tiles differ from the unmasked launch'
    assert bool((bits(out[~live]) == SENTINEL).all()), 'a masked-off tile was written'


def test_active_tiles_describe_16x16_blocks():
    """rnr_conv_active_tiles on an alpha map with a known block structure: one positive pixel in chosen 16 x 16 blocks (a corner,
    an edge, an interior pixel), zeros and negative values elsewhere."""
    N, H, W, cins, c_out = CASES[1]
    d = conv_desc(0, cins, c_out, OUT)
    rng = np.random.default_rng(81)
    want = (rng.random((N, H // 16, W // 16)) < 0.4).astype(np.uint8)
    want[0, 0, 0], want[-1, -1, -1] = 1, 0
    alpha = np.where(rng.random((N, H, W)) < 0.5, 0.0, -1.0).astype(np.float32)
    for k, (n, ty, tx) in enumerate(zip(*np.nonzero(want))):
        dy, dx = [(0, 0), (15, 15), (0, 15), (7, 9), (15, 0)][k % 5]
        alpha[n, 16 * ty + dy, 16 * tx + dx] = 0.25
    buf = conv_active_tiles(d, alpha, N, H, W, guard=64, fill=0xAA)
    assert buf.numel() == want.size + 64
    assert np.array_equal(buf[:want.size].numpy(), want.reshape(-1))
    assert bool((buf[want.size:] == 0xAA).all()), 'bytes behind the mask were written'
