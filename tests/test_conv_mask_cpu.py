"""CPU: what tests/test_gpu_conv_mask_sweep.py rests on, checked without a GPU — the float64 restatements of oracle/conv64.py
against plainer ones, the exactness of the 'exact' inputs on every shape the sweep uses, and through the host-side planner
(no kernel launches) that every row of the sweep lands on the pixel tile it names and every refused shape is refused."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import conv64 as o64
from rnr_amd import _lib
from rnr_amd.testing import conv_desc
from test_gpu_conv_mask_sweep import MASKED_CASES, RAY_CASES, REFUSED_CASES, exact_case, ray_id


def L():
    return _lib.load()


def _reflect(i, n):
    return -i if i < 0 else (2 * (n - 1) - i if i >= n else i)


def conv_loops(kind, x, w):
    """Four loops over (view, output row, output column, output channel) straight from the definitions: ReflectionPad2d(1) +
    3x3, ReflectionPad2d(1) + 4x4 stride 2, ConvTranspose2d(4, stride 2, padding 1).  x [N,C,H,W], w in torch's layout; float64."""
    N, C, H, W = x.shape
    k = 3 if kind == 0 else 4
    c_out = w.shape[1] if kind == 2 else w.shape[0]
    Ho, Wo = (H, W) if kind == 0 else ((H // 2, W // 2) if kind == 1 else (2 * H, 2 * W))
    out = np.zeros((N, c_out, Ho, Wo))
    for n in range(N):
        for oy in range(Ho):
            for ox in range(Wo):
                for co in range(c_out):
                    s = 0.0
                    for ky in range(k):
                        for kx in range(k):
                            if kind == 2:       # out[oy] += x[iy] * w[ky] with oy = 2 iy - 1 + ky
                                ny, nx = oy + 1 - ky, ox + 1 - kx
                                if ny % 2 or nx % 2 or not (0 <= ny // 2 < H and 0 <= nx // 2 < W):
                                    continue
                                s += float(np.dot(x[n, :, ny // 2, nx // 2], w[:, co, ky, kx]))
                            else:
                                st = 1 if kind == 0 else 2
                                iy, ix = _reflect(st * oy - 1 + ky, H), _reflect(st * ox - 1 + kx, W)
                                s += float(np.dot(x[n, :, iy, ix], w[co, :, ky, kx]))
                    out[n, co, oy, ox] = s
    return out


@pytest.mark.parametrize('kind', [0, 1, 2])
def test_conv64_equals_a_four_loop_convolution(kind):
    """conv64 on a 2-view 4 x 6 map with a two-source concat (5 + 3 channels; scale / shift / LReLU on the first, shift / ReLU
    on the second, as the GPU tests feed it): reflect padding on all four borders is inside the map's 3x3 / 4x4 windows."""
    g = torch.Generator().manual_seed(40 + kind)
    N, H, W, cins, c_out = 2, 4, 6, [5, 3], 4
    srcs = [(torch.randn(N, cins[0], H, W, generator=g).double(), torch.rand(N, cins[0], generator=g).double() + 0.5,
             torch.randn(N, cins[0], generator=g).double(), 1),
            (torch.randn(N, cins[1], H, W, generator=g).double(), None, torch.randn(N, cins[1], generator=g).double(), 2)]
    k = 3 if kind == 0 else 4
    w = torch.randn((8, c_out, 4, 4) if kind == 2 else (c_out, 8, k, k), generator=g).double()
    xs = []
    for raw, sc, sh, act in srcs:
        x = raw.numpy() * (sc.numpy()[:, :, None, None] if sc is not None else 1.0) + sh.numpy()[:, :, None, None]
        xs.append(np.where(x > 0, x, 0.2 * x if act == 1 else 0.0))
    want = conv_loops(kind, np.concatenate(xs, 1), w.numpy())
    got = o64.conv64(kind, srcs, w)
    assert got.dtype == torch.float64 and tuple(got.shape) == want.shape
    assert float(np.abs(got.numpy() - want).max()) < 1e-13 * float(np.abs(want).max())


def test_tile_mask64_on_a_hand_written_example():
    """Two views of 4 x 6 pixels in 2 x 3 tiles: entries in (view, tile row, tile column) order; a tile is live through one
    corner pixel, never through negative values or zeros of either sign."""
    a = np.zeros((2, 4, 6), np.float32)
    a[0, 0, 0] = 1.0            # view 0, tile (0, 0): its first pixel
    a[0, 1, 5] = 1e-30          # view 0, tile (0, 1): its last pixel
    a[0, 2, 0:3] = -1.0         # view 0, tile (1, 0): negative only
    a[0, 3, 3] = -0.0           # view 0, tile (1, 1): -0.0
    a[1, 3, 5] = 0.5            # view 1, tile (1, 1): the very last pixel
    a[1, 1, 2] = 2.0            # view 1, tile (0, 0): its last pixel
    got = o64.tile_mask64(torch.from_numpy(a), 2, 3)
    assert got.dtype == torch.uint8 and got.tolist() == [1, 1, 0, 0, 1, 0, 0, 1]
    assert o64.tile_mask64(a, 4, 6).tolist() == [1, 1] and o64.tile_mask64(a, 1, 1).tolist() == (a > 0).reshape(-1).astype(int).tolist()


def test_ray_epilogue64_equals_its_formula():
    g = torch.Generator().manual_seed(3)
    conv, w, bias = torch.randn(2, 3, 4, 16, generator=g), torch.rand(2, 3, 4, 16, generator=g), torch.randn(16, generator=g)
    got = o64.ray_epilogue64(conv, bias, w, 12)
    assert got.dtype == torch.float64 and tuple(got.shape) == (2, 3, 3, 4)
    for c in range(3):
        want = sum((np.tanh(conv[..., 3 * r + c].double().numpy() + float(bias[3 * r + c])) + 1.0) * w[..., 3 * r + c].double().numpy()
                   for r in range(4))
        assert float(np.abs(got[:, c].numpy() - want).max()) < 1e-14


EXACT_SHAPES = [pytest.param(c.N, c.H, c.W, c.cins, c.c_out, id=c.id) for c in MASKED_CASES if not c.id.endswith('_f16x3')] + \
               [pytest.param(c.N, c.H, c.W, c.cins, c.c_out, id='ray-' + ray_id(c)) for c in RAY_CASES]


@pytest.mark.parametrize('N,H,W,cins,c_out', EXACT_SHAPES)
def test_exact_inputs_are_exact_in_float32(N, H, W, cins, c_out):
    """The property the bitwise GPU comparisons rest on, for every shape they use (the two emulation formats share their
    shapes): the inputs obey exact_conv_case's ranges, the float32 prologue act(scale * raw + shift) is exact, and conv64 cast
    to float32 equals torch's float32 convolution — another summation order — bit for bit, and is itself exact (no rounding in
    the cast)."""
    srcs, w = exact_case(N, H, W, cins, c_out)
    for raw, sc, sh, act in srcs:
        assert raw.dtype == torch.float32 and torch.equal(raw, raw.round()) and float(raw.abs().max()) <= 3
        assert set(sc.unique().tolist()) <= {0.5, 1.0, 2.0}
        assert torch.equal(sh * 2, (sh * 2).round()) and float(sh.abs().max()) <= 1.5
        assert act in (o64.ACT_NONE, o64.ACT_RELU)
    assert torch.equal(w * 8, (w * 8).round()) and float(w.abs().max()) <= 0.25 and w.unique().numel() == 5
    x32 = o64.conv_input(srcs)
    x64 = o64.conv_input([(raw.double(), sc.double(), sh.double(), act) for raw, sc, sh, act in srcs])
    assert torch.equal(x32.double(), x64) and float(x32.abs().max()) <= 7.5
    ref = o64.conv64(0, srcs, w)
    assert torch.equal(ref.float().double(), ref)
    f32 = F.conv2d(F.pad(x32, (1, 1, 1, 1), mode='reflect'), w)
    assert torch.equal((ref.float() + 0.0).view(torch.int32), (f32 + 0.0).view(torch.int32))
    assert torch.equal(ref * 16, (ref * 16).round())            # sums of multiples of 2^-4


@pytest.mark.parametrize('c', MASKED_CASES, ids=lambda c: c.id)
def test_plan_geometry_of_the_masked_cases(c):
    """Every row of the sweep has N * (H / th) * (W / tw) maskable tiles with the th x tw it names (default tuning), no split-K
    workspace, and the algorithm its kernel family reports."""
    d = conv_desc(0, c.cins, c.c_out, c.flags)
    assert c.H % c.th == 0 and c.W % c.tw == 0
    assert L().rnr_conv_tile_count(ctypes.byref(d), c.N, c.H, c.W) == c.N * (c.H // c.th) * (c.W // c.tw)
    assert L().rnr_conv_workspace_bytes(ctypes.byref(d), c.N, c.H, c.W) == 256
    assert L().rnr_conv_algorithm(ctypes.byref(d), c.N, c.H, c.W) == (3 if c.flags & _lib.CONV_WINOGRAD else 0)


def test_the_masked_cases_cover_every_maskable_tile():
    """(th, tw) of the rows: 16 x 4 of the out layer's Winograd kernel, 32 x 8 / 32 x 4 / 32 x 2 of the halo kernels — with both
    emulation formats and with one and two column tiles."""
    assert {(c.th, c.tw) for c in MASKED_CASES} == {(4, 16), (8, 32), (4, 32), (2, 32)}
    assert {c.flags for c in MASKED_CASES} == {0, _lib.CONV_WINOGRAD, _lib.CONV_F32_EMU_BF16X6, _lib.CONV_F32_EMU_F16X3}
    assert len({c.id for c in MASKED_CASES}) == len(MASKED_CASES) == 15


@pytest.mark.parametrize('kind,N,H,W,cins,c_out', REFUSED_CASES)
def test_plan_refuses_a_mask(kind, N, H, W, cins, c_out):
    assert L().rnr_conv_tile_count(ctypes.byref(conv_desc(kind, cins, c_out)), N, H, W) == 0


@pytest.mark.parametrize('c', RAY_CASES, ids=ray_id)
def test_plan_geometry_of_the_ray_cases(c):
    """The mask of a ray launch: 32 x 8 tiles from the descriptor without Winograd flags on the one size with at least 257
    direct tiles (16 x 4 tiles with the flag: not the ray launch's layout), none on the two small maps."""
    big = (c.N, c.H, c.W) == (3, 96, 320)
    plain, wino = conv_desc(0, c.cins, c.c_out), conv_desc(0, c.cins, c.c_out, _lib.CONV_WINOGRAD)
    assert L().rnr_conv_tile_count(ctypes.byref(plain), c.N, c.H, c.W) == (c.N * (c.H // 8) * (c.W // 32) if big else 0)
    assert L().rnr_conv_tile_count(ctypes.byref(wino), c.N, c.H, c.W) == (c.N * (c.H // 4) * (c.W // 16) if big else 0)
