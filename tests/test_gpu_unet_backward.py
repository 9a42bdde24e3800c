"""-m gpu: the HIP backward of the U-Net (csrc/unet_bwd.hip, UNetPlan(training=True), rnr_amd.autograd.UNetFn) against float64
torch autograd (tests/unet_bwd_ref.py, pinned on the CPU by tests/test_unet_backward_cpu.py).

Bounds come from the arithmetic, never from a measured error:
  * sums made in float32 (weight gradient, ring pixels): (n + 4) 2^-24 sum|terms|, n the number of summands;
  * sums made in float64 (BatchNorm / bias gradients): 4 2^-24 sum|terms|; g_y: 16 roundings of the formula's term magnitudes;
  * interior pixels of the data gradient, which the forward kernels compute: those kernels' own bound, 1e-4 of the output peak;
  * whole network: relative rms error per tensor at most RATIO x that of torch's float32 autograd on the CPU (computed here);
    the issue's condition is 8, tightened to twice the largest measured ratio as it asks (see RATIO); the cases at production
    width (nf0 = 64) keep the derived 8.
The `*_wide` tests and test_unet_out_backward take their shapes from oracle/unet_bwd_cases.py: the channel widths of the trained
network on maps of a few pixels, with the same bounds — they do not depend on width.
Every direct call of the C ABI starts from outputs filled with NaN and is repeated: the second result must have the same bits."""
import ctypes

import pytest
import torch

import unet_bwd_ref as ub
from oracle import unet_bwd_cases as uc
from unet_bwd_ref import EPS

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
D = torch.float64
ACTS = {0: None, 1: 'lrelu', 2: 'relu'}


def _pad16(c):
    return (c + 15) // 16 * 16


def _L():
    from rnr_amd import _lib
    return _lib.load()


def _nhwc(x, c_pad=None):
    """[N,C,H,W] (CPU) -> float32 [N,H,W,c_pad] on the device, padding channels 0."""
    from rnr_amd.testing import channel_last
    return channel_last(x, c_pad).to(DEV)


def _nchw(t, c):
    return t.cpu()[..., :c].permute(0, 3, 1, 2).contiguous()


def _padc(v, c_pad):
    out = torch.zeros(v.shape[0], c_pad, dtype=torch.float32)
    out[:, :v.shape[1]] = v
    return out.to(DEV).contiguous()


def _check(rc):
    from rnr_amd import _lib
    _lib.check(rc)


class _Src:
    """One convolution source: raw values, per-view scale / shift and an activation; .x64 = the consumer-side value in float64
    from the float32 operands."""

    def __init__(self, g, n, c, h, w, act):
        from rnr_amd._lib import RnrConvSrc
        self.c, self.c_pad, self.act = c, _pad16(c), act
        self.raw = torch.randn(n, c, h, w, generator=g)
        self.scale = torch.rand(n, c, generator=g) + 0.5
        self.shift = torch.randn(n, c, generator=g) * 0.5
        v = self.raw.double() * self.scale.double()[:, :, None, None] + self.shift.double()[:, :, None, None]
        self.x64 = ub.act(v, ACTS[act])
        self.d_raw, self.d_scale, self.d_shift = _nhwc(self.raw), _padc(self.scale, self.c_pad), _padc(self.shift, self.c_pad)
        self.struct = RnrConvSrc(self.d_raw.data_ptr(), self.d_scale.data_ptr(), self.d_shift.data_ptr(), self.c_pad, act)


def _desc(kind, cins, cout, flags=0):
    from rnr_amd._lib import RnrConvDesc
    c1 = cins[1] if len(cins) > 1 else 0
    return RnrConvDesc(kind, cins[0], _pad16(cins[0]), c1, _pad16(c1) if c1 else 0, cout, _pad16(cout), flags)


# ------------------------------------------------------------------------------------------------
# 1. weight gradient
# ------------------------------------------------------------------------------------------------
WG_SHAPES = [(2, 6, 10, (5, 3), 7), (1, 2, 2, (5, 3), 7), (2, 32, 16, (64,), 64), (3, 40, 24, (24, 40), 80)]


@pytest.mark.parametrize('kind', [0, 1, 2])
@pytest.mark.parametrize('N,H,W,cins,cout', WG_SHAPES, ids=lambda v: str(v).replace(' ', ''))
def test_weight_gradient_vs_float64_autograd(N, H, W, cins, cout, kind):
    _check_weight_gradient(N, H, W, cins, cout, kind)


WG_WIDE = [(c, k) for c in uc.WG_CASES for k in c['kinds']]


@pytest.mark.parametrize('case,kind', WG_WIDE, ids=['%s-k%d' % (c['id'], k) for c, k in WG_WIDE])
def test_weight_gradient_wide(case, kind):
    """oracle/unet_bwd_cases.py: every wave tile of wg_kernel, more than one tile per axis, ragged slices, production width."""
    _check_weight_gradient(case['N'], case['H'], case['W'], case['cins'], case['c_out'], kind)


def _check_weight_gradient(N, H, W, cins, cout, kind):
    from rnr_amd import ops
    L = _L()
    g = torch.Generator().manual_seed(1000 * kind + H * W + cout)
    srcs = [_Src(g, N, c, H, W, act) for c, act in zip(cins, (1, 2))]
    oh, ow = ub.out_hw(kind, H, W)
    gy = torch.randn(N, cout, oh, ow, generator=g)
    cin, k = sum(cins), 3 if kind == 0 else 4
    wshape = (cin, cout, k, k) if kind == 2 else (cout, cin, k, k)
    x = torch.cat([s.x64 for s in srcs], 1)

    def grad_w(xx, gg):     # the gradient is linear in W: evaluate it at W = 0
        wz = torch.zeros(wshape, dtype=D, requires_grad=True)
        (ub.conv_forward(kind, xx, wz) * gg).sum().backward()
        return wz.grad
    ref, mag = grad_w(x, gy.double()), grad_w(x.abs(), gy.double().abs())
    bound = (N * oh * ow + 4) * EPS * mag

    d = _desc(kind, cins, cout)
    d_gy = _nhwc(gy)
    ws = torch.empty(L.rnr_conv2d_weight_backward_workspace_bytes(ctypes.byref(d), N, H, W), dtype=torch.uint8, device=DEV)
    outs = []
    for _ in range(2):
        out = torch.full(wshape, float('nan'), dtype=torch.float32, device=DEV)
        _check(L.rnr_conv2d_weight_backward(ctypes.byref(d), ctypes.byref(srcs[0].struct),
                                            ctypes.byref(srcs[1].struct) if len(srcs) > 1 else None, ops._ptr(d_gy), ops._ptr(out),
                                            N, H, W, ops._ptr(ws), ws.numel(), ops._stream()))
        torch.cuda.synchronize()
        outs.append(out.cpu())
    got = outs[0]
    assert torch.isfinite(got).all(), 'output not overwritten everywhere'
    err = (got.double() - ref).abs()
    print('weight gradient kind %d %s: worst error / bound = %.3f' % (kind, (N, H, W, cins, cout), float((err / bound.clamp_min(1e-300)).max())))
    assert (err <= bound).all(), float((err / bound.clamp_min(1e-300)).max())
    assert torch.equal(outs[0], outs[1]), 'two runs differ'


# ------------------------------------------------------------------------------------------------
# 2. data gradient: the forward kernels on g_y + the ring kernel
# ------------------------------------------------------------------------------------------------
def _data_gradient(L, d, kind, wt, cins, d_gy, N, H, W):
    """The recipe of include/rnr_hip.h for every source -> [(grad_in [N,H,W,c_s_pad] on the CPU, gradient descriptor)]; every
    source is computed twice from NaN-filled outputs and the two results must have the same bits."""
    from rnr_amd import ops
    from rnr_amd._lib import RnrConvDesc, RnrConvSrc
    oh, ow = ub.out_hw(kind, H, W)
    d_w = wt.to(DEV).contiguous()
    res, off = [], 0
    for s, c in enumerate(cins):
        bd = RnrConvDesc()
        _check(L.rnr_conv_backward_desc(ctypes.byref(d), s, ctypes.byref(bd)))
        if kind == 0:
            wb = wt[:, off:off + c].flip(2, 3).transpose(0, 1)
        elif kind == 1:
            wb = wt[:, off:off + c]
        else:
            wb = wt[off:off + c]
        wb = wb.contiguous().to(DEV)
        packed = torch.empty(L.rnr_packed_weight_floats(ctypes.byref(bd)), dtype=torch.float32, device=DEV)
        _check(L.rnr_pack_conv_weight(ctypes.byref(bd), ops._ptr(wb), ops._ptr(packed), ops._stream()))
        ws = torch.empty(max(256, L.rnr_conv_workspace_bytes(ctypes.byref(bd), N, oh, ow)), dtype=torch.uint8, device=DEV)
        src = RnrConvSrc(d_gy.data_ptr(), None, None, d.c_out_pad, 0)
        runs = []
        for _ in range(2):
            gin = torch.full((N, H, W, bd.c_out_pad), float('nan'), dtype=torch.float32, device=DEV)
            _check(L.rnr_conv2d(ctypes.byref(bd), ctypes.byref(src), None, ops._ptr(packed), ops._ptr(gin), None, N, oh, ow,
                                ops._ptr(ws), ws.numel(), ops._stream()))
            _check(L.rnr_conv2d_input_backward_ring(ctypes.byref(d), s, ops._ptr(d_gy), ops._ptr(d_w), ops._ptr(gin), N, H, W,
                                                    ops._stream()))
            torch.cuda.synchronize()
            runs.append(gin.cpu())
        assert torch.equal(runs[0], runs[1]), 'two runs differ'
        res.append((runs[0], bd))
        off += c
    return res


def _check_data_gradient(kind, N, H, W, cins, cout, flags=0, seed=0):
    L = _L()
    g = torch.Generator().manual_seed(seed + 77 * kind + H + W)
    cin, k = sum(cins), 3 if kind == 0 else 4
    oh, ow = ub.out_hw(kind, H, W)
    wt = torch.randn((cin, cout, k, k) if kind == 2 else (cout, cin, k, k), generator=g) / (cout * k * k) ** 0.5
    gy = torch.randn(N, cout, oh, ow, generator=g)
    x0 = torch.zeros(N, cin, H, W, dtype=D)
    ref = ub.autograd_input_grad(kind, x0, wt, gy)                              # the operator is linear: x does not matter
    mag = ub.autograd_input_grad(kind, x0, wt.abs(), gy.abs())                  # sum of the terms' magnitudes
    cnt = ub.autograd_input_grad(kind, x0[:1, :1], torch.ones(((1, cout, k, k) if kind == 2 else (cout, 1, k, k))),
                                 torch.ones(1, cout, oh, ow))[0, 0]             # number of summands per pixel
    ring = ub.ring_mask(kind, H, W)
    d = _desc(kind, cins, cout, flags)
    res = _data_gradient(L, d, kind, wt, cins, _nhwc(gy), N, H, W)
    off = 0
    for (got_t, bd), c in zip(res, cins):
        assert torch.isfinite(got_t).all(), 'output not overwritten everywhere'
        assert (got_t[..., c:] == 0).all(), 'padding channels must be 0'
        got = _nchw(got_t, c).double()
        r, m = ref[:, off:off + c], mag[:, off:off + c]
        err = (got - r).abs()
        rb = (cnt + 4)[None, None] * EPS * m
        worst_ring = float((err / rb.clamp_min(1e-300))[:, :, ring].max())
        assert (err <= rb)[:, :, ring].all(), worst_ring
        worst_in = 0.0
        if (~ring).any():
            worst_in = float(err[:, :, ~ring].max() / r.abs().max())
            assert worst_in <= 1e-4, worst_in
        print('data gradient kind %d N%d %dx%d source %d: ring worst error / bound %.3f, interior worst / peak %.2e'
              % (kind, N, H, W, off and 1, worst_ring, worst_in))
        off += c
    return res


@pytest.mark.parametrize('kind,hw', [(k, s) for k in (0, 1, 2) for s in [(2, 2), (4, 6), (3, 4), (40, 24)]
                                     if not (k == 1 and s == (3, 4))], ids=lambda v: str(v).replace(' ', ''))
def test_data_gradient_vs_float64_autograd(kind, hw):
    _check_data_gradient(kind, 2, hw[0], hw[1], (5, 3), 7)


@pytest.mark.parametrize('kind,N,H,W,cins,cout', uc.DG_CASES, ids=lambda v: str(v).replace(' ', ''))
def test_data_gradient_wide(kind, N, H, W, cins, cout):
    """144 gradient-input columns from sources of 72 and 60 live channels; the 1 x 1 input of the transposed kind."""
    _check_data_gradient(kind, N, H, W, cins, cout)


WINO_CANDIDATES = [(1, 64, 64), (2, 64, 64), (1, 128, 128), (2, 128, 128), (1, 256, 256), (2, 256, 256), (1, 512, 512), (2, 512, 512)]


@pytest.mark.parametrize('kind', [0, 1, 2])
def test_data_gradient_on_a_winograd_plan(kind):
    """The first candidate shape whose gradient descriptor rnr_conv_algorithm puts on a Winograd kernel (64-channel sources, the
    flags UNetPlan's default conv_algo sets for the forward)."""
    from rnr_amd import _lib
    from rnr_amd._lib import RnrConvDesc
    L = _L()
    own = {0: _lib.CONV_WINOGRAD4, 1: _lib.CONV_WINOGRAD42S, 2: _lib.CONV_WINOGRAD42}[kind]
    flags = _lib.CONV_WINOGRAD | own
    cins, cout = (64, 64), 64
    d = _desc(kind, cins, cout, flags)
    bd = RnrConvDesc()
    _check(L.rnr_conv_backward_desc(ctypes.byref(d), 0, ctypes.byref(bd)))
    shape = None
    for n, h, w in WINO_CANDIDATES:
        oh, ow = ub.out_hw(kind, h, w)
        if L.rnr_conv_algorithm(ctypes.byref(bd), n, oh, ow) > 0:
            shape = (n, h, w)
            break
    assert shape is not None, 'no candidate shape runs the gradient convolution on a Winograd kernel'
    print('kind %d: Winograd gradient plan at N %d, %d x %d (algorithm %d, tile %d)'
          % (kind, *shape, L.rnr_conv_algorithm(ctypes.byref(bd), shape[0], *ub.out_hw(kind, *shape[1:])),
             L.rnr_conv_winograd_tile(ctypes.byref(bd), shape[0], *ub.out_hw(kind, *shape[1:]))))
    _check_data_gradient(kind, shape[0], shape[1], shape[2], cins, cout, flags, seed=5)


# ------------------------------------------------------------------------------------------------
# 3. rnr_conv_out_backward and rnr_bn_finalize_saved
# ------------------------------------------------------------------------------------------------
def _out_backward_draw(g, N, h, w, c, c_pad, mode, bn, two):
    eps = 1e-5
    y = torch.randn(N, c, h, w, generator=g) * 1.5 + 0.3
    gz0 = torch.randn(N, c, h, w, generator=g)
    gz1 = torch.randn(N, c, h, w, generator=g) if two else None
    y64 = y.double()
    gamma = saved = mu = r = None
    if bn:
        gamma = torch.randn(c, generator=g)
        gamma[2] = 0.0
        beta = torch.randn(c, generator=g)
        if mode == 0:
            mu, var = y64.mean((2, 3)), y64.var((2, 3), unbiased=False)                  # [N,c]
        elif mode == 1:
            mu, var = y64.mean((0, 2, 3))[None], y64.var((0, 2, 3), unbiased=False)[None]   # [1,c]
        else:
            mu, var = torch.randn(1, c, generator=g).double() * 0.3, torch.rand(1, c, generator=g).double() + 0.5
        r = 1.0 / torch.sqrt(var + eps)
        scale = (gamma.double()[None] * r).float().expand(N, c).contiguous()
        shift = (beta.double()[None] - mu * gamma.double()[None] * r).float().expand(N, c).contiguous()
        saved = torch.zeros(mu.shape[0], c_pad, 2, dtype=D)
        saved[:, :c, 0], saved[:, :c, 1] = mu, r
    else:
        scale, shift = None, torch.randn(1, c, generator=g).expand(N, c).contiguous()       # a bias
    v = y64 * (scale.double()[:, :, None, None] if scale is not None else 1.0) + shift.double()[:, :, None, None]
    return y, gz0, gz1, gamma, saved, scale, shift, mu, r, v


def _out_backward_find(g, N, h, w, c, c_pad, mode, bn, two):
    """CPU draws, deterministic: the first one without a pre-activation next to the kink -> (draw, number of draws)."""
    for tries in range(1, 101):
        case = _out_backward_draw(g, N, h, w, c, c_pad, mode, bn, two)
        if float(case[-1].abs().min()) > 1e-4:
            break
    return case, tries


def _out_backward_case(L, g, N, h, w, c, mode, act, bn, two, c_pad=None):
    """-> worst error / bound of (g_y, g_beta, g_gamma); 0 for g_gamma without BatchNorm."""
    from rnr_amd import ops
    c_pad = c_pad or _pad16(c)
    case, _ = _out_backward_find(g, N, h, w, c, c_pad, mode, bn, two)
    y, gz0, gz1, gamma, saved, scale, shift, mu, r, v = case
    y64 = y.double()
    assert float(v.abs().min()) > 1e-4, 'a pre-activation too close to the kink'
    slope = {0: 1.0, 1: 0.2, 2: 0.0}[act]
    gz = (gz0 + gz1) if two else gz0                                                      # one float32 rounding, as the kernel
    gv = gz.double() * torch.where(v > 0, 1.0, slope)
    gv_mag = ((gz0.double().abs() + gz1.double().abs()) if two else gz0.double().abs()) * torch.where(v > 0, 1.0, slope)
    if bn and mode != 2:
        grp = (2, 3) if mode == 0 else (0, 2, 3)
        m = h * w if mode == 0 else N * h * w
        mu_b, r_b = (mu[:, :, None, None], r[:, :, None, None])
        S1 = gv.sum(grp, keepdim=True)
        Dm = (gv * (y64 - mu_b) * r_b).sum(grp, keepdim=True)
        ga = gamma.double()[None, :, None, None]
        ref_gy = ga * r_b * (gv - S1 / m - (y64 - mu_b) * r_b * Dm / m)
        mag_gy = (ga * r_b).abs() * (gv_mag + S1.abs() / m + ((y64 - mu_b) * r_b * Dm / m).abs())
        ref_gg, mag_gg = Dm.sum((0, 2, 3)), (gv_mag * ((y64 - mu_b) * r_b).abs()).sum((0, 2, 3))
    elif bn:
        ref_gy, mag_gy = scale.double()[:, :, None, None] * gv, scale.double().abs()[:, :, None, None] * gv_mag
        t = (y64 - mu[:, :, None, None]) * r[:, :, None, None]
        ref_gg, mag_gg = (gv * t).sum((0, 2, 3)), (gv_mag * t.abs()).sum((0, 2, 3))
    else:
        ref_gy, mag_gy, ref_gg, mag_gg = gv, gv_mag, None, None
    ref_gb, mag_gb = gv.sum((0, 2, 3)), gv_mag.sum((0, 2, 3))

    d_y, d_g0, d_g1 = _nhwc(y, c_pad), _nhwc(gz0, c_pad), (_nhwc(gz1, c_pad) if two else None)
    d_sc = _padc(scale, c_pad) if scale is not None else None
    d_sh = _padc(shift, c_pad)
    d_gamma = gamma.to(DEV) if bn else None
    d_saved = saved.to(DEV) if bn else None
    ws = torch.empty(L.rnr_conv_out_backward_workspace_bytes(N, h, w, c_pad), dtype=torch.uint8, device=DEV)
    runs = []
    for _ in range(2):
        o_gy = torch.full((N, h, w, c_pad), float('nan'), dtype=torch.float32, device=DEV)
        o_gg = torch.full((c,), float('nan'), dtype=torch.float32, device=DEV)
        o_gb = torch.full((c,), float('nan'), dtype=torch.float32, device=DEV)
        _check(L.rnr_conv_out_backward(ops._ptr(d_y), ops._ptr(d_sc), ops._ptr(d_sh), act, ops._ptr(d_g0), ops._ptr(d_g1),
                                       ops._ptr(d_gamma), ops._ptr(d_saved), mode, ops._ptr(o_gy), ops._ptr(o_gg), ops._ptr(o_gb),
                                       N, h, w, c, c_pad, ops._ptr(ws), ws.numel(), ops._stream()))
        torch.cuda.synchronize()
        runs.append((o_gy.cpu(), o_gg.cpu(), o_gb.cpu()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][2], runs[1][2]), 'two runs differ'
    o_gy, o_gg, o_gb = runs[0]
    assert (o_gy[..., c:] == 0).all(), 'padding channels must be 0'
    tag = 'mode %d act %d bn %d two %d' % (mode, act, bn, two)
    e = (_nchw(o_gy, c).double() - ref_gy).abs()
    worst = [float((e / (16 * EPS * mag_gy).clamp_min(1e-300)).max()), 0.0, 0.0]
    assert (e <= 16 * EPS * mag_gy).all(), (tag, worst[0])
    e = (o_gb.double() - ref_gb).abs()
    worst[1] = float((e / (4 * EPS * mag_gb).clamp_min(1e-300)).max())
    assert (e <= 4 * EPS * mag_gb).all(), (tag, 'g_beta', worst[1])
    if bn:
        assert torch.equal(runs[0][1], runs[1][1])
        e = (o_gg.double() - ref_gg).abs()
        worst[2] = float((e / (4 * EPS * mag_gg).clamp_min(1e-300)).max())
        assert (e <= 4 * EPS * mag_gg).all(), (tag, 'g_gamma', worst[2])
    else:
        assert torch.isnan(o_gg).all(), 'g_gamma must not be written without BatchNorm'
    return worst


@pytest.mark.parametrize('hw', [(5, 7), (16, 16)], ids=lambda s: '%dx%d' % s)
def test_conv_out_backward(hw):
    L = _L()
    g = torch.Generator().manual_seed(hw[0] * 31 + hw[1])
    for act in (0, 1, 2):
        for two in (False, True):
            for mode in (0, 1, 2):
                _out_backward_case(L, g, 3, hw[0], hw[1], 7, mode, act, True, two)
            _out_backward_case(L, g, 3, hw[0], hw[1], 7, 0, act, False, two)


def out_backward_wide_seed(case):
    return case['c_pad'] * 131 + case['h'] * 31 + case['w']


@pytest.mark.parametrize('case', uc.OB_CASES, ids=[c['id'] for c in uc.OB_CASES])
def test_conv_out_backward_wide(case):
    """oracle/unet_bwd_cases.py: idle lanes in the reduce workgroup, parameter gradients in two workgroups, OB_MAX_CPAD, ragged
    parts and apply workgroups — over the grid of test_conv_out_backward (uc.OB_GRID, the bias-only form included)."""
    L = _L()
    g = torch.Generator().manual_seed(out_backward_wide_seed(case))
    worst = [0.0, 0.0, 0.0]
    for act, two, mode, bn in uc.OB_GRID:
        got = _out_backward_case(L, g, case['N'], case['h'], case['w'], case['c'], mode, act, bn, two, case['c_pad'])
        worst = [max(a, b) for a, b in zip(worst, got)]
    print('conv_out_backward %s: worst error / bound g_y %.3f, g_beta %.3f, g_gamma %.3f' % ((case['id'],) + tuple(worst)))


def test_conv_out_backward_refuses_more_than_1024_columns():
    """c_pad = 1040: an error that names the limit, before any launch (the outputs keep their NaN)."""
    from rnr_amd import _lib, ops
    L = _L()
    N, h, w, c_pad = 1, 2, 2, uc.OB_REFUSED_CPAD
    c = c_pad - 3
    y, gz = torch.randn(N, h, w, c_pad, device=DEV), torch.randn(N, h, w, c_pad, device=DEV)
    o_gy = torch.full((N, h, w, c_pad), float('nan'), device=DEV)
    o_gb = torch.full((c,), float('nan'), device=DEV)
    nbytes = L.rnr_conv_out_backward_workspace_bytes(N, h, w, c_pad)
    ws = torch.full((nbytes // 4,), float('nan'), device=DEV)
    with pytest.raises(_lib.RnrError, match=r'at most %d\b' % uc.OB_MAX_CPAD):
        null = ops._ptr(None)
        _check(L.rnr_conv_out_backward(ops._ptr(y), null, null, 1, ops._ptr(gz), null, null, null, 0, ops._ptr(o_gy), null,
                                       ops._ptr(o_gb), N, h, w, c, c_pad, ops._ptr(ws), nbytes, ops._stream()))
    torch.cuda.synchronize()
    assert torch.isnan(o_gy).all() and torch.isnan(o_gb).all() and torch.isnan(ws).all(), 'a refused call launched something'


# ------------------------------------------------------------------------------------------------
# 3b. rnr_unet_out_backward
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('apply_tanh', [0, 1])
@pytest.mark.parametrize('n,c,h,w,c_pad', uc.UO_CASES, ids=lambda v: str(v))
def test_unet_out_backward(n, c, h, w, c_pad, apply_tanh):
    """g_raw[n,h,w,ch] = g_out[n,ch,h,w] (1 - out^2) against float64 from the float32 operands.  The kernel rounds o^2, 1 - o^2
    and the product: three roundings of the term magnitude |g| (1 + o^2); without tanh it copies, so the bits are g_out's and
    `out` may be NULL.  Padding channels exactly 0."""
    from rnr_amd import ops
    L = _L()
    g = torch.Generator().manual_seed(n * 1000 + c)
    g_out = torch.randn(n, c, h, w, generator=g)
    out = torch.tanh(torch.randn(n, c, h, w, generator=g) * 1.5)
    assert (n * h * w * c_pad) % 256 != 0
    d_g, d_o = g_out.to(DEV), (out.to(DEV) if apply_tanh else None)
    runs = []
    for _ in range(2):
        raw = torch.full((n, h, w, c_pad), float('nan'), device=DEV)
        _check(L.rnr_unet_out_backward(ops._ptr(d_g), ops._ptr(d_o), apply_tanh, ops._ptr(raw), n, c, h, w, c_pad, ops._stream()))
        torch.cuda.synchronize()
        runs.append(raw.cpu())
    assert torch.equal(runs[0], runs[1]), 'two runs differ'
    got = runs[0]
    assert torch.isfinite(got).all(), 'output not overwritten everywhere'
    assert (got[..., c:] == 0).all(), 'padding channels must be 0'
    if apply_tanh:
        ref = g_out.double() * (1 - out.double() ** 2)
        bound = 3 * EPS * g_out.double().abs() * (1 + out.double() ** 2)
        err = (_nchw(got, c).double() - ref).abs()
        worst = float((err / bound.clamp_min(1e-300)).max())
        print('unet_out_backward %s tanh: worst error / bound = %.3f' % ((n, c, h, w, c_pad), worst))
        assert (err <= bound).all(), worst
    else:
        assert torch.equal(_nchw(got, c), g_out), 'without tanh the gradient is copied'
        print('unet_out_backward %s no tanh: bitwise copy' % ((n, c, h, w, c_pad),))


@pytest.mark.parametrize('whole', [0, 1])
def test_bn_finalize_saved_has_the_existing_bits(whole):
    """One stand-alone finalise kernel sits behind rnr_bn_finalize, _reset, _batch and _saved: the same bits from each, statistics
    reset by all but the first."""
    _bn_finalize_case(whole, 3, 7, 16)


@pytest.mark.parametrize('whole', [0, 1])
def test_bn_finalize_saved_on_more_than_one_workgroup(whole):
    """N=2, c=260, c_pad=272: the smallest shape with more than one 256-lane workgroup and a ragged tail in both grids (272
    lanes for the whole batch, 544 per view)."""
    _bn_finalize_case(whole, 2, 260, 272)


def _bn_finalize_case(whole, N, c, c_pad):
    from rnr_amd import ops
    L = _L()
    g = torch.Generator().manual_seed(3 + whole)
    count = 35.0
    y = torch.randn(N, c, 35, generator=g, dtype=D) * 2 + 1
    stats = torch.zeros(N, c_pad, 2, dtype=D)
    stats[:, :c, 0], stats[:, :c, 1] = y.sum(2), (y * y).sum(2)
    gamma, beta = torch.randn(c, generator=g).to(DEV), torch.randn(c, generator=g).to(DEV)
    mk = lambda: (torch.full((N, c_pad), float('nan'), device=DEV), torch.full((N, c_pad), float('nan'), device=DEV))
    (sc0, sh0), (sc1, sh1) = mk(), mk()
    rm0, rv0 = torch.rand(c, generator=g).to(DEV), (torch.rand(c, generator=g) + 0.5).to(DEV)
    rm1, rv1 = rm0.clone(), rv0.clone()
    st0, st1 = stats.to(DEV), stats.to(DEV)
    saved = torch.full((1 if whole else N, c_pad, 2), float('nan'), dtype=D, device=DEV)
    if whole:
        _check(L.rnr_bn_finalize_batch(ops._ptr(st0), ops._ptr(gamma), ops._ptr(beta), ops._ptr(sc0), ops._ptr(sh0), ops._ptr(rm0),
                                       ops._ptr(rv0), 0.1, N, c, c_pad, count, 1e-5, ops._stream()))
    else:
        # plain rnr_bn_finalize first: the same affine, the statistics untouched
        st2, (sc2, sh2) = stats.to(DEV), mk()
        _check(L.rnr_bn_finalize(ops._ptr(st2), ops._ptr(gamma), ops._ptr(beta), ops._ptr(sc2), ops._ptr(sh2), N, c, c_pad, count,
                                 1e-5, ops._stream()))
        _check(L.rnr_bn_finalize_reset(ops._ptr(st0), ops._ptr(gamma), ops._ptr(beta), ops._ptr(sc0), ops._ptr(sh0), N, c, c_pad,
                                       count, 1e-5, ops._stream()))
    _check(L.rnr_bn_finalize_saved(ops._ptr(st1), ops._ptr(gamma), ops._ptr(beta), ops._ptr(sc1), ops._ptr(sh1),
                                   ops._ptr(rm1) if whole else None, ops._ptr(rv1) if whole else None, 0.1, ops._ptr(saved), whole,
                                   N, c, c_pad, count, 1e-5, ops._stream()))
    torch.cuda.synchronize()
    assert torch.equal(sc0, sc1) and torch.equal(sh0, sh1) and torch.equal(rm0, rm1) and torch.equal(rv0, rv1)
    assert (st0 == 0).all() and (st1 == 0).all()
    if not whole:
        assert torch.equal(sc2, sc1) and torch.equal(sh2, sh1) and torch.equal(st2.cpu(), stats)
    yy = y.permute(1, 0, 2).reshape(c, -1)[None] if whole else y
    mu, var = yy.mean(2), yy.var(2, unbiased=False)
    sv = saved.cpu()
    torch.testing.assert_close(sv[:, :c, 0], mu, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(sv[:, :c, 1], 1 / torch.sqrt(var + 1e-5), rtol=1e-10, atol=0)
    assert (sv[:, c:] == 0).all()
    assert (sc1[:, c:] == 0).all() and (sh1[:, c:] == 0).all()


# ------------------------------------------------------------------------------------------------
# 4. whole network
# ------------------------------------------------------------------------------------------------
# (num_down, N, H, W, bn train mode) -> seed chosen on the CPU so that the float64 oracle has no pre-activation with |v| < 2e-5
NET_SEEDS = {(2, 2, 32, 32, True): 14, (5, 2, 32, 32, True): 3, (2, 1, 64, 32, True): 32, (5, 1, 64, 32, True): 6,
             (2, 2, 32, 32, False): 127, (5, 2, 32, 32, False): 21}
# The issue's condition is 8 (4.5 x rms rounding of F(4x4, .) over the direct form, plus another summation order); the measured
# ratios came out at 1.3 .. 2.55 (profiles/unet_backward_accuracy.txt), so the constant is tightened to twice the largest, 2.552.
RATIO = 5.1
# Production width, nf0 = 64 with three levels: weights up to [512,128,4,4] and [256,256,.,.] on maps of 8 x 8 down to 1 x 1.
# (nf0, num_down, N, H, W, bn train mode) -> seed, found on the CPU under the same condition.  RATIO was tightened from
# measurements at nf0 = 4 and is not assumed at this width: these cases keep the derived condition, 8.
WIDE_NET_SEEDS = {(64, 3, 1, 8, 8, True): 57, (64, 3, 2, 8, 8, True): 38, (64, 3, 2, 8, 8, False): 1729}
RATIO_WIDE = 8.0


def _make_net(num_down, seed, use_gcn=False, nf0=4):
    import network
    torch.manual_seed(seed)
    net = network.RenderingNet(nf0=nf0, in_channels=16, out_channels=6, num_down_unet=num_down, use_gcn=use_gcn)
    g = torch.Generator().manual_seed(seed + 1)
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.weight.data = torch.rand(m.weight.shape, generator=g) + 0.5
            m.bias.data = torch.randn(m.bias.shape, generator=g) * 0.2
            m.running_mean.data = torch.randn(m.running_mean.shape, generator=g) * 0.2
            m.running_var.data = torch.rand(m.running_var.shape, generator=g) + 0.5
    return net


def _net_inputs(seed, N, H, W):
    g = torch.Generator().manual_seed(seed + 2)
    return torch.randn(N, 16, H, W, generator=g), torch.randn(N, 6, H, W, generator=g)


def _ref_grads(sd, num_down, x, lw, bn_train, dtype):
    ref = ub.UnetRef(sd, num_down, dtype=dtype, prefix='net.')
    xx = x.to(dtype).clone().requires_grad_()
    (ref.forward(xx, bn_train) * lw.to(dtype)).sum().backward()
    return xx.grad, {k: p.grad for k, p in ref.p.items()}, ref.min_abs_preact


def _hip_grads(net, x, lw, bn_train, input_grad=True):
    """One forward / backward of the opted-in module on the device -> (gradient of x or None, {state-dict key: gradient}) on the
    CPU; parameter gradients are cleared first."""
    net.train(bn_train)
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout2d):
            m.eval()
    net.zero_grad(set_to_none=True)
    dx = x.to(DEV)
    if input_grad:
        dx.requires_grad_()
    (net(dx, None) * lw.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    sdv = net.net.state_dict(keep_vars=True)
    return (dx.grad.cpu() if input_grad else None), {k: v.grad.cpu() for k, v in sdv.items() if v.grad is not None}


def _assert_ratios(gx, gp, gx64, gp64, gx32, gp32, limit):
    """Per tensor e_hip / max(e_t32, 2^-23) <= limit -> the worst ratio."""
    worst = 0.0
    rows = [('input', gx, gx64, gx32)] + [(k, gp.get(k), gp64[k], gp32[k]) for k in sorted(gp64)]
    for name, got, r64, r32 in rows:
        assert got is not None, name
        e_hip, e_t32 = ub.rel_rms(got, r64), ub.rel_rms(r32, r64)
        ratio = e_hip / max(e_t32, 2.0 ** -23)
        worst = max(worst, ratio)
        assert ratio <= limit, (name, e_hip, e_t32)
    return worst


NET_CASES = [(4, 2, 2, 32, 32, True), (4, 5, 2, 32, 32, True), (4, 2, 1, 64, 32, True), (4, 5, 1, 64, 32, True),
             (4, 2, 2, 32, 32, False), (4, 5, 2, 32, 32, False)] + sorted(WIDE_NET_SEEDS)


@pytest.mark.parametrize('nf0,num_down,N,H,W,bn_train', NET_CASES,
                         ids=['-'.join(str(v) for v in c[1:]) if c[0] == 4 else 'nf%d-' % c[0] + '-'.join(str(v) for v in c[1:])
                              for c in NET_CASES])
def test_whole_network_vs_float64_and_float32_autograd(nf0, num_down, N, H, W, bn_train):
    wide = nf0 != 4
    seed = WIDE_NET_SEEDS[(nf0, num_down, N, H, W, bn_train)] if wide else NET_SEEDS[(num_down, N, H, W, bn_train)]
    net = _make_net(num_down, seed, nf0=nf0)
    x, lw = _net_inputs(seed, N, H, W)
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    gx64, gp64, min_v = _ref_grads(sd, num_down, x, lw, bn_train, torch.float64)
    assert min_v >= 2e-5, 'seed %d: a pre-activation of the oracle lies at %.2e from its kink' % (seed, min_v)
    gx32, gp32, _ = _ref_grads(sd, num_down, x, lw, bn_train, torch.float32)

    net = net.to(DEV).enable_hip_backward()
    gx, gp = _hip_grads(net, x, lw, bn_train)
    worst = _assert_ratios(gx, gp, gx64, gp64, gx32, gp32, RATIO_WIDE if wide else RATIO)
    print('whole network %s%s: worst e_hip / max(e_t32, 2^-23) = %.3f'
          % ('nf0 %d ' % nf0 if wide else '', (num_down, N, H, W, bn_train), worst))


def test_frozen_input_leaves_the_parameter_gradients_bitwise():
    """UNetPlan.backward(want_input_grad=False) skips the data gradient of the first layer and nothing else: the same net and data
    with and without x.requires_grad_() give every parameter gradient the same bits."""
    key = (2, 2, 32, 32, True)
    net = _make_net(2, NET_SEEDS[key]).to(DEV).enable_hip_backward()
    x, lw = _net_inputs(NET_SEEDS[key], 2, 32, 32)
    gx, with_x = _hip_grads(net, x, lw, True)
    none, frozen = _hip_grads(net, x, lw, True, input_grad=False)
    assert gx is not None and torch.isfinite(gx).all() and none is None
    assert set(frozen) == set(with_x) and len(frozen) >= 20
    for k in sorted(with_x):
        assert torch.equal(frozen[k].view(torch.int32), with_x[k].view(torch.int32)), k


def test_fewer_views_than_the_plan_holds():
    """The ordinary last batch: one module runs a training step at N = 2, then one at N = 1 on the SAME plan (built for two
    views).  The N = 1 gradients meet the float64 condition of a fresh N = 1 run (the case (2, 1, 64, 32, True) and its seed)."""
    key = (2, 1, 64, 32, True)
    seed = NET_SEEDS[key]
    net = _make_net(2, seed)
    x, lw = _net_inputs(seed, 1, 64, 32)
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    gx64, gp64, min_v = _ref_grads(sd, 2, x, lw, True, torch.float64)
    assert min_v >= 2e-5, 'seed %d: a pre-activation of the oracle lies at %.2e from its kink' % (seed, min_v)
    gx32, gp32, _ = _ref_grads(sd, 2, x, lw, True, torch.float32)
    net = net.to(DEV).enable_hip_backward()
    x2, lw2 = _net_inputs(seed + 100, 2, 64, 32)
    _hip_grads(net, x2, lw2, True)
    plans = [v for k, v in net.net._plans.items() if len(k) == 5]
    assert len(plans) == 1 and plans[0].N == 2
    gx, gp = _hip_grads(net, x, lw, True)
    now = [v for k, v in net.net._plans.items() if len(k) == 5]
    assert len(now) == 1 and now[0] is plans[0] and now[0].N == 2, 'the training plan was rebuilt for the smaller batch'
    assert tuple(gx.shape) == (1, 16, 64, 32)
    worst = _assert_ratios(gx, gp, gx64, gp64, gx32, gp32, RATIO)
    print('whole network (2, 1, 64, 32, True) on a plan for two views: worst e_hip / max(e_t32, 2^-23) = %.3f' % worst)


def test_dead_parameters_get_no_gradient():
    """use_gcn=True adds the `fuse` block, which never reaches the output."""
    net = _make_net(2, 11, use_gcn=True).to(DEV).enable_hip_backward()
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout2d):
            m.eval()
    x = torch.randn(1, 16, 32, 32, device=DEV)
    net(x, None).sum().backward()
    fuse = [k for k, p in net.named_parameters() if '.fuse.' in k]
    assert fuse
    for k, p in net.named_parameters():
        assert (p.grad is None) == ('.fuse.' in k), k


# ------------------------------------------------------------------------------------------------
# 6. inference untouched
# ------------------------------------------------------------------------------------------------
def test_inference_is_untouched_by_a_training_plan():
    net = _make_net(2, 21).to(DEV)
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout2d):
            m.eval()
    x = torch.randn(2, 16, 32, 32, device=DEV)
    with torch.no_grad():
        before = net(x, None).clone()
    net.enable_hip_backward()
    net(x, None).sum().backward()               # builds and runs a training plan on the same weights (no optimiser step)
    assert any(len(k) == 5 for k in net.net._plans)
    net.enable_hip_backward(False)
    with torch.no_grad():
        after = net(x, None)
    assert torch.equal(before, after)
    with pytest.raises(NotImplementedError, match='inference-only'):
        net(x.clone().requires_grad_(), None)


# ------------------------------------------------------------------------------------------------
# 5. end to end: texture mapper -> RenderingNet -> ray renderer, one loss, one backward()
# ------------------------------------------------------------------------------------------------
def test_image_loss_trains_texture_features_unet_and_lighting():
    """The graph of train_rnr.py at 1 x 64 x 64: TextureMapper(32, 16, 4) -> opted-in RenderingNet (rays_lt of 8 rays) ->
    RayRenderer under LightingSH.  One backward reaches the FEATURE channels (>= 6) of every texture level — without the U-Net
    backward only the albedo channels 0..5 get a gradient —, every live U-Net parameter and LightingSH.coeff; ten Adam steps lower
    the L1 loss against a fixed target, on ONE plan object (weights repacked in place)."""
    import numpy as np

    import network
    import texture_bwd_ref as tb
    from test_gpu_shade_sweep import _renderer_inputs
    from texture_bwd_ref import T
    N, H, W, R, nd = 1, 64, 64, 8, 3
    rng = np.random.default_rng(5)
    torch.manual_seed(5)
    tm = network.TextureMapper(32, 16, 4, apply_sh=True)
    for l, p in enumerate(tm.textures):
        p.data.copy_(T((0.2 + 0.8 * rng.random(tuple(p.shape))).astype(np.float32)) * (1.0 if l == 0 else 0.1))
    tm = tm.to(DEV)
    net = network.RenderingNet(nf0=4, in_channels=16, out_channels=3 * R, num_down_unet=2, use_gcn=False).to(DEV).enable_hip_backward()
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout2d):
            m.eval()
    l_dir = T(rng.standard_normal((3, 50)).astype(np.float32))
    l_dir = l_dir / l_dir.norm(dim=0, keepdim=True)
    coeff0 = T((rng.standard_normal((9, 3)) * 0.3 + 0.2).astype(np.float32))
    lighting = network.LightingSH(l_dir, lmax=2, init_coeff=coeff0, fix_params=False, lp_recon_h=16, lp_recon_w=32).to(DEV)
    rr = network.RayRenderer(lighting, network.Interpolater())
    uv, sh, _ = tb.seam_scene(51, N, H, W, 16)
    rays_uv = T(_renderer_inputs(rng, 3, R, N, H, W, 1, lp_hw=(16, 32))[0]).to(DEV)
    d_uv, d_sh = uv.to(DEV), sh.to(DEV)
    target = torch.rand(N, 3, H, W, generator=torch.Generator().manual_seed(6)).to(DEV)

    def loss_fn():
        neural = tm(d_uv, d_sh, sh_start_ch=6)
        y = net(neural, None)
        rays_lt = ((y * 0.5 + 0.5) * 2).reshape(N, R, 3, H, W)
        out = rr(neural[:, 3:6], rays_uv, rays_lt, lighting_idx=0, albedo_diffuse=neural[:, :3], num_ray_diffuse=nd,
                 seperate_albedo=True)[0]
        return (out - target).abs().mean()

    loss0 = loss_fn()
    loss0.backward()
    for l, p in enumerate(tm.textures):
        assert p.grad is not None and float(p.grad[..., 6:].abs().max()) > 0, 'no gradient on the feature channels of level %d' % l
        assert float(p.grad[..., :6].abs().max()) > 0
    for k, p in net.net._live_params():
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0, k
    assert lighting.coeff.grad is not None and float(lighting.coeff.grad.abs().max()) > 0
    plans = [v for k, v in net.net._plans.items() if len(k) == 5]
    assert len(plans) == 1
    params = list(tm.parameters()) + [p for p in net.parameters() if p.grad is not None] + [lighting.coeff]
    opt = torch.optim.Adam(params, lr=2e-3)
    losses = [float(loss0.detach())]
    for _ in range(10):
        opt.step()
        opt.zero_grad()
        loss = loss_fn()
        loss.backward()
        losses.append(float(loss.detach()))
    print('end to end: L1 loss %.5f -> %.5f over ten Adam steps' % (losses[0], losses[-1]))
    assert losses[-1] < losses[0], losses
    now = [v for k, v in net.net._plans.items() if len(k) == 5]
    assert len(now) == 1 and now[0] is plans[0], 'the training plan was rebuilt between steps'
