"""-m gpu: train-mode Dropout2d on the HIP training path of the U-Net (csrc/dropout.hip, rnr_conv_out_backward_dropout,
UNetPlan(training=True, dropout=...), Unet._forward_train) against tests/unet_dropout_ref.py: the draw bit for bit, the two new
entry points bit for bit, the out-layer backward under the bounds of tests/test_gpu_unet_backward.py with magnitudes scaled by the
multipliers, and the whole network against float64 / float32 torch autograd that apply the HIP draw's own masks.

Whole-network criterion: per tensor e_hip / max(e_t32, 2^-23) <= 8 (the derived bound, RATIO_WIDE of test_gpu_unet_backward.py;
the tightened RATIO was measured without dropout and is not assumed here).  Measured: profiles/unet_backward_accuracy.txt.
Every case asserts the three conditions its seed was found under on the CPU: no pre-activation of the float64 oracle with |v| <
2e-5, every view of every dropped layer keeps a channel, every dropped layer with 8 or more (view, channel) entries drops one."""

import numpy as np
import pytest
import torch

import test_gpu_unet_backward as tb
import unet_bwd_ref as ub
import unet_dropout_ref as ud
from oracle import unet_bwd_cases as uc
from unet_bwd_ref import EPS

pytestmark = pytest.mark.gpu
DEV = tb.DEV
D = torch.float64
LIMIT = tb.RATIO_WIDE
P_ALL = 0.3


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------
# 1. rnr_dropout_draw
# ------------------------------------------------------------------------------------------------
DRAW_LAYERS = [(7, 16, 0.1), (4, 16, 0.5), (64, 64, 0.0), (130, 144, 0.3), (512, 512, 1.0)]
DRAW_SEED = 0x9E3779B97F4A7C15
DRAW_OFFSET = 2 ** 32 - 8


def _i64(v):
    return ((int(v) + (1 << 63)) % (1 << 64)) - (1 << 63)


def _draw(layers, rows, num_views, seed, offset, expect_error=None):
    """rnr_dropout_draw into NaN-filled [rows, c_pad] tables -> the tables on the CPU."""
    from rnr_amd import _lib, ops
    L = tb._L()
    bufs = [torch.full((rows, c_pad), float('nan'), dtype=torch.float32, device=DEV) for _, c_pad, _ in layers]
    arr = (_lib.RnrDropoutLayer * len(layers))(*[_lib.RnrDropoutLayer(b.data_ptr(), c, c_pad, p)
                                                 for b, (c, c_pad, p) in zip(bufs, layers)])
    rc = L.rnr_dropout_draw(arr, len(layers), num_views, _i64(seed), _i64(offset), ops._stream())
    torch.cuda.synchronize()
    if expect_error is not None:
        assert rc != 0
        with pytest.raises(_lib.RnrError, match=expect_error):
            _lib.check(rc)
    else:
        _lib.check(rc)
    return [b.cpu() for b in bufs]


@pytest.mark.parametrize('num_views', [2, 3])
def test_dropout_draw_equals_the_restatement(num_views):
    want = ud.draw(DRAW_LAYERS, num_views, DRAW_SEED, DRAW_OFFSET)
    runs = [_draw(DRAW_LAYERS, 3, num_views, DRAW_SEED, DRAW_OFFSET) for _ in range(2)]
    for got, again, ref, (c, c_pad, p) in zip(runs[0], runs[1], want, DRAW_LAYERS):
        assert _same_bits(got, again), 'two runs differ'
        assert _same_bits(got[:num_views], torch.from_numpy(ref)), (c, c_pad, p)
        assert torch.isnan(got[num_views:]).all(), 'rows >= num_views were written'
        assert (got[:num_views, c:] == 0).all(), 'padding channels must be 0'
        if p == 0.0:
            assert (got[:num_views, :c] == 1).all()
        if p == 1.0:
            assert (got[:num_views] == 0).all()
    mixed = runs[0][3][:num_views, :130]
    assert (mixed == 0).any() and (mixed > 0).any()


@pytest.mark.parametrize('layers,why', [([(4, 16, 0.5)] * 33, 'at most 32'), ([(4, 16, 1.5)], r'outside \[0, 1\]'),
                                        ([(4, 16, -0.1)], r'outside \[0, 1\]'), ([(4, 24, 0.5)], 'multiple of 16')],
                         ids=['33-layers', 'p-above-1', 'p-below-0', 'c_pad-24'])
def test_dropout_draw_refuses_before_any_launch(layers, why):
    got = _draw(layers, 2, 2, 1, 0, expect_error=why)
    assert all(torch.isnan(b).all() for b in got), 'a refused call wrote something'


# ------------------------------------------------------------------------------------------------
# 2. rnr_dropout_affine
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('form', ['scale-null', 'shift-null', 'both', 'in-place'])
def test_dropout_affine_is_the_float32_product(form):
    from rnr_amd import _lib, ops
    L = tb._L()
    rows, n, c_pad = 3, 2, 144
    g = torch.Generator().manual_seed(17)
    scale, shift = torch.randn(rows, c_pad, generator=g), torch.randn(rows, c_pad, generator=g)
    mult = torch.from_numpy(ud.draw([(130, c_pad, 0.3)], rows, 5, 0)[0])
    d_scale = None if form == 'scale-null' else scale.to(DEV)
    d_shift = None if form == 'shift-null' else shift.to(DEV)
    want_sc = mult if d_scale is None else mult * scale         # one float32 product on the CPU
    want_sh = torch.zeros_like(mult) if d_shift is None else mult * shift
    if form == 'in-place':
        o_sc, o_sh = d_scale, d_shift
        keep_sc, keep_sh = scale, shift
    else:
        o_sc = torch.full((rows, c_pad), float('nan'), device=DEV)
        o_sh = torch.full((rows, c_pad), float('nan'), device=DEV)
        keep_sc = keep_sh = torch.full((rows, c_pad), float('nan'))
    _lib.check(L.rnr_dropout_affine(ops._ptr(d_scale), ops._ptr(d_shift), ops._ptr(mult.to(DEV)), ops._ptr(o_sc), ops._ptr(o_sh),
                                    n, c_pad, ops._stream()))
    torch.cuda.synchronize()
    assert _same_bits(o_sc[:n], want_sc[:n]) and _same_bits(o_sh[:n], want_sh[:n])
    assert _same_bits(o_sc[n:], keep_sc[n:]) and _same_bits(o_sh[n:], keep_sh[n:]), 'rows >= num_views were touched'
    if form == 'both':
        assert _same_bits(d_scale, scale) and _same_bits(d_shift, shift), 'an input was written'


# ------------------------------------------------------------------------------------------------
# 3. rnr_conv_out_backward_dropout
# ------------------------------------------------------------------------------------------------
def _call_out_backward(L, entry, y, sc, sh, mult, act, g0, g1, gamma, saved, mode, N, h, w, c, c_pad):
    """Two runs from NaN-filled outputs -> [(g_y, g_gamma, g_beta)] on the CPU.  entry 'plain': rnr_conv_out_backward."""
    from rnr_amd import ops
    ws = torch.empty(L.rnr_conv_out_backward_workspace_bytes(N, h, w, c_pad), dtype=torch.uint8, device=DEV)
    runs = []
    for _ in range(2):
        o_gy = torch.full((N, h, w, c_pad), float('nan'), dtype=torch.float32, device=DEV)
        o_gg = torch.full((c,), float('nan'), dtype=torch.float32, device=DEV)
        o_gb = torch.full((c,), float('nan'), dtype=torch.float32, device=DEV)
        tail = (ops._ptr(gamma), ops._ptr(saved), mode, ops._ptr(o_gy), ops._ptr(o_gg), ops._ptr(o_gb), N, h, w, c, c_pad,
                ops._ptr(ws), ws.numel(), ops._stream())
        if entry == 'plain':
            tb._check(L.rnr_conv_out_backward(ops._ptr(y), ops._ptr(sc), ops._ptr(sh), act, ops._ptr(g0), ops._ptr(g1), *tail))
        else:
            tb._check(L.rnr_conv_out_backward_dropout(ops._ptr(y), ops._ptr(sc), ops._ptr(sh), ops._ptr(mult), act, ops._ptr(g0),
                                                      ops._ptr(g1), *tail))
        torch.cuda.synchronize()
        runs.append((o_gy.cpu(), o_gg.cpu(), o_gb.cpu()))
    return runs


def _device_case(case, c_pad, two, bn):
    y, gz0, gz1, gamma, saved, scale, shift = case[:7]
    return (tb._nhwc(y, c_pad), tb._padc(scale, c_pad) if scale is not None else None, tb._padc(shift, c_pad),
            tb._nhwc(gz0, c_pad), tb._nhwc(gz1, c_pad) if two else None, gamma.to(DEV) if bn else None,
            saved.to(DEV) if bn else None)


def test_conv_out_backward_dropout_without_mult_is_conv_out_backward():
    """mult = NULL over the grid of test_conv_out_backward (act x one / two consumers x three modes x BatchNorm or bias), N = 3,
    5 x 7, 7 channels: every output has rnr_conv_out_backward's bits."""
    L = tb._L()
    N, h, w, c, c_pad = 3, 5, 7, 7, 16
    g = torch.Generator().manual_seed(5 * 31 + 7)
    for act, two, mode, bn in uc.OB_GRID:
        case, _ = tb._out_backward_find(g, N, h, w, c, c_pad, mode, bn, two)
        d_y, d_sc, d_sh, d_g0, d_g1, d_gamma, d_saved = _device_case(case, c_pad, two, bn)
        args = (act, d_g0, d_g1, d_gamma, d_saved, mode, N, h, w, c, c_pad)
        plain = _call_out_backward(L, 'plain', d_y, d_sc, d_sh, None, *args)[0]
        new = _call_out_backward(L, 'dropout', d_y, d_sc, d_sh, None, *args)[0]
        for a, b, name in zip(plain, new, ('g_y', 'g_gamma', 'g_beta')):
            assert _same_bits(a, b), (name, act, two, mode, bn)


def _ob_mask(g, N, c, p):
    """keep [N, c]: random, channel 0 kept in view 0 and dropped in view 1, channel 1 dropped in every view -> float32 mult."""
    keep = torch.rand(N, c, generator=g) >= p
    keep[0, 0], keep[1, 0] = True, False
    keep[:, 1] = False
    if c > 3:
        keep[:, 3] = True
    return keep, keep.float() * float(ud.keep_scale(p))


def _out_backward_dropout_case(L, g, N, h, w, c, mode, act, bn, two, c_pad):
    """tb._out_backward_case's float64 formulas on g_v * mult, its bounds with magnitudes scaled by mult -> worst error / bound."""
    case, _ = tb._out_backward_find(g, N, h, w, c, c_pad, mode, bn, two)
    y, gz0, gz1, gamma, saved, scale, shift, mu, r, v = case
    assert float(v.abs().min()) > 1e-4, 'a pre-activation too close to the kink'
    keep, mult = _ob_mask(g, N, c, 0.3)
    m64 = mult.double()[:, :, None, None]
    y64 = y.double()
    slope = {0: 1.0, 1: 0.2, 2: 0.0}[act]
    gz = (gz0 + gz1) if two else gz0
    # v' = mult v has v's sign where mult > 0; where mult = 0 the factor is irrelevant (g_v = 0)
    d_act = torch.where(v > 0, 1.0, slope)
    gv = gz.double() * d_act * m64
    gv_mag = ((gz0.double().abs() + gz1.double().abs()) if two else gz0.double().abs()) * d_act * m64
    if bn and mode != 2:
        grp = (2, 3) if mode == 0 else (0, 2, 3)
        m = h * w if mode == 0 else N * h * w
        mu_b, r_b = mu[:, :, None, None], r[:, :, None, None]
        S1 = gv.sum(grp, keepdim=True)
        Dm = (gv * (y64 - mu_b) * r_b).sum(grp, keepdim=True)
        ga = gamma.double()[None, :, None, None]
        ref_gy = ga * r_b * (gv - S1 / m - (y64 - mu_b) * r_b * Dm / m)
        mag_gy = (ga * r_b).abs() * (gv_mag + S1.abs() / m + ((y64 - mu_b) * r_b * Dm / m).abs())
        ref_gg, mag_gg = Dm.sum((0, 2, 3)), (gv_mag * ((y64 - mu_b) * r_b).abs()).sum((0, 2, 3))
    elif bn:
        a = (gamma.double()[None] * r)[:, :, None, None]           # gamma r from `saved`: scale holds mult
        ref_gy, mag_gy = a * gv, a.abs() * gv_mag
        t = (y64 - mu[:, :, None, None]) * r[:, :, None, None]
        ref_gg, mag_gg = (gv * t).sum((0, 2, 3)), (gv_mag * t.abs()).sum((0, 2, 3))
    else:
        ref_gy, mag_gy, ref_gg, mag_gg = gv, gv_mag, None, None
    ref_gb, mag_gb = gv.sum((0, 2, 3)), gv_mag.sum((0, 2, 3))

    # the tables the consumers applied: one float32 product each, as rnr_dropout_affine forms them
    sc_d = mult * scale if scale is not None else mult
    sh_d = mult * shift
    d_y, _, _, d_g0, d_g1, d_gamma, d_saved = _device_case(case, c_pad, two, bn)
    runs = _call_out_backward(L, 'dropout', d_y, tb._padc(sc_d, c_pad), tb._padc(sh_d, c_pad), tb._padc(mult, c_pad), act, d_g0,
                              d_g1, d_gamma, d_saved, mode, N, h, w, c, c_pad)
    for a, b in zip(runs[0], runs[1]):
        assert _same_bits(a, b), 'two runs differ'
    o_gy, o_gg, o_gb = runs[0]
    tag = 'mode %d act %d bn %d two %d' % (mode, act, bn, two)
    assert (o_gy[..., c:] == 0).all(), 'padding channels must be 0'
    assert (o_gy[..., 1] == 0).all() and o_gb[1] == 0, (tag, 'the channel dropped in every view')
    if not (bn and mode == 1):          # (whole-batch statistics couple the views: S1 and D of channel 0 come from view 0 too)
        assert (o_gy[1, :, :, 0] == 0).all(), (tag, 'channel 0 is dropped in view 1')
    gy = tb._nchw(o_gy, c).double()
    e = (gy - ref_gy).abs()
    worst = [float((e / (16 * EPS * mag_gy).clamp_min(1e-300)).max()), 0.0, 0.0]
    assert (e <= 16 * EPS * mag_gy).all(), (tag, worst[0])
    e = (o_gb.double() - ref_gb).abs()
    worst[1] = float((e / (4 * EPS * mag_gb).clamp_min(1e-300)).max())
    assert (e <= 4 * EPS * mag_gb).all(), (tag, 'g_beta', worst[1])
    if bn:
        assert o_gg[1] == 0, (tag, 'g_gamma of the channel dropped in every view')
        e = (o_gg.double() - ref_gg).abs()
        worst[2] = float((e / (4 * EPS * mag_gg).clamp_min(1e-300)).max())
        assert (e <= 4 * EPS * mag_gg).all(), (tag, 'g_gamma', worst[2])
    else:
        assert torch.isnan(o_gg).all(), 'g_gamma must not be written without BatchNorm'
    return worst


OB_LIMIT_CASE = next(c for c in uc.OB_CASES if c['c_pad'] == uc.OB_MAX_CPAD)
OB_DROPOUT_SHAPES = [(3, 5, 7, 7, 16), (3, 16, 16, 7, 16),
                     (OB_LIMIT_CASE['N'], OB_LIMIT_CASE['h'], OB_LIMIT_CASE['w'], OB_LIMIT_CASE['c'], OB_LIMIT_CASE['c_pad'])]


@pytest.mark.parametrize('N,h,w,c,c_pad', OB_DROPOUT_SHAPES, ids=lambda v: str(v))
def test_conv_out_backward_dropout(N, h, w, c, c_pad):
    L = tb._L()
    g = torch.Generator().manual_seed(c_pad * 131 + h * 31 + w + 1)
    worst = [0.0, 0.0, 0.0]
    for act, two, mode, bn in uc.OB_GRID:
        got = _out_backward_dropout_case(L, g, N, h, w, c, mode, act, bn, two, c_pad)
        worst = [max(a, b) for a, b in zip(worst, got)]
    print('conv_out_backward_dropout %s: worst error / bound g_y %.3f, g_beta %.3f, g_gamma %.3f' % ((N, h, w, c, c_pad), *worst))


# ------------------------------------------------------------------------------------------------
# 4. whole network
# ------------------------------------------------------------------------------------------------
# (nf0, num_down, N, H, W, BatchNorm train mode) -> seed of the network, the inputs and the masks, found on the CPU
NET_SEEDS = {(4, 2, 2, 32, 32, True): 33, (4, 5, 2, 32, 32, True): 1, (4, 5, 2, 32, 32, False): 14, (4, 2, 1, 64, 32, True): 4,
             (64, 3, 2, 8, 8, True): 8}
MIXED_SEED = 1          # test_mixed_dropout_settings: found the same way, first try
BATCH_SEED = 72         # test_bare_plan_in_batch_mode_with_given_masks: the oracle runs view by view; 72 tries


def _dropouts(net):
    return net.net._step_dropouts()[:-1]


def _set_modes(net, bn_train, p=P_ALL):
    """BatchNorm in `bn_train` mode, every Dropout2d live with probability p."""
    net.train(bn_train)
    for m in _dropouts(net):
        m.train()
        m.p = p
    return net


def _probs(net):
    return [float(m.p) if m.training else 0.0 for m in _dropouts(net)]


def check_masks(mults, layers):
    """The two mask conditions of a case."""
    for k, (m, (c, c_pad, p)) in enumerate(zip(mults, layers)):
        keep = np.asarray(m)[:, :c] > 0
        if p < 1.0:
            assert keep.any(1).all(), 'layer %d: a view keeps no channel' % k
        if p > 0.0 and keep.size >= 8:
            assert not keep.all(), 'layer %d drops nothing' % k


def _ref_grads(sd, num_down, x, lw, bn_train, dtype, mults):
    ref = ud.UnetDropoutRef(sd, num_down, mults, dtype=dtype, prefix='net.')
    xx = x.to(dtype).clone().requires_grad_()
    out = ref.forward(xx, bn_train)
    (out * lw.to(dtype)).sum().backward()
    return out.detach(), xx.grad, {k: p.grad for k, p in ref.p.items()}, ref.min_abs_preact


def references(net, nf0, num_down, x, lw, bn_train, seed, offset=0):
    """The restatement's masks for this network at (seed, offset), checked, and the float64 / float32 references under them."""
    layers = ud.unet_layers(nf0, num_down, _probs(net))
    mults = ud.draw(layers, x.shape[0], seed, offset)
    check_masks(mults, layers)
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    r64 = _ref_grads(sd, num_down, x, lw, bn_train, torch.float64, mults)
    assert r64[3] >= 2e-5, 'seed %d: a pre-activation of the oracle lies at %.2e from its kink' % (seed, r64[3])
    r32 = _ref_grads(sd, num_down, x, lw, bn_train, torch.float32, mults)
    return layers, mults, r64, r32


def _live_plan(net):
    plan, = [p for p in net.net._plans.values() if p.training and p.dropout_live]
    return plan


def _step(net, x, lw, seed=None):
    """One forward / backward of the opted-in module as its modes stand -> (output, gradient of x, {key: gradient}) on the CPU."""
    net.zero_grad(set_to_none=True)
    dx = x.to(DEV).requires_grad_()
    dlw = lw.to(DEV)
    if seed is not None:
        torch.cuda.manual_seed(seed)
    out = net(dx, None)
    (out * dlw).sum().backward()
    torch.cuda.synchronize()
    sdv = net.net.state_dict(keep_vars=True)
    return out.detach().cpu(), dx.grad.cpu(), {k: v.grad.cpu() for k, v in sdv.items() if v.grad is not None}


def _assert_keep(plan, mults, layers):
    keeps = plan.dropout_keep()
    assert len(keeps) == len(layers)
    for k, (got, m, (c, c_pad, p)) in enumerate(zip(keeps, mults, layers)):
        assert torch.equal(got.cpu(), torch.from_numpy(np.asarray(m)[:, :c] > 0)), 'layer %d: masks differ from the restatement' % k


def _ratios(out, gx, gp, r64, r32, limit=LIMIT):
    o64, gx64, gp64, _ = r64
    o32, gx32, gp32, _ = r32
    e_hip, e_t32 = ub.rel_rms(out, o64), ub.rel_rms(o32, o64)
    r_out = e_hip / max(e_t32, 2.0 ** -23)
    assert r_out <= limit, ('output', e_hip, e_t32)
    return max(r_out, tb._assert_ratios(gx, gp, gx64, gp64, gx32, gp32, limit))


@pytest.mark.parametrize('nf0,num_down,N,H,W,bn_train', sorted(NET_SEEDS), ids=lambda v: str(v))
def test_whole_network_with_live_dropout(nf0, num_down, N, H, W, bn_train):
    seed = NET_SEEDS[(nf0, num_down, N, H, W, bn_train)]
    net = _set_modes(tb._make_net(num_down, seed, nf0=nf0), bn_train)
    x, lw = tb._net_inputs(seed, N, H, W)
    layers, mults, r64, r32 = references(net, nf0, num_down, x, lw, bn_train, seed)
    net = net.to(DEV).enable_hip_backward()
    out, gx, gp = _step(net, x, lw, seed)
    _assert_keep(_live_plan(net), mults, layers)
    worst = _ratios(out, gx, gp, r64, r32)
    print('whole network, Dropout2d p = %.1f live %s: worst e_hip / max(e_t32, 2^-23) = %.3f'
          % (P_ALL, (nf0, num_down, N, H, W, bn_train), worst))


def test_plan_sized_for_three_views_runs_two():
    """The masks of a 2-view call do not depend on the plan's size: a 3-view call sizes the plan, the 2-view call that follows
    draws the 2-view restatement's tables and meets the whole-network criterion."""
    key = (4, 2, 2, 32, 32, True)
    seed = NET_SEEDS[key]
    net = _set_modes(tb._make_net(2, seed), True)
    x, lw = tb._net_inputs(seed, 2, 32, 32)
    layers, mults, r64, r32 = references(net, 4, 2, x, lw, True, seed)
    net = net.to(DEV).enable_hip_backward()
    x3, lw3 = tb._net_inputs(seed + 100, 3, 32, 32)
    _step(net, x3, lw3, seed + 100)
    plan = _live_plan(net)
    assert plan.N == 3
    out, gx, gp = _step(net, x, lw, seed)
    assert _live_plan(net) is plan and plan.N == 3, 'the plan was rebuilt for the smaller batch'
    _assert_keep(plan, mults, layers)
    worst = _ratios(out, gx, gp, r64, r32)
    print('whole network with live dropout, two views on a plan for three: worst ratio %.3f' % worst)


def _mixed_modes(net):
    """in_layer's module at p = 0.5, one UpBlock module in eval mode, one at p = 0, the rest at 0.3."""
    _set_modes(net, True)
    mods = _dropouts(net)
    up = [m for m in net.net.unet_block.up.net if isinstance(m, torch.nn.Dropout2d)]
    sub_up = [m for m in net.net.unet_block.submodule.up.net if isinstance(m, torch.nn.Dropout2d)]
    mods[0].p = 0.5
    up[0].eval()
    sub_up[1].p = 0.0
    return [mods.index(up[0]), mods.index(sub_up[1])]


def test_mixed_dropout_settings():
    seed, nd = MIXED_SEED, 5
    net = tb._make_net(nd, seed)
    ones = _mixed_modes(net)
    probs = _probs(net)
    assert probs[0] == 0.5 and all(probs[i] == 0.0 for i in ones) and sorted(set(probs)) == [0.0, 0.3, 0.5]
    x, lw = tb._net_inputs(seed, 2, 32, 32)
    layers, mults, r64, r32 = references(net, 4, nd, x, lw, True, seed)
    net = net.to(DEV).enable_hip_backward()
    out, gx, gp = _step(net, x, lw, seed)
    plan = _live_plan(net)
    _assert_keep(plan, mults, layers)
    for i in ones:
        s = plan._dropped[i]
        assert (s['mult'][:2, :s['out'].c] == 1).all(), 'a module in eval mode or at p = 0 multiplies by exactly 1'
    for s, m in zip(plan._dropped, mults):
        assert _same_bits(s['mult'][:2], torch.from_numpy(m)), 'multipliers differ from the restatement'
    worst = _ratios(out, gx, gp, r64, r32)
    print('whole network, mixed dropout settings: worst ratio %.3f' % worst)


def test_bare_plan_in_batch_mode_with_given_masks():
    """bn_mode 'batch' (statistics per view) on a bare UNetPlan with the caller's masks (set_dropout_keep): the reference runs
    view by view, parameter gradients summed."""
    from rnr_amd import ops
    from rnr_amd.testing import channel_last
    from rnr_amd.unet import UNetPlan
    seed, nd, N, H, W = BATCH_SEED, 2, 2, 32, 32
    net = tb._make_net(nd, seed)
    x, lw = tb._net_inputs(seed, N, H, W)
    layers = ud.unet_layers(4, nd, P_ALL)
    mults = ud.draw(layers, N, seed, 0)
    check_masks(mults, layers)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}

    def ref(dtype):
        outs, gxs, gps, min_v = [], [], {}, float('inf')
        for n in range(N):
            o, gx, gp, mv = _ref_grads(sd, nd, x[n:n + 1], lw[n:n + 1], True, dtype, [m[n:n + 1] for m in mults])
            outs.append(o)
            gxs.append(gx)
            min_v = min(min_v, mv)
            for k, v in gp.items():
                gps[k] = gps[k] + v if k in gps else v
        return torch.cat(outs), torch.cat(gxs), gps, min_v
    r64, r32 = ref(torch.float64), ref(torch.float32)
    assert r64[3] >= 2e-5, 'seed %d: a pre-activation of the oracle lies at %.2e from its kink' % (seed, r64[3])

    dsd = {k: v.to(DEV) for k, v in sd.items()}
    plan = UNetPlan(dsd, 16, 6, 4, nd, (H, W), N, DEV, bn_mode='batch', training=True, dropout=[P_ALL] * len(layers) + [None])
    assert plan.dropout_live
    with pytest.raises(RuntimeError, match='never drawn'):
        plan.forward(channel_last(x, plan.in_c_pad).to(DEV))
    plan.set_dropout_keep([torch.from_numpy(m[:, :c] > 0) for m, (c, _, _) in zip(mults, layers)])
    raw = plan.forward(channel_last(x, plan.in_c_pad).to(DEV))
    for s, m in zip(plan._dropped, mults):
        assert _same_bits(s['mult'][:N], torch.from_numpy(m)), 'set_dropout_keep forms the multipliers of the draw'
    out = ops.nhwc_to_nchw(raw, 6, bias=plan.out_bias, apply_tanh=True)
    g_raw = ops.unet_out_backward(lw.to(DEV), out, True, plan.out.c_pad)
    g_in, grads = plan.backward(g_raw)
    torch.cuda.synchronize()
    gx = ops.nhwc_to_nchw(g_in.contiguous(), 16).cpu()
    gp = {k[len('net.'):]: v.cpu() for k, v in grads.items()}
    worst = _ratios(out.cpu(), gx, gp, r64, r32)
    print("bare plan, bn_mode 'batch', given masks: worst ratio %.3f" % worst)


# ------------------------------------------------------------------------------------------------
# 8 - 11. generator semantics, nothing live, bound Adam, the inference plan's refusal
# ------------------------------------------------------------------------------------------------
def test_generator_semantics():
    seed = 33
    net = _set_modes(tb._make_net(2, seed), True).to(DEV).enable_hip_backward()
    x, lw = tb._net_inputs(seed, 2, 32, 32)
    gen = torch.cuda.default_generators[torch.device(DEV).index]
    blocks = 2 * sum(l[1] for l in ud.unet_layers(4, 2, P_ALL)) // 4
    advance = (blocks + 3) // 4 * 4

    torch.cuda.manual_seed(seed)
    saved = torch.cuda.get_rng_state(DEV)
    assert gen.get_offset() == 0
    first = _step(net, x, lw)
    plan = _live_plan(net)
    keep1 = [k.cpu() for k in plan.dropout_keep()]
    assert gen.get_offset() == advance and gen.initial_seed() == seed
    second = _step(net, x, lw)                   # no reseed: the next blocks
    keep2 = [k.cpu() for k in plan.dropout_keep()]
    assert gen.get_offset() == 2 * advance
    assert any(not torch.equal(a, b) for a, b in zip(keep1, keep2)), 'a second step reused the masks'
    want2 = ud.draw(ud.unet_layers(4, 2, P_ALL), 2, seed, advance)
    for k, m, (c, _, _) in zip(keep2, want2, ud.unet_layers(4, 2, P_ALL)):
        assert torch.equal(k, torch.from_numpy(m[:, :c] > 0))
    again = _step(net, x, lw, seed)              # the same seed: the same bits
    assert _same_bits(first[0], again[0]) and _same_bits(first[1], again[1])
    assert set(first[2]) == set(again[2]) and all(_same_bits(first[2][k], again[2][k]) for k in first[2])
    assert not _same_bits(first[0], second[0])
    torch.cuda.set_rng_state(saved, DEV)
    _step(net, x, lw)
    for a, b in zip(keep1, plan.dropout_keep()):
        assert torch.equal(a, b.cpu()), 'set_rng_state did not bring the first tables back'


@pytest.mark.parametrize('how', ['eval', 'p0'])
def test_nothing_live_nothing_changed(how):
    seed = 33
    x, lw = tb._net_inputs(seed, 2, 32, 32)
    base = tb._make_net(2, seed).to(DEV).enable_hip_backward()
    base.train(True)
    for m in _dropouts(base):
        m.eval()
    want = _step(base, x, lw)
    net = tb._make_net(2, seed).to(DEV).enable_hip_backward()
    _set_modes(net, True, p=0.0 if how == 'p0' else P_ALL)
    if how == 'eval':
        for m in _dropouts(net):
            m.eval()
    gen = torch.cuda.default_generators[torch.device(DEV).index]
    torch.cuda.manual_seed(seed)
    got = _step(net, x, lw)
    assert gen.get_offset() == 0, 'a plan that is not live drew from the generator'
    plans = [p for p in net.net._plans.values() if p.training]
    assert len(plans) == 1 and not plans[0].dropout_live and all(len(k) == 5 for k in net.net._plans)
    assert _same_bits(want[0], got[0]) and _same_bits(want[1], got[1])
    assert set(want[2]) == set(got[2]) and all(_same_bits(want[2][k], got[2][k]) for k in want[2])


def test_bound_adam_keeps_a_live_plan_current():
    """nf0 4, num_down 5: the bias-only layers' shift is written by the optimiser's mirrors, and the dropped tables are folded from
    it on the next forward."""
    from rnr_amd.optim import Adam
    seed, nd = 1, 5
    net = _set_modes(tb._make_net(nd, seed), True).to(DEV).enable_hip_backward()
    x, lw = tb._net_inputs(seed, 2, 32, 32)
    opt = Adam(net.parameters(), lr=5e-3).bind(net)
    torch.cuda.manual_seed(seed)
    (net(x.to(DEV), None) * lw.to(DEV)).sum().backward()
    plan = _live_plan(net)
    opt.step()
    torch.cuda.manual_seed(seed)
    got = net(x.to(DEV), None).detach().clone()
    assert _live_plan(net) is plan, 'the bound plan was rebuilt'
    fresh = tb._make_net(nd, seed + 50)
    fresh.load_state_dict(net.state_dict())
    fresh = _set_modes(fresh.to(DEV).enable_hip_backward(), True)
    torch.cuda.manual_seed(seed)
    want = fresh(x.to(DEV), None).detach()
    for a, b in zip(plan.dropout_keep(), _live_plan(fresh).dropout_keep()):
        assert torch.equal(a, b)
    assert _same_bits(got, want)


def test_inference_plan_still_refuses_live_dropout():
    net = _set_modes(tb._make_net(2, 21), True).to(DEV).enable_hip_backward()
    x = torch.randn(1, 16, 32, 32, device=DEV)
    with torch.no_grad(), pytest.raises(NotImplementedError, match='Dropout2d in training mode'):
        net(x, None)
