"""-m gpu: the BatchNorm statistics every convolution path publishes, against oracle/bn64.py (float64) applied to the output
the same launch WROTE — so the statistics are tested on their own, free of the convolution's rounding (which
test_gpu_unet.py bounds against float64 convolutions), and at the benchmark's full layer sizes.

Inputs.  One source per input (two for the skip-concat shapes), scale 1, shift D_n = 1 + n / (2N) per view, activation none,
raw channel 0 all zero (so input channel 0 is the constant D_n).  Weights w0 ~ N(0, 1/fan), centred per output channel, fan =
the taps that reach one output pixel (9 C, 16 C, 4 C), plus an offset R[co] on input channel 0: R / taps on each of its taps
(9, 16), and for the transposed convolution R on the four centre entries, exactly one of which reaches each output pixel.
Output channel co has mean ~ D_n R[co] and std ~ 1, R on the ladder 0, 1, 3, 10, 30, 100, 300, 1000.  Every tenth channel is
exactly constant (weights on input channel 0 only), the next all zero; gamma is 0 or negative on some channels.  The bounds use
the mean / std each channel actually reaches, from the reference.

Tolerances, derived from the arithmetic.  u = 2^-53.  The kernels' s1 = sum v and s2 = sum v^2 of float32 outputs v are
float64 sums of exact terms (v and v^2 are exact in double) along chains of at most k additions: a lane's own outputs
(<= 64), the cross-lane shuffle and LDS combine (<= 14), the float64 atomics of the workgroups of one view into one word
(<= n / 16 for a view of n pixels: the reduce kernel takes 16 rows per workgroup at the least; tiles and the straddling
branch's per-element atomics only occur below that) and the shard sum (8): k = 128 + n / 16.  Hence
  |s1 - S1| <= k u sum|v|,   |s2 - S2| <= k u S2.
The finalise computes var = s2/n - (s1/n)^2: with |mean| sum|v|/n <= S2/n (Cauchy-Schwarz) and the two roundings of the last
subtraction, |var - VAR| <= 4 k u S2/n.  scale = gamma / sqrt(var + eps) rounded once to float32:
  |scale - SCALE| <= |SCALE| (2^-23 + 2 k u (S2/n) / (VAR + eps)),
where 2 k u (S2/n) / VAR ~ 2 k u (1 + r^2) for mean/std r: 2e-11 at r = 30 on a 16 x 16 map, 4e-6 at r = 1000 on 512^2.
shift = beta - mean scale rounded once to float32: |shift - SHIFT| <= 2^-23 (|beta| + |MEAN SCALE|) + |SCALE| k u sqrt(S2/n) + |MEAN SCALE| 2 k u
(S2/n) / (VAR + eps).  A float32 partial sum of 64 outputs has relative error ~2^-24 sqrt(64) ~ 5e-7 in s1 and s2: 10^7 times
the bound, and after the cancellation in var a relative scale error of 1e-4 at mean/std 30 on a 16 x 16 map."""
import ctypes

import numpy as np
import pytest
import torch

from rnr_amd.testing import run_conv, run_conv_fused

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
U = 2.0 ** -53
LADDER = [0.0, 1.0, 3.0, 10.0, 30.0, 100.0, 300.0, 1000.0]
EPS = 1e-5


def pad16(c):
    return (c + 15) // 16 * 16


def chain(n):
    return 128 + n / 16


def make_case(kind, N, H, W, cins, c_out, seed):
    """(srcs for run_conv, weight, gamma, beta) as the module docstring describes."""
    g = torch.Generator().manual_seed(seed)
    D = 1.0 + torch.arange(N, dtype=torch.float32) / (2 * N)
    srcs = []
    for C in cins:
        raw = torch.randn(N, C, H, W, generator=g)
        raw[:, 0] = 0.0
        srcs.append((raw, torch.ones(N, C), D[:, None].expand(N, C).contiguous(), 0))
    cin = sum(cins)
    k = 3 if kind == 0 else 4
    taps = 9 if kind == 0 else (16 if kind == 1 else 4)
    fan = cin * taps
    w = torch.randn(c_out, cin, k, k, generator=g)             # [co, ci, ky, kx]; transposed below for kind 2
    w = (w - w.mean(dim=(1, 2, 3), keepdim=True)) / fan ** 0.5
    # the kernel entries of input channel 0 that carry the offset: all of them under reflection; for the transposed
    # convolution (zero border) the four centre ones, of which every output pixel receives exactly one
    hot = torch.zeros(k, k)
    if kind == 2:
        hot[1:3, 1:3] = 1.0
    else:
        hot[:] = 1.0 / taps
    for co in range(c_out):
        cls = co % 10
        if cls < 8:
            w[co, 0] += LADDER[cls] * hot
        elif cls == 8:                                         # exactly constant: input channel 0 only
            w[co] = 0.0
            w[co, 0] = float(torch.rand(1, generator=g)) * 3.0 * hot
        else:                                                  # all zero
            w[co] = 0.0
    if kind == 2:
        w = w.transpose(0, 1).contiguous()
    gamma = torch.rand(c_out, generator=g) + 0.5
    gamma[3::7] = 0.0
    gamma[2::5] *= -1.0
    beta = torch.randn(c_out, generator=g) * 2.0
    return srcs, w, gamma, beta


def ratios(ref):
    """|mean| / std per channel; 0 for the constant channels"""
    r = ref['mean'].abs() / ref['var'].sqrt().clamp_min(1e-300)
    return torch.where(ref['var'] > 0, r, torch.zeros_like(r))


def assert_sums(stats, out, c_out, what):
    """rnr_conv2d's statistics buffer against the float64 sums over the output it wrote, and the variance derived from them."""
    from oracle import bn64
    ref = bn64.per_view(out, c_out, torch.ones(c_out), torch.zeros(c_out))
    n = ref['count']
    k = chain(n)
    a1 = out[..., :c_out].double().abs().sum(dim=(1, 2))
    s1, s2 = stats[:, :c_out, 0], stats[:, :c_out, 1]
    e1 = ((s1 - ref['s1']).abs() / (k * U * a1).clamp_min(1e-300)).max()
    e2 = ((s2 - ref['s2']).abs() / (k * U * ref['s2']).clamp_min(1e-300)).max()
    var = s2 / n - (s1 / n) ** 2
    ev = ((var - ref['var']).abs() / (4 * k * U * ref['s2'] / n).clamp_min(1e-300)).max()
    rel1 = float(((s1 - ref['s1']).abs() / a1.clamp_min(1e-300)).max())
    assert float(e1) <= 1 and float(e2) <= 1 and float(ev) <= 1, \
        '%s: s1 / s2 / var at %.3g / %.3g / %.3g of the bound (s1 rel. error %.2e, mean/std up to %.0f)' % (
            what, e1, e2, ev, rel1, float(ratios(ref).max()))


def assert_affine(scale, shift, ref, beta, c_out, what):
    """scale / shift [N or 1, c_pad] float32 against bn64's float64 values (per view or batch_all)."""
    n = ref['count']
    k = chain(n)
    ms = ref['s2'] / n
    vterm = 2 * k * U * ms / (ref['var'] + EPS)
    SC, SH = ref['scale'], ref['shift']
    tol_sc = SC.abs() * (2.0 ** -23 + vterm)
    msc = (ref['mean'] * SC).abs()
    tol_sh = 2.0 ** -23 * (beta.double().abs() + msc) + SC.abs() * k * U * ms.sqrt() + msc * vterm
    got_sc, got_sh = scale[..., :c_out].double(), shift[..., :c_out].double()
    esc = (got_sc - SC).abs() / tol_sc.clamp_min(1e-300)
    esh = (got_sh - SH).abs() / tol_sh.clamp_min(1e-300)
    if float(esc.max()) > 1 or float(esh.max()) > 1:
        # the worst relative scale error per rung of the mean/std ladder, for the record
        r = ratios(ref).expand_as(got_sc).flatten()
        rel = ((got_sc - SC).abs() / SC.abs().clamp_min(1e-300)).flatten()
        rungs = []
        for lo, hi in ((0, 2), (2, 6), (6, 20), (20, 60), (60, 200), (200, 600), (600, 3000)):
            sel = (r >= lo) & (r < hi)
            if bool(sel.any()):
                rungs.append('r<%d: %.1e' % (hi, float(rel[sel].max())))
        raise AssertionError('%s: scale / shift at %.3g / %.3g of the bound; worst relative scale error %s' % (
            what, float(esc.max()), float(esh.max()), ', '.join(rungs)))
    cp = scale.shape[-1]
    if cp > c_out:
        assert float(scale[..., c_out:].abs().max()) == 0.0 and float(shift[..., c_out:].abs().max()) == 0.0, what


def assert_running(rm, rv, ref, what):
    """running buffers after one update, 0.9 r + 0.1 stat rounded once to float32, against bn64.batch_all: the statistic's
    own error (|mean - MEAN| <= k u sqrt(S2/n), |var - VAR| <= 4 k u S2/n, times n/(n-1) for the unbiased variance) times 0.1.
    The kernels receive the momentum as a float32, 0.1 + 1.5e-9: that moves each update by 1.5e-9 (|stat| + |old|)."""
    n, k = ref['count'], chain(ref['count'])
    dm = abs(float(np.float32(0.1)) - 0.1)
    unb = ref['var'] * n / (n - 1)
    old_m, old_v = (ref['running_mean'] - 0.1 * ref['mean']) / 0.9, (ref['running_var'] - 0.1 * unb) / 0.9
    tol_m = 2.0 ** -23 * ref['running_mean'].abs() + 0.1 * k * U * (ref['s2'] / n).sqrt() + dm * (ref['mean'].abs() + old_m.abs())
    tol_v = 2.0 ** -23 * ref['running_var'].abs() + 0.1 * 4 * k * U * ref['s2'] / (n - 1) + dm * (unb + old_v.abs()) + 1e-300
    em = float(((rm.cpu().double() - ref['running_mean']).abs() / tol_m).max())
    ev = float(((rv.cpu().double() - ref['running_var']).abs() / tol_v).max())
    assert em <= 1 and ev <= 1, '%s: running_mean / running_var at %.3g / %.3g of the bound' % (what, em, ev)


SWEEP = [
    # kind, N, H, W, [C per source], c_out, flags, algorithm rnr_conv_algorithm reports, split-K depth of the plan    path
    # (maps smaller than a tile are always split here, so their view-straddling statistics come from splitk_reduce_kernel)
    (0, 16, 72, 72, [40], 24, 0, 0, 1),                # conv_mfma_kernel (gather, odd size), single-view tiles
    (0, 4, 200, 200, [16], 24, 0, 0, 1),               # ... non-multiple-of-32 map, 40000 pixels per view
    (0, 2, 24, 24, [40], 24, 0, 0, 6),                 # ... small: split six ways, statistics in splitk_reduce_kernel
    (0, 3, 2, 2, [32], 32, 0, 0, 4),                   # 2 x 2 maps: the reduce kernel's view-straddling branch
    (1, 5, 8, 8, [16], 16, 0, 0, 4),                   # 4x4 stride 2 onto 4 x 4 maps, five views, straddling
    (0, 3, 256, 256, [64], 64, 0, 0, 1),               # conv_halo_kernel 32 pixels wide, per-view tickets
    (1, 4, 256, 256, [32], 64, 0, 0, 1),               # conv_halo_kernel, 4x4 stride 2
    (2, 4, 64, 64, [128], 128, 0, 0, 1),               # transposed, four views
    (2, 16, 64, 64, [128], 128, 0, 0, 1),              # transposed, 16 views
    (0, 16, 16, 16, [16], 16, 0, 0, 1),                # maps 16 pixels wide (two image rows per MFMA row block)
    (0, 256, 16, 16, [16], 32, 0, 0, 1),               # ... 256 views
    (0, 1, 512, 512, [64, 64], 78, 0, 0, 1),           # conv_halo_kernel R16 80-column configuration, skip concat, 512^2
    (0, 2, 128, 128, [64, 64], 78, 0, 0, 4),           # ... split four ways
    (0, 1, 64, 64, [256], 256, 0, 0, 2),               # halo kernel split two ways
    (2, 2, 4, 4, [512], 512, 0, 0, 32),                # 4 x 4 maps, deep split, straddling reduce
    (2, 3, 16, 16, [512], 512, 0, 0, 1),               # the U-Net's layer 12 at three views
    (1, 1, 32, 32, [512], 512, 0, 0, 16),              # layer 11: 4x4 stride 2 onto a 16 x 16 map
    (0, 1, 512, 512, [16], 128, 0, 0, 1),              # 512^2: the 256 x 128 direct configuration
    (0, 3, 256, 256, [64], 64, 'bf16x6', 0, 1),        # conv_halo_emu_kernel, bf16x6
    (0, 3, 256, 256, [64], 64, 'f16x3', 0, 1),         # conv_halo_emu_kernel, f16x3 (partials rescaled by winv)
    (2, 16, 64, 64, [128], 128, 'f16x3', 0, 1),        # f16x3 transposed
    (0, 1, 64, 64, [112], 64, 'f16x3', 0, 7),          # emulation, split
    (0, 2, 16, 16, [512], 512, 'bf16x6', 0, 32),       # emulation, deep split
    (0, 2, 64, 128, [64], 128, 'w', 1, 1),             # conv_wino_kernel F(2x2, 3x3)
    (0, 1, 32, 32, [512], 512, 'w', 1, 4),             # ... split four ways + reduce
    (1, 4, 256, 256, [16], 128, 'w', 2, 1),            # conv_wino2_kernel, stride 2
    (2, 2, 64, 64, [128], 256, 'w', 2, 1),             # conv_wino2p_kernel, transposed
    (2, 16, 16, 16, [512], 512, 'w', 2, 1),            # layer 12 at 16 views
    (0, 4, 64, 64, [112], 78, 'w', 3, 1),              # conv_wino80_kernel
    (0, 1, 512, 512, [64, 64], 78, 'w', 3, 1),         # the out layer at 512^2
    (0, 16, 64, 64, [64], 128, 'w4', 4, 1),            # conv_wino4_kernel unsplit, 16 views
    (0, 1, 64, 64, [512], 512, 'w4', 4, 4),            # conv_wino4_kernel split four ways
    (0, 1, 512, 512, [64], 64, 'w4', 4, 1),            # L2 / L21 at 512^2
]


def _flags(f):
    from rnr_amd import _lib
    if f == 'w':
        return _lib.CONV_WINOGRAD
    if f == 'w4':
        return _lib.CONV_WINOGRAD | _lib.CONV_WINOGRAD4
    return _lib.EMU_FLAGS[f] if f else 0


@pytest.mark.parametrize('kind,N,H,W,cins,c_out,fl,algo,splitk', SWEEP)
def test_bn_statistics_sweep(kind, N, H, W, cins, c_out, fl, algo, splitk):
    """Every path that publishes statistics: rnr_conv2d's caller buffer (s1, s2 and the variance derived from them), then
    rnr_conv2d_fused with BatchNorm twice on one sync buffer (whichever finalise route the plan takes: in-launch tickets per
    view or per launch, bn_finalize_shards_kernel, split-K reduce + finalise), which must leave the sync buffer at zero, then
    rnr_bn_finalize / _reset / _batch (with running buffers) on the first call's statistics.  Bounds: module docstring."""
    from oracle import bn64
    from rnr_amd import _lib
    from rnr_amd.ops import _ptr, _stream
    L = _lib.load()
    flags = _flags(fl)
    desc = _lib.RnrConvDesc(kind, cins[0], pad16(cins[0]), cins[1] if len(cins) > 1 else 0,
                            pad16(cins[1]) if len(cins) > 1 else 0, c_out, pad16(c_out), flags)
    assert L.rnr_conv_algorithm(ctypes.byref(desc), N, H, W) == algo
    oh, ow = (H, W) if kind == 0 else ((H // 2, W // 2) if kind == 1 else (2 * H, 2 * W))
    ws = L.rnr_conv_workspace_bytes(ctypes.byref(desc), N, H, W)       # 256, or the split-K slabs + 256
    assert (1 if ws <= 256 else (ws - 256) // (N * oh * ow * pad16(c_out) * 4)) == splitk
    srcs, w, gamma, beta = make_case(kind, N, H, W, cins, c_out, seed=97 * kind + 13 * N + H + W + c_out)
    tag = '%s/%s' % (fl, algo)
    out, stats = run_conv(kind, srcs, w, c_out, N, H, W, flags=flags)
    assert torch.isfinite(out).all()
    ref = bn64.per_view(out, c_out, gamma, beta, EPS)
    assert float(ratios(ref)[:, 7::10].min()) > 300, 'the ladder must reach mean/std of several hundred'
    assert_sums(stats, out, c_out, 'rnr_conv2d ' + tag)
    out_f, scale, shift, sync = run_conv_fused(kind, srcs, w, c_out, N, H, W, gamma, beta, flags=flags, repeats=2)
    assert torch.equal(out_f.view(torch.int32), out.view(torch.int32)), 'out_raw differs between the two entry points'
    assert int(sync.abs().max()) == 0, 'sync buffer not returned to zero'
    assert_affine(scale, shift, ref, beta, c_out, 'rnr_conv2d_fused ' + tag)
    # the separate finalise kernels on the caller buffer's statistics
    cp = pad16(c_out)
    n = ref['count']
    gd, bd = gamma.to(DEV), beta.to(DEV)
    sc, sh = torch.empty(N, cp, device=DEV), torch.empty(N, cp, device=DEV)
    st = stats.to(DEV)
    _lib.check(L.rnr_bn_finalize(_ptr(st), _ptr(gd), _ptr(bd), _ptr(sc), _ptr(sh), N, c_out, cp, float(n), EPS, _stream()))
    torch.cuda.synchronize()
    assert torch.equal(st.cpu(), stats)
    assert_affine(sc.cpu(), sh.cpu(), ref, beta, c_out, 'rnr_bn_finalize ' + tag)
    _lib.check(L.rnr_bn_finalize_reset(_ptr(st), _ptr(gd), _ptr(bd), _ptr(sc), _ptr(sh), N, c_out, cp, float(n), EPS, _stream()))
    torch.cuda.synchronize()
    assert int((st != 0).sum()) == 0
    assert_affine(sc.cpu(), sh.cpu(), ref, beta, c_out, 'rnr_bn_finalize_reset ' + tag)
    g = torch.Generator().manual_seed(5)
    rm0, rv0 = torch.randn(c_out, generator=g), torch.rand(c_out, generator=g) + 0.1
    rm, rv = rm0.to(DEV), rv0.to(DEV)
    st = stats.to(DEV)
    _lib.check(L.rnr_bn_finalize_batch(_ptr(st), _ptr(gd), _ptr(bd), _ptr(sc), _ptr(sh), _ptr(rm), _ptr(rv), 0.1, N, c_out, cp,
                                       float(n), EPS, _stream()))
    torch.cuda.synchronize()
    assert int((st != 0).sum()) == 0
    refb = bn64.batch_all(out, c_out, gamma, beta, EPS, rm0, rv0, 0.1)
    assert_affine(sc.cpu(), sh.cpu(), refb, beta, c_out, 'rnr_bn_finalize_batch ' + tag)
    assert_running(rm, rv, refb, 'rnr_bn_finalize_batch ' + tag)


def _offset_unet(mode, n, update_running_stats=False):
    from rnr_amd.scene import unet_state_dict
    from rnr_amd.unet import UNetPlan
    sd = unet_state_dict(30, 78, 64, 5, seed=3)
    g = torch.Generator().manual_seed(6)
    for k in [k for k, v in sd.items() if k.endswith('.weight') and v.dim() == 1]:       # the BatchNorm layers
        sd[k[:-len('weight')] + 'running_mean'] = torch.randn(sd[k].numel(), generator=g)
        sd[k[:-len('weight')] + 'running_var'] = torch.rand(sd[k].numel(), generator=g) + 0.5
    sd = {k: v.to(DEV) if torch.is_tensor(v) else v for k, v in sd.items()}
    plan = UNetPlan(sd, 30, 78, 64, 5, (256, 256), n, torch.device(DEV), bn_mode=mode,
                    update_running_stats=update_running_stats)
    x = torch.randn(n, 256, 256, plan.in_c_pad, generator=torch.Generator().manual_seed(4))
    x[..., :30] += 3.0 + torch.arange(30) / 10           # a DC offset on every input channel
    x[..., 30:] = 0
    return sd, plan, x.to(DEV)


@pytest.mark.parametrize('mode,n', [('batch', 3), ('batch_all', 2), ('batch_all', 1)])
def test_unet_plan_layer_statistics(mode, n):
    """UNetPlan on the benchmark network (nf0 64, five levels, 256^2) with an input carrying a DC offset: every BatchNorm
    layer's scale / shift against bn64 applied to the output that layer wrote, per view ('batch') or over the batch
    ('batch_all', whose running buffers are updated in place: the separate-launch path at two views, the fused one at one)."""
    from oracle import bn64
    sd, plan, x = _offset_unet(mode, n, update_running_stats=(mode == 'batch_all'))
    before = {k: v.detach().cpu().clone() for k, v in sd.items() if torch.is_tensor(v)}
    plan.forward(x, n)
    torch.cuda.synchronize()
    checked = 0
    for i, s in enumerate(plan.steps):
        bn = s['bn']
        if bn is None:
            continue
        o = s['out']
        raw = o.data[:n].cpu()
        gamma, beta = bn['gamma'].cpu(), bn['beta'].cpu()
        if mode == 'batch':
            ref = bn64.per_view(raw, o.c, gamma, beta, EPS)
            assert_affine(o.scale[:n].cpu(), o.shift[:n].cpu(), ref, beta, o.c, 'layer %d' % i)
        else:
            rm, rv = bn['running_mean'], bn['running_var']
            key = [k for k, v in sd.items() if v.data_ptr() == rm.data_ptr()][0]
            ref = bn64.batch_all(raw, o.c, gamma, beta, EPS, before[key], before[key[:-4] + 'var'], 0.1)
            assert_affine(o.scale[:n].cpu(), o.shift[:n].cpu(), ref, beta, o.c, 'layer %d' % i)
            assert_running(rm, rv, ref, 'layer %d' % i)
        checked += 1
    assert checked >= 10
    assert all(int(s['sync'].max()) == 0 for s in plan.steps if s['sync'] is not None)


def test_unet_plan_running_mode_affine():
    """bn_mode 'running': scale / shift are the state-dict's running buffers folded once (eval-mode BatchNorm), one float32
    rounding of gamma / sqrt(running_var + eps) and beta - running_mean scale each: 2^-22 relative."""
    sd, plan, x = _offset_unet('running', 1)
    checked = 0
    bnkeys = sorted({k[:-len('.running_mean')] for k in sd if k.endswith('.running_mean')})
    folded = {}
    for k in bnkeys:
        sc = sd[k + '.weight'].double() / torch.sqrt(sd[k + '.running_var'].double() + EPS)
        folded[k] = (sc.cpu(), (sd[k + '.bias'].double() - sd[k + '.running_mean'].double() * sc).cpu())
    for s in plan.steps:
        o = s['out']
        if s.get('bias') is not None or o.scale is None:
            continue
        sc, sh = o.scale[0, :o.c].cpu().double(), o.shift[0, :o.c].cpu().double()
        hits = [k for k, (a, b) in folded.items() if a.numel() == o.c and
                bool(((a - sc).abs() <= 2.0 ** -22 * a.abs() + 1e-30).all()) and
                bool(((b - sh).abs() <= 2.0 ** -22 * (b.abs() + (a * sd[k + '.running_mean'].cpu().double()).abs()) + 1e-30).all())]
        assert hits, 'no BatchNorm of the state dict folds to this layer\'s scale / shift'
        checked += 1
    assert checked >= 10


def test_dropin_unet_running_buffers_on_offset_input_and_eps_check():
    """The drop-in pytorch_prototyping.Unet (via network.RenderingNet) in train-mode BatchNorm on an input with a DC offset:
    every live BatchNorm's running_mean / running_var after one call against bn64.batch_all of the output its plan wrote,
    num_batches_tracked counted; then eps / momentum edited after the first forward must be refused, not ignored."""
    import network
    from oracle import bn64
    torch.manual_seed(0)
    net = network.RenderingNet(nf0=16, in_channels=12, out_channels=6, num_down_unet=5, use_gcn=False).to(DEV)
    net.eval()
    bns = []
    for mod in net.modules():
        if type(mod) == torch.nn.BatchNorm2d:
            mod.train()
            bns.append(mod)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 12, 64, 64, generator=g) + 5.0
    before = {id(m): (m.running_mean.detach().cpu().clone(), m.running_var.detach().cpu().clone(), int(m.num_batches_tracked))
              for m in bns}
    with torch.no_grad():
        net(x.to(DEV), None)
    torch.cuda.synchronize()
    unet = [m for m in net.modules() if hasattr(m, '_plans')][0]
    plan = list(unet._plans.values())[0]
    assert plan.bn_mode == 'batch_all'
    by_ptr = {m.running_mean.data_ptr(): m for m in bns}
    checked = 0
    for s in plan.steps:
        bn = s['bn']
        if bn is None or bn['running_mean'] is None:
            continue
        m = by_ptr[bn['running_mean'].data_ptr()]
        rm0, rv0, nb0 = before[id(m)]
        o = s['out']
        ref = bn64.batch_all(o.data[:2].cpu(), o.c, m.weight.detach().cpu(), m.bias.detach().cpu(), EPS, rm0, rv0, 0.1)
        assert_running(m.running_mean, m.running_var, ref, 'drop-in')
        assert int(m.num_batches_tracked) == nb0 + 1
        checked += 1
    assert checked >= 10
    live = unet._live_batchnorms()
    for attr, val in (('eps', 1e-3), ('momentum', 0.2)):
        old = getattr(live[0], attr)
        setattr(live[0], attr, val)
        with pytest.raises(NotImplementedError, match='BatchNorm2d'):
            with torch.no_grad():
                net(x.to(DEV), None)
        setattr(live[0], attr, old)
    with torch.no_grad():
        net(x.to(DEV), None)
