"""-m gpu: WHERE the kernels of csrc/unet_bwd.hip touch memory.  Like the forward convolutions they address their operands and a
shared workspace through descriptors without bounds: a write past a slab or a read of a stale slab neither faults nor — next to
fresh allocations — changes a value the float64 sweeps of tests/test_gpu_unet_backward.py look at.

  (a) guard bands   rnr_conv2d_weight_backward, rnr_conv2d_input_backward_ring, rnr_conv_out_backward and rnr_unet_out_backward
                    with every device operand carved out of a sentinel-filled allocation of its own (rnr_amd.testing.Guarded), at
                    the weakest alignment include/rnr_hip.h grants, workspaces at exactly the size their *_workspace_bytes function
                    returns, workspaces and outputs prefilled with the sentinel NaN: guards intact, outputs finite where the ABI
                    says they are written and untouched where it says they are not, and BITWISE the unguarded run's (a read of
                    workspace that was never written would show there).  No float64 reference: the values are bounded elsewhere.
  (b) NaN tracers   one NaN in an input must surface exactly where the operation's index structure says — the support of the
                    float64 reference run on indicator inputs (one-hot at the NaN's position, ones elsewhere, non-negative
                    weights), never torch's own NaN propagation; everything outside is bitwise the clean run.

Shapes: oracle/unet_bwd_cases.py (held against the host arithmetic by tests/test_unet_bwd_cases_cpu.py)."""
import pytest
import torch

import unet_bwd_ref as ub
from oracle import unet_bwd_cases as uc
from rnr_amd.testing import (SENTINEL, pad16, run_conv_out_backward, run_input_backward_ring, run_unet_out_backward,
                             run_weight_backward)
from test_gpu_conv_guard import assert_intact, bits
from test_gpu_unet_backward import _out_backward_draw

pytestmark = pytest.mark.gpu
D = torch.float64
NAN = float('nan')


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
def wg_inputs(case, kind, acts=(1, 2)):
    """Sources as (raw, scale, shift, act) with scale and shift on both, and g_y; every value non-zero."""
    N, H, W = case['N'], case['H'], case['W']
    g = torch.Generator().manual_seed(17 + 1000 * kind + H * W + case['c_out'])
    srcs = [(torch.randn(N, c, H, W, generator=g), torch.rand(N, c, generator=g) + 0.5, torch.randn(N, c, generator=g) * 0.5, a)
            for c, a in zip(case['cins'], acts)]
    gy = torch.randn(N, case['c_out'], *ub.out_hw(kind, H, W), generator=g)
    return srcs, gy


def wg_support(kind, x_ind, gy_ind, wshape):
    """Where the float64 weight gradient of indicator inputs is non-zero (the gradient is linear in W: evaluated at W = 0)."""
    wz = torch.zeros(wshape, dtype=D, requires_grad=True)
    (ub.conv_forward(kind, x_ind.double(), wz) * gy_ind.double()).sum().backward()
    assert bool((wz.grad >= 0).all())
    return wz.grad > 0


def dg_inputs(kind, N, H, W, cins, cout):
    g = torch.Generator().manual_seed(5 + 77 * kind + H + W)
    cin, k = sum(cins), 3 if kind == 0 else 4
    wt = torch.randn((cin, cout, k, k) if kind == 2 else (cout, cin, k, k), generator=g) / (cout * k * k) ** 0.5
    gy = torch.randn(N, cout, *ub.out_hw(kind, H, W), generator=g)
    return wt, gy


def ring_prefill(N, H, W, cs_pad, nan):
    """grad_in before the ring kernel: the sentinel NaN, or a finite pattern that differs from element to element."""
    if nan:
        return torch.full((N, H, W, cs_pad), SENTINEL, dtype=torch.int32)
    return (torch.arange(N * H * W * cs_pad, dtype=torch.float32) * 0.25 + 1.0).reshape(N, H, W, cs_pad)


# ------------------------------------------------------------------------------------------------
# (a) guard bands
# ------------------------------------------------------------------------------------------------
WG_GUARD = [(c, k) for c in uc.WG_CASES if c['guard'] for k in c['kinds']]


@pytest.mark.parametrize('case,kind', WG_GUARD, ids=['%s-k%d' % (c['id'], k) for c, k in WG_GUARD])
def test_weight_gradient_guarded(case, kind):
    srcs, gy = wg_inputs(case, kind)
    args = (kind, srcs, gy, case['c_out'], case['N'], case['H'], case['W'])
    plain = run_weight_backward(*args)
    guarded, rep = run_weight_backward(*args, guard=True)
    assert_intact('rnr_conv2d_weight_backward', rep, ['src%d.%s' % (j, n) for j in range(len(srcs)) for n in ('data', 'scale', 'shift')]
                  + ['g_y', 'grad_weight', 'workspace'])
    assert bool(torch.isfinite(guarded).all()), 'grad_weight not finite (a sentinel was read, or an element never written)'
    assert torch.equal(bits(guarded), bits(plain)), 'guarded and unguarded grad_weight differ'


DG_GUARD = [c + (s,) for c in uc.DG_GUARD for s in range(len(c[4]))]


@pytest.mark.parametrize('kind,N,H,W,cins,cout,source', DG_GUARD, ids=lambda v: str(v).replace(' ', ''))
def test_ring_guarded(kind, N, H, W, cins, cout, source):
    """The ring kernel alone on a grad_in full of the sentinel: ring pixels finite with padding channels 0, every other pixel
    still the sentinel."""
    wt, gy = dg_inputs(kind, N, H, W, cins, cout)
    c, cp = cins[source], pad16(cins[source])
    args = (kind, cins, cout, source, gy, wt, ring_prefill(N, H, W, cp, True), N, H, W)
    plain = run_input_backward_ring(*args)
    guarded, rep = run_input_backward_ring(*args, guard=True)
    assert_intact('rnr_conv2d_input_backward_ring', rep, ['g_y', 'weight', 'grad_in'])
    ring = ub.ring_mask(kind, H, W)
    assert bool(ring.any()) and (kind == 0 or bool((~ring).any()))
    assert bool(torch.isfinite(guarded[:, ring]).all()), 'a ring pixel was not written'
    assert bool((guarded[:, ring][..., c:] == 0).all()), 'padding channels of the ring pixels must be 0'
    assert bool((bits(guarded)[:, ~ring] == SENTINEL).all()), 'a pixel outside the ring was written'
    assert torch.equal(bits(guarded), bits(plain)), 'guarded and unguarded grad_in differ'


OB_GUARD = [c for c in uc.OB_CASES if c['guard']]
# one call per statistics form, the activations and the second consumer in turn
OB_GUARD_GRID = [(1, True, 0, True), (2, False, 1, True), (0, True, 2, True), (1, False, 0, False)]


def ob_inputs(case, act, two, mode, bn):
    g = torch.Generator().manual_seed(case['c_pad'] + 10 * mode + act + 100 * two)
    y, gz0, gz1, gamma, saved, scale, shift, _, _, _ = _out_backward_draw(g, case['N'], case['h'], case['w'], case['c'], case['c_pad'],
                                                                          mode, bn, two)
    return dict(y=y, scale=scale, shift=shift, act=act, gz0=gz0, gz1=gz1, gamma=gamma, saved=saved, mode=mode, c_pad=case['c_pad'])


@pytest.mark.parametrize('case', OB_GUARD, ids=[c['id'] for c in OB_GUARD])
def test_conv_out_backward_guarded(case):
    c = case['c']
    for act, two, mode, bn in OB_GUARD_GRID:
        tag = 'rnr_conv_out_backward mode %d act %d bn %d two %d' % (mode, act, bn, two)
        a = ob_inputs(case, act, two, mode, bn)
        plain = run_conv_out_backward(**a)
        gy, gg, gb, rep = run_conv_out_backward(guard=True, **a)
        assert_intact(tag, rep, ['y', 'g_z0', 'shift', 'g_y', 'g_gamma', 'g_beta', 'workspace'] + (['g_z1'] if two else [])
                      + (['scale', 'gamma', 'saved'] if bn else []))
        assert bool(torch.isfinite(gy).all()) and bool(torch.isfinite(gb).all()), '%s: g_y / g_beta not finite' % tag
        assert bool((gy[..., c:] == 0).all()), '%s: padding channels of g_y must be 0' % tag
        if bn:
            assert bool(torch.isfinite(gg).all()), '%s: g_gamma not finite' % tag
        else:
            assert bool((bits(gg) == SENTINEL).all()), '%s: g_gamma must not be written without BatchNorm' % tag
            assert bool(torch.isnan(plain[1]).all())
        for name, g_, p_ in zip(('g_y', 'g_gamma', 'g_beta'), (gy, gg, gb), plain):
            if bn or name != 'g_gamma':
                assert torch.equal(bits(g_), bits(p_)), '%s: guarded and unguarded %s differ' % (tag, name)


@pytest.mark.parametrize('apply_tanh', [0, 1])
@pytest.mark.parametrize('n,c,h,w,c_pad', uc.UO_CASES, ids=lambda v: str(v))
def test_unet_out_backward_guarded(n, c, h, w, c_pad, apply_tanh):
    g = torch.Generator().manual_seed(n * 1000 + c + 1)
    g_out = torch.randn(n, c, h, w, generator=g)
    out = torch.tanh(torch.randn(n, c, h, w, generator=g)) if apply_tanh else None
    plain = run_unet_out_backward(g_out, out, apply_tanh, c_pad)
    guarded, rep = run_unet_out_backward(g_out, out, apply_tanh, c_pad, guard=True)
    assert_intact('rnr_unet_out_backward', rep, ['g_out', 'g_raw'] + (['out'] if apply_tanh else []))
    assert bool(torch.isfinite(guarded).all()) and bool((guarded[..., c:] == 0).all())
    assert torch.equal(bits(guarded), bits(plain)), 'guarded and unguarded g_raw differ'


# ------------------------------------------------------------------------------------------------
# (b) NaN tracers
# ------------------------------------------------------------------------------------------------
WG_TRACER = [(c, k) for c in uc.WG_CASES if c['tracer'] for k in c['kinds']]


def _assert_traced(tag, got, clean, must):
    nan = torch.isnan(got)
    assert bool(nan[must].all()), '%s: %d of %d elements that read the NaN are not NaN' % (tag, int((~nan[must]).sum()), int(must.sum()))
    assert not bool(nan[~must].any()), '%s: NaN outside the footprint, first at %s' % (
        tag, tuple(int(v) for v in (nan & ~must).nonzero()[0]) if bool((nan & ~must).any()) else None)
    same = bits(got)[~must] == bits(clean)[~must]
    assert bool(same.all()), '%s: %d elements outside the footprint differ from the clean run' % (tag, int((~same).sum()))


@pytest.mark.parametrize('case,kind', WG_TRACER, ids=['%s-k%d' % (c['id'], k) for c, k in WG_TRACER])
def test_weight_gradient_nan_in_g_y(case, kind):
    """One NaN in g_y[n, co*, oy*, ox*], co* in the second M tile: grad_weight is NaN for that co*, every live ci and exactly the
    taps whose anchor pixel reads (oy*, ox*) — for the transposed kind one parity class, 4 of the 16 taps at an interior pixel
    — and bitwise the clean run everywhere else."""
    N, H, W, cins, cout = case['N'], case['H'], case['W'], case['cins'], case['c_out']
    srcs, gy = wg_inputs(case, kind)
    clean = run_weight_backward(kind, srcs, gy, cout, N, H, W)
    assert bool(torch.isfinite(clean).all()) and cout > 128
    oh, ow = ub.out_hw(kind, H, W)
    ones = torch.ones(N, sum(cins), H, W)
    for n, co, oy, ox in [(0, 128, 0, 0), (N - 1, cout - 1, oh - 1, ow - 1), (0, 129, oh // 2, ow // 2 - 1), (N - 1, 128, oh // 2 - 1, ow - 1),
                          (0, cout - 1, oh // 2 + 1, 1)]:
        tag = 'NaN in g_y at view %d channel %d pixel (%d, %d)' % (n, co, oy, ox)
        poisoned = gy.clone()
        poisoned[n, co, oy, ox] = NAN
        got = run_weight_backward(kind, srcs, poisoned, cout, N, H, W)
        ind = torch.zeros_like(gy)
        ind[n, co, oy, ox] = 1.0
        must = wg_support(kind, ones, ind, tuple(clean.shape))
        co_axis = 1 if kind == 2 else 0
        assert bool(must.any()) and set(must.nonzero()[:, co_axis].tolist()) == {co}
        taps = must.select(co_axis, co).flatten(1).sum(1)               # per input channel
        assert bool((taps == taps[0]).all()), 'the reading taps are the same for every input channel'
        if kind == 2 and 0 < oy < oh - 1 and 0 < ox < ow - 1:
            assert int(taps[0]) == 4
        if kind == 1:
            assert int(taps[0]) == 16
        _assert_traced(tag, got, clean, must)


@pytest.mark.parametrize('src1_act', [2, 1], ids=['relu', 'lrelu'])
@pytest.mark.parametrize('case,kind', WG_TRACER, ids=['%s-k%d' % (c['id'], k) for c, k in WG_TRACER])
def test_weight_gradient_nan_in_source_1(case, kind, src1_act):
    """One NaN in source 1's raw data at a channel beyond column 128 of the concatenated input (N tile 1): NaN for that input
    channel, every output channel and exactly the taps through which an output pixel reads the poisoned pixel; ReLU and
    LeakyReLU both let it through (rnr_conv_src in include/rnr_hip.h)."""
    N, H, W, cins, cout = case['N'], case['H'], case['W'], case['cins'], case['c_out']
    srcs, gy = wg_inputs(case, kind, acts=(1, src1_act))
    clean = run_weight_backward(kind, srcs, gy, cout, N, H, W)
    assert bool(torch.isfinite(clean).all())
    ones = torch.ones_like(gy)
    first = 128 - pad16(cins[0])                            # the first channel of source 1 that lies in column 128 or beyond
    assert 0 < first < cins[1] - 1
    for n, c1, iy, ix in [(0, first, 0, 0), (N - 1, cins[1] - 1, H - 1, W - 1), (0, first + 1, H // 2, W // 2), (N - 1, first, H - 1, 1),
                          (0, cins[1] - 1, 1, W - 1)]:
        tag = 'NaN in source 1 at view %d channel %d pixel (%d, %d)' % (n, c1, iy, ix)
        raw = srcs[1][0].clone()
        raw[n, c1, iy, ix] = NAN
        got = run_weight_backward(kind, [srcs[0], (raw,) + srcs[1][1:]], gy, cout, N, H, W)
        ci = cins[0] + c1
        ind = torch.zeros(N, sum(cins), H, W)
        ind[n, ci, iy, ix] = 1.0
        must = wg_support(kind, ind, ones, tuple(clean.shape))
        ci_axis = 0 if kind == 2 else 1
        assert bool(must.any()) and set(must.nonzero()[:, ci_axis].tolist()) == {ci}
        taps = must.select(ci_axis, ci).flatten(1).sum(1)               # per output channel
        assert bool((taps == taps[0]).all()) and int(taps[0]) >= 1
        _assert_traced(tag, got, clean, must)


OB_TRACER = [c for c in uc.OB_CASES if c['tracer']]


def ob_dependence(ind, mode, bn):
    """The index structure of rnr_conv_out_backward's formulas (include/rnr_hip.h), run on a non-negative indicator of g_z with
    every difference replaced by a sum: g_y reads g_v of its own element and, under train-mode BatchNorm, S1 and D of its
    statistics group; g_beta / g_gamma read every g_v of their channel.  -> (g_y [N,c,h,w], per-channel [c]) as booleans."""
    dep = ind.double()
    if bn and mode != 2:
        grp = (2, 3) if mode == 0 else (0, 2, 3)
        dep = dep + dep.sum(grp, keepdim=True)
    return dep > 0, ind.double().sum((0, 2, 3)) > 0


@pytest.mark.parametrize('case', OB_TRACER, ids=[c['id'] for c in OB_TRACER])
def test_conv_out_backward_nan_in_g_z(case):
    """One NaN in g_z0[n*, p*, c*], c* > 256 (the second workgroup of parameter-gradient lanes, the second pass of the
    coefficient loop): g_beta[c*], with BatchNorm g_gamma[c*], and g_y of channel c* over the statistic's group — view n* per
    view, every view over the whole call, that pixel alone for running statistics and without BatchNorm.  Every other channel,
    and channel c* outside the group, is bitwise the clean run."""
    N, h, w, c = case['N'], case['h'], case['w'], case['c']
    assert c > 258
    for act, two, mode, bn in [(1, True, 0, True), (2, False, 1, True), (0, True, 2, True), (2, True, 0, False), (1, False, 1, True),
                               (0, False, 0, True)]:
        a = ob_inputs(case, act, two, mode, bn)
        clean = run_conv_out_backward(**a)
        for n_, py, px, ch in [(1, 4, 3, 258), (0, h - 1, w - 1, c - 1), (N - 1, 0, 0, 257)]:
            tag = 'mode %d act %d bn %d two %d, NaN in g_z0 at view %d pixel (%d, %d) channel %d' % (mode, act, bn, two, n_, py, px, ch)
            gz0 = a['gz0'].clone()
            gz0[n_, ch, py, px] = NAN
            gy, gg, gb = run_conv_out_backward(**dict(a, gz0=gz0))
            ind = torch.zeros(N, c, h, w)
            ind[n_, ch, py, px] = 1.0
            must_y, must_c = ob_dependence(ind, mode, bn)
            want = {0: h * w, 1: N * h * w, 2: 1}[mode] if bn else 1
            assert int(must_y.sum()) == want and int(must_c.sum()) == 1 and bool(must_c[ch])
            must_pad = torch.zeros(N, h, w, case['c_pad'], dtype=torch.bool)
            must_pad[..., :c] = must_y.permute(0, 2, 3, 1)
            _assert_traced(tag + ': g_y', gy, clean[0], must_pad)
            _assert_traced(tag + ': g_beta', gb, clean[2], must_c)
            if bn:
                _assert_traced(tag + ': g_gamma', gg, clean[1], must_c)
            else:
                assert bool(torch.isnan(gg).all()) and bool(torch.isnan(clean[1]).all())       # never written


@pytest.mark.parametrize('kind,N,H,W,cins,cout,source', DG_GUARD, ids=lambda v: str(v).replace(' ', ''))
def test_ring_nan_in_g_y(kind, N, H, W, cins, cout, source):
    """One NaN in g_y reaches exactly the ring pixels whose defining sum (tests/unet_bwd_ref.py, on a one-hot g_y and all-ones
    weights) contains it, in every live channel of the source; the padding channels stay 0 and the pixels outside the ring keep
    what grad_in held."""
    wt, gy = dg_inputs(kind, N, H, W, cins, cout)
    assert bool((wt != 0).all())
    c, cp, off = cins[source], pad16(cins[source]), sum(cins[:source])
    before = ring_prefill(N, H, W, cp, False)
    clean = run_input_backward_ring(kind, cins, cout, source, gy, wt, before, N, H, W)
    ring = ub.ring_mask(kind, H, W)
    assert bool(torch.isfinite(clean).all())
    oh, ow = ub.out_hw(kind, H, W)
    for n, co, oy, ox in [(0, 0, 0, 0), (N - 1, cout - 1, oh - 1, ow - 1), (0, 129, oh // 2, ow // 2), (N - 1, 64, 0, ow // 2), (0, 1, oh // 2, 0)]:
        tag = 'NaN in g_y at view %d channel %d pixel (%d, %d)' % (n, co, oy, ox)
        poisoned = gy.clone()
        poisoned[n, co, oy, ox] = NAN
        got = run_input_backward_ring(kind, cins, cout, source, poisoned, wt, before, N, H, W)
        ind = torch.zeros_like(gy)
        ind[n, co, oy, ox] = 1.0
        reach = ub.defining_sum(kind, ind, torch.ones_like(wt), H, W)[:, off:off + c] > 0         # [N,c,H,W]
        reach &= ring[None, None]
        must = torch.zeros(N, H, W, cp, dtype=torch.bool)
        must[..., :c] = reach.permute(0, 2, 3, 1)
        _assert_traced(tag, got, clean, must)
        assert torch.equal(bits(got)[:, ~ring], bits(before)[:, ~ring]), '%s: a pixel outside the ring was written' % tag
