"""-m gpu: precision='f16' through the Python layer — UNetPlan on the two golden networks and on a seeded RenderingNet-shaped one
(108 -> 78 channels, nf0 = 16, 2 x 128^2: the large layers run conv_halo_emu_kernel's one-term format, the bottom ones fall back
to the fp32 kernels from the same buffers), RNRPipeline on the golden frame64 scene.  The yardstick is the 'f32' plan / pipeline of
the same weights and inputs: PSNR of the tanh output resp. of the frame at peak 1 >= 50 dB, the project's north_star figure.  A CPU
run of the reference U-Net with fp16-rounded operands and fp32 accumulation measured 65.6 dB against float64 at this
configuration, so the arithmetic alone keeps 15 dB of margin.  Measured here (profiles/f16_accuracy.txt):
    unet_nf4 64^2  67.0 dB    unet_dnr_nf4 32^2  68.0 dB    nf0 = 16, 108 -> 78, 2 x 128^2  65.2 dB    frame64  83.0 dB"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NORTH_STAR_DB = 50.0


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def psnr1(a, b):
    """PSNR at peak 1."""
    return -10.0 * float(torch.log10(((a.double() - b.double()) ** 2).mean()))


def tanh_out(plan, x, cout):
    from rnr_amd import ops
    raw = plan.forward(ops.nchw_to_nhwc(x.to(DEV), plan.in_c_pad))
    return ops.nhwc_to_nchw(raw, cout, bias=plan.out_bias, apply_tanh=True).cpu()


def compare_plans(tag, sd, x, cin, cout, nf0, hw):
    from rnr_amd import _lib
    from rnr_amd.unet import UNetPlan
    mk = lambda **kw: UNetPlan(sd, cin, cout, nf0, 5, (hw, hw), x.shape[0], torch.device(DEV), **kw)
    half, exact = mk(precision='f16'), mk(precision='f32')
    assert half.conv_algo == 'direct' and half.precision == 'f16'                  # forced, whatever the default algorithm is
    assert all(s['desc'].flags & _lib.CONV_F16 and not s['desc'].flags & (_lib.CONV_WINOGRAD | _lib.CONV_F32_EMU_ANY)
               for s in half.steps)
    algos = [half.L.rnr_conv_algorithm(ctypes.byref(s['desc']), x.shape[0], *s['in_hw']) for s in half.steps]
    assert set(algos) == {0}
    y16, y32 = tanh_out(half, x, cout), tanh_out(exact, x, cout)
    assert bool(torch.isfinite(y16).all())
    p = psnr1(y16, y32)
    print('\nF16-PSNR %s: tanh output vs the f32 plan %.2f dB at peak 1, max |diff| %.3g' % (tag, p, float((y16 - y32).abs().max())))
    assert p >= NORTH_STAR_DB, p
    assert not torch.equal(y16, y32), 'the f16 plan returned the f32 plan\'s output: the flag did not reach the kernels'
    # the first convolution reads the network input alone (no BatchNorm statistics in front of it): its raw output is
    # bit-identical from run to run
    first = half.steps[0]['out'].data[:x.shape[0]].clone()
    tanh_out(half, x, cout)
    assert torch.equal(half.steps[0]['out'].data[:x.shape[0]], first)
    return half, exact


@pytest.mark.parametrize('name,cin,cout,hw', [('unet_nf4', 10, 6, 64), ('unet_dnr_nf4', 7, 3, 32)])
def test_f16_plan_on_the_golden_networks(golden, name, cin, cout, hw):
    g = golden(name)
    sd = {k[3:]: T(g[k]) for k in g.files if k.startswith('sd:')}
    compare_plans(name, sd, T(g['x']), cin, cout, 4, hw)


def test_f16_plan_on_a_rendering_net_shape():
    from rnr_amd import _lib, testing
    sd = testing.unet_state_dict(108, 78, 16, seed=5)
    x = torch.randn(2, 108, 128, 128, generator=torch.Generator().manual_seed(6))
    half, _ = compare_plans('nf0=16 108->78 2x128^2', sd, x, 108, 78, 16, 128)
    # where the new kernels run: the planner's answer per layer, against the f32 descriptor's direct plan (the bottom layers'
    # maps are narrower than 16 pixels and fall back)
    big = [s for s in half.steps if min(s['in_hw']) >= 32]
    assert len(big) >= 8
    # share_weights_with obeys the precision: the donor's buffers hold the one-plane image
    from rnr_amd.unet import UNetPlan
    twin = UNetPlan(sd, 108, 78, 16, 5, (128, 128), 2, torch.device(DEV), precision='f16', share_weights_with=half)
    assert twin.steps[0]['packed'].data_ptr() == half.steps[0]['packed'].data_ptr()
    y_twin, y_half = tanh_out(twin, x, 78), tanh_out(half, x, 78)
    # the first layer's raw output depends on the packed weights and the input alone: two plans on one set of packed weights share
    # it bit for bit; behind it the BatchNorm statistics (float64 sums whose order is not fixed) stand between the two runs, so the
    # outputs are held to a distance far below the mode's own from 'f32' (65 dB), not to equality
    assert torch.equal(twin.steps[0]['out'].data, half.steps[0]['out'].data)
    assert psnr1(y_twin, y_half) >= 75.0
    with pytest.raises(ValueError, match='precision'):
        UNetPlan(sd, 108, 78, 16, 5, (128, 128), 2, torch.device(DEV), precision='f16x3', share_weights_with=half)
    f32 = _lib.load().rnr_packed_weight_floats
    for s in half.steps:
        d0 = _lib.RnrConvDesc.from_buffer_copy(s['desc'])
        d0.flags = 0
        n = f32(ctypes.byref(d0))
        assert s['packed'].numel() == n + 16 + (n + 1) // 2


def test_f16_range_surfaces_through_check_finite_first():
    """An activation of 65520 and above is an infinite fp16: the first forward of a check_finite='first' plan raises and names
    the range; the f32 plan takes the same input without complaint, and ordinary inputs pass."""
    from rnr_amd import ops, testing
    from rnr_amd.unet import UNetPlan
    sd = testing.unet_state_dict(16, 8, 16, seed=21, use_gcn=False)
    x = torch.randn(1, 16, 64, 64, generator=torch.Generator().manual_seed(9))
    mk = lambda **kw: UNetPlan(sd, 16, 8, 16, 5, (64, 64), 1, torch.device(DEV), **kw)
    ok = mk(precision='f16', check_finite='first')
    assert ok.check_finite == 'first'
    ok.forward(ops.nchw_to_nhwc(x.to(DEV), ok.in_c_pad))
    assert ok.check_finite is False
    bad = mk(precision='f16', check_finite='first')
    big = x.clone()
    big[0, 3, 20, 20] = 70000.0
    with pytest.raises(FloatingPointError, match=r"precision='f16'.*65520.*RNR_CONV_F16"):
        bad.forward(ops.nchw_to_nhwc(big.to(DEV), bad.in_c_pad))
    always = mk(precision='f16', check_finite=True)
    always.forward(ops.nchw_to_nhwc(x.to(DEV), always.in_c_pad))
    with pytest.raises(FloatingPointError, match='65520'):
        always.forward(ops.nchw_to_nhwc(big.to(DEV), always.in_c_pad))
    exact = mk(check_finite=True)
    exact.forward(ops.nchw_to_nhwc(big.to(DEV), exact.in_c_pad))


def test_f16_pipeline_on_the_golden_frame(golden):
    from rnr_amd import testing
    from rnr_amd.pipeline import RNRPipeline
    gm, gf = golden('rasterizer_module64'), golden('frame64')
    mesh = {'v': gm['buf_vertices'][0], 'vt': gm['mesh_vt'], 'vn': gm['buf_vertices_normals'][0],
            'f_v_idx': gm['mesh_f_v_idx'], 'f_vt_idx': gm['mesh_f_vt_idx'], 'f_vn_idx': gm['mesh_f_vn_idx']}
    sd = {k[3:]: T(gf[k]) for k in gf.files if k.startswith('sd:')}
    tex = [T(gf['tex%d' % i]) for i in range(4)]
    mk = lambda **kw: RNRPipeline(mesh, 64, tex, sd, testing.ray_pivots(6, 2, 5), testing.ray_pivots(6, 2, 10), T(gf['lp']), nf0=4,
                                  max_views=2, device=DEV, **kw)
    v = {k: T(gm[k]).to(DEV) for k in ['proj', 'pose', 'proj_inv', 'R_inv']}
    frame = lambda pipe: pipe.render(v['proj'], v['pose'], v['proj_inv'], v['R_inv']).cpu().clone()
    half = mk(precision='f16')
    assert half.unet.precision == 'f16' and half.unet.conv_algo == 'direct'
    f16, f32 = frame(half), frame(mk())
    p = psnr1(f16, f32)
    print('\nF16-PSNR frame64: frame vs the f32 pipeline %.2f dB at peak 1, max |diff| %.3g' % (p, float((f16 - f32).abs().max())))
    assert bool(torch.isfinite(f16).all()) and p >= NORTH_STAR_DB, p
    assert not torch.equal(f16, f32)
    # dead-tile elimination: the out layer's masked launch skips background tiles, the frame does not change
    assert torch.equal(frame(mk(precision='f16', skip_background_tiles=False)), f16)
