"""-m gpu: the HIP backward of the texture mapper (rnr_texture_mapper_backward, both kernel forms), its autograd wiring through
network.TextureMapper, the refusal of the U-Net to take an input that requires grad, and the chain photograph -> ray renderer ->
albedo channels -> texture of train_rnr.py, against torch.autograd through the float64 oracle/shade64.py (pinned by
tests/test_texture_backward_cpu.py).

The bound is derived in tests/texture_bwd_ref.py, per texel and channel: |got - ref| <= (n_t + 6) EPS A_t; never from a measured
error.  The worst error / bound of every case is printed.  Every direct call of the C ABI starts from gradient buffers filled
with 1e30: the entry point has to clear them."""
import ctypes

import numpy as np
import pytest
import torch

import texture_bwd_ref as tb
from test_gpu_shade_sweep import _renderer_inputs
from texture_bwd_ref import EPS, T

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
D = torch.float64


def _abi_backward(uv, sh, g, sizes, C, sh_start, fill=1e30):
    """rnr_texture_mapper_backward on gradient buffers filled with `fill` -> (return code, list of [S,S,C] CPU tensors)."""
    from rnr_amd import _lib, ops
    N, H, W = uv.shape[:3]
    d_uv, d_g = uv.to(DEV).contiguous(), (g.to(DEV).contiguous() if g is not None else None)
    d_sh = sh.to(DEV).contiguous() if sh is not None else None
    grads = [torch.full((s, s, C), fill, dtype=torch.float32, device=DEV) for s in sizes]
    nl = len(sizes)
    ptrs = (ctypes.c_void_p * max(nl, 1))(*[t.data_ptr() for t in grads])
    szs = (ctypes.c_int * max(nl, 1))(*sizes)
    torch.cuda.synchronize()
    rc = _lib.load().rnr_texture_mapper_backward(ops._ptr(d_uv), ops._ptr(d_sh), ops._ptr(d_g), ptrs, szs, nl, C,
                                                 int(sh_start if sh_start is not None else 3), N, H, W, ops._stream())
    torch.cuda.synchronize()
    return rc, [t.cpu() for t in grads]


def _check(uv, sh, g, sizes, C, sh_start, what):
    rc, got = _abi_backward(uv, sh, g, sizes, C, sh_start)
    assert rc == 0
    return tb.check_grads(got, uv, sh, g, sizes, C, sh_start, what)


# ------------------------------------------------------------------------------------------------
# 1. sweep: channel counts, level pyramids, SH on and off, both image sizes (7 x 13: one lane per (pixel, channel); 20 x 24: tiles)
# ------------------------------------------------------------------------------------------------
SWEEP = [(37, 30, 3, 3), (32, 16, 4, 6), (5, 1, 1, None), (8, 9, 4, 0), (33, 3, 3, None),
         (6, 70, 1, None)]      # 70 channels: two passes through the 64-channel LDS tile of the per-lane form


@pytest.mark.parametrize('hw', [(7, 13), (20, 24)], ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('S,C,levels,sh_start', SWEEP, ids=lambda v: str(v))
def test_texture_backward_sweep_vs_float64_autograd(S, C, levels, sh_start, hw):
    """2 views; random uv plus the pinned uv (0,0), (1,1), (1 - 2^-24, 0), (-0.1, 0.5), (1.0000001, 0.5); C = 30 (37/18/9, two
    16-channel passes of the tile form), 16, 1, 9 (8/4/2/1: down to a 1 x 1 level), 3 and 70."""
    sizes = tb.level_sizes(S, levels)
    uv, sh, g = tb.random_scene(S * 100 + C, 2, hw[0], hw[1], C, sh_start is not None)
    _check(uv, sh, g, sizes, C, sh_start, 'sweep S%d C%d %dx%d' % (S, C, hw[0], hw[1]))


# ------------------------------------------------------------------------------------------------
# 2. smooth uv with a seam: the LDS box and the straight-to-global taps in one tile
# ------------------------------------------------------------------------------------------------
def test_texture_backward_seam_fixture_scene(golden):
    """The fixture's 2 x 20 x 24 scene (S 32, C 16, 4 levels, sh_start 6): a uv ramp with a jump of 0.25 halfway across each row
    and one row of random uv, so a tile's level-0 footprint does not fit its box."""
    f = golden('texture_bwd/texture_bwd_cases')
    uv, sh, g = T(f['uv']), T(f['sh']), T(f['grad_out'])
    _check(uv, sh, g, [int(s) for s in f['sizes']], 16, int(f['sh_start_ch']), 'seam 2x20x24')


@pytest.mark.parametrize('N,H,W', [(3, 33, 65), (1, 9, 1)], ids=['3x33x65', '1x9x1'])
def test_texture_backward_seam_ragged_sizes(N, H, W):
    """3 x 33 x 65: a multiple of neither 64 pixels nor of the 16 x 16 tile; 1 x 9 x 1: one column."""
    uv, sh, g = tb.seam_scene(N * 1000 + H, N, H, W, 16)
    _check(uv, sh, g, tb.level_sizes(32, 4), 16, 6, 'seam %dx%dx%d' % (N, H, W))


@pytest.mark.parametrize('form', ['a', 'b'])
def test_texture_backward_each_form_forced(form, monkeypatch):
    """RNR_TEXTURE_BWD_FORM (what scripts/texture_backward_time.py alternates) on shapes the dispatch would give to the other
    form: the per-lane form on 3 x 33 x 65 (ragged last workgroup), the tile form on 2 x 7 x 13 (one partial tile per view) and
    on a 512-texel level whose random-uv footprint never fits the box."""
    monkeypatch.setenv('RNR_TEXTURE_BWD_FORM', form)
    if form == 'a':
        uv, sh, g = tb.seam_scene(5, 3, 33, 65, 16)
        _check(uv, sh, g, tb.level_sizes(32, 4), 16, 6, 'forced a')
    else:
        uv, sh, g = tb.random_scene(6, 2, 7, 13, 30, True)
        _check(uv, sh, g, tb.level_sizes(37, 3), 30, 3, 'forced b, 7x13')
        uv, sh, g = tb.random_scene(7, 1, 20, 24, 3, False)
        _check(uv, None, g, [512, 256], 3, None, 'forced b, S512')


# ------------------------------------------------------------------------------------------------
# 3. contention
# ------------------------------------------------------------------------------------------------
def test_texture_backward_contention_one_uv():
    """Every pixel of 1 x 33 x 65 has uv (0.37, 0.37): 2145 adds per touched texel and channel.  Same bound, one run."""
    C, sizes = 9, tb.level_sizes(8, 4)
    uv, sh, g = tb.random_scene(9, 1, 33, 65, C, True)
    uv = torch.full_like(uv, 0.37)
    n_t, _ = tb.tap_stats(uv, sh, g, sizes, C, 0)
    assert max(int(n.max()) for n in n_t) == 2145
    _check(uv, sh, g, sizes, C, 0, 'contention')


# ------------------------------------------------------------------------------------------------
# 4. zeros
# ------------------------------------------------------------------------------------------------
def test_texture_backward_zero_gradient_gives_exact_zero():
    """grad_out = 0 (and -0): every level exactly 0, from buffers filled with 1e30: the entry point clears them."""
    uv, sh, g = tb.seam_scene(4, 2, 20, 24, 16)
    for zero in (torch.zeros_like(g), -torch.zeros_like(g)):
        rc, got = _abi_backward(uv, sh, zero, tb.level_sizes(32, 4), 16, 6)
        assert rc == 0 and all(float(t.abs().max()) == 0.0 for t in got)


@pytest.mark.parametrize('hw', [(7, 13), (20, 24)], ids=lambda s: '%dx%d' % s)
def test_texture_backward_left_half_zero(hw):
    """grad_out zero on the left half of the image (a masked loss), u rising with the column: texels only the left half
    touches must be exactly 0 (check_grads asserts that wherever A_t = 0), the others meet the bound."""
    uv, sh, g = tb.seam_scene(8, 2, hw[0], hw[1], 16)
    g[..., :hw[1] // 2] = 0.0
    sizes = tb.level_sizes(32, 4)
    _, A_all = tb.tap_stats(uv, sh, torch.ones_like(g), sizes, 16, 6)
    _, A = tb.tap_stats(uv, sh, g, sizes, 16, 6)
    assert int(((A_all[0] > 0) & (A[0] == 0)).sum()) > 0        # some texels are touched by the left half alone
    _check(uv, sh, g, sizes, 16, 6, 'left half zero %dx%d' % hw)


# ------------------------------------------------------------------------------------------------
# 5. argument checks
# ------------------------------------------------------------------------------------------------
def test_texture_backward_argument_errors_launch_nothing():
    """Each bad call returns an error code and leaves the 1e30-filled buffers as they were (no clear, no launch)."""
    from rnr_amd import _lib
    uv, sh, g = tb.random_scene(1, 1, 7, 13, 16, True)
    sizes = [8, 4]
    untouched = lambda got: all(bool((t == 1e30).all()) for t in got)
    rc, got = _abi_backward(uv, sh, g, sizes, 16, 8)            # 8 + 9 > 16 with an SH map
    assert rc != 0 and untouched(got) and 'sh_start_ch' in _lib.load().rnr_last_error().decode()
    rc, got = _abi_backward(uv, None, g, sizes, 16, 8)          # ... and fine without one
    assert rc == 0 and not untouched(got)
    rc, got = _abi_backward(uv, sh, g, [], 16, 6)               # num_levels 0
    assert rc != 0
    rc, got = _abi_backward(uv, sh, None, sizes, 16, 6)         # null grad_out
    assert rc != 0 and untouched(got)


# ------------------------------------------------------------------------------------------------
# 6. wiring: network.TextureMapper -> loss.backward()
# ------------------------------------------------------------------------------------------------
def _mapper(seed, fix_texture=False):
    import network
    rng = np.random.default_rng(seed)
    tm = network.TextureMapper(32, 16, 4, apply_sh=True, fix_texture=fix_texture)
    for l, p in enumerate(tm.textures):
        p.data.copy_(T((0.2 + 0.8 * rng.random(tuple(p.shape))).astype(np.float32)) * (1.0 if l == 0 else 0.1))
    return tm.to(DEV)


def test_texture_mapper_module_gradients():
    """.grad of loss = <g, TextureMapper(uv, sh)> on every level: the parameter's shape [1,S,S,C], within the bound of the float64
    yardstick (and so is ops.texture_mapper_backward on the same inputs); a second backward accumulates; under no_grad no
    grad_fn and the same bits; a uv_map or an SH map that requires grad raises."""
    from rnr_amd import ops
    tm = _mapper(0)
    sizes = tb.level_sizes(32, 4)
    uv, sh, g = tb.seam_scene(21, 1, 64, 64, 16)
    d_uv, d_sh, d_g = uv.to(DEV), sh.to(DEV), g.to(DEV)
    out = tm(d_uv, d_sh, sh_start_ch=6)
    assert out.grad_fn is not None and out.requires_grad
    (out * d_g).sum().backward()
    first = [p.grad.clone() for p in tm.textures]
    assert [tuple(t.shape) for t in first] == [(1, s, s, 16) for s in sizes]
    tb.check_grads([t[0].cpu() for t in first], uv, sh, g, sizes, 16, 6, 'TextureMapper.grad')
    tb.check_grads([t.cpu() for t in ops.texture_mapper_backward(d_uv, d_sh, d_g, sizes, 6)], uv, sh, g, sizes, 16, 6,
                   'ops.texture_mapper_backward')
    (tm(d_uv, d_sh, sh_start_ch=6) * d_g).sum().backward()
    # the second backward adds a gradient that is again within the bound: twice the yardstick within twice the bound plus the add
    ref = tb.oracle_grads(uv, sh, g, sizes, 16, 6)
    n_t, A_t = tb.tap_stats(uv, sh, g, sizes, 16, 6)
    for p, r, n, A in zip(tm.textures, ref, n_t, A_t):
        assert ((p.grad[0].cpu().to(D) - 2 * r).abs() <= 2 * (n.to(D) + 7) * EPS * A).all()
    with torch.no_grad():
        quiet = tm(d_uv, d_sh, sh_start_ch=6)
    assert quiet.grad_fn is None and not quiet.requires_grad and torch.equal(quiet, out)
    with pytest.raises(NotImplementedError, match='uv_map'):
        tm(d_uv.clone().requires_grad_(), d_sh, sh_start_ch=6)
    with pytest.raises(NotImplementedError, match='sh_basis_map'):
        tm(d_uv, d_sh.clone().requires_grad_(), sh_start_ch=6)


def test_texture_mapper_computes_only_the_levels_that_need_grad(monkeypatch):
    """Level 1 frozen: its .grad stays None and the backward asks the kernel for the other three levels only."""
    from rnr_amd import ops
    tm = _mapper(1)
    tm.textures[1].requires_grad_(False)
    asked = []
    real = ops.texture_mapper_backward
    monkeypatch.setattr(ops, 'texture_mapper_backward', lambda uv, sh, g, sizes, s0: (asked.append(list(sizes)), real(uv, sh, g, sizes, s0))[1])
    uv, sh, g = tb.seam_scene(22, 2, 20, 24, 16)
    (tm(uv.to(DEV), sh.to(DEV), sh_start_ch=6) * g.to(DEV)).sum().backward()
    assert asked == [[32, 8, 4]] and tm.textures[1].grad is None
    got = [tm.textures[l].grad[0].cpu() for l in (0, 2, 3)]
    tb.check_grads(got, uv, sh, g, [32, 8, 4], 16, 6, 'levels 0, 2, 3')


def test_texture_mapper_fix_texture_builds_no_graph():
    tm = _mapper(2, fix_texture=True)
    uv, sh, _ = tb.seam_scene(23, 1, 20, 24, 16)
    out = tm(uv.to(DEV), sh.to(DEV), sh_start_ch=6)
    assert out.grad_fn is None and not out.requires_grad


def test_rendering_net_refuses_the_texture_output_in_grad_mode():
    """RenderingNet has no backward: on the module's output (which requires grad now) it raises instead of cutting the graph
    silently; on the same tensor under no_grad, and on .detach(), it runs and gives equal outputs."""
    import network
    tm = _mapper(3)
    net = network.RenderingNet(nf0=4, in_channels=16, out_channels=3, num_down_unet=5, use_gcn=False).to(DEV).eval()
    uv, sh, _ = tb.seam_scene(24, 1, 64, 64, 16)
    neural = tm(uv.to(DEV), sh.to(DEV), sh_start_ch=6)
    assert neural.requires_grad
    with pytest.raises(NotImplementedError, match='inference-only'):
        net(neural, None)
    with torch.no_grad():
        quiet = net(neural, None)
    det = net(neural.detach(), None)
    assert quiet.shape == (1, 3, 64, 64) and torch.isfinite(quiet).all() and torch.equal(quiet, det)
    assert quiet.grad_fn is None and det.grad_fn is None


# ------------------------------------------------------------------------------------------------
# 7. end to end: the graph of train_rnr.py:512-539, 564-585, 596-608 with rays_lt supplied
# ------------------------------------------------------------------------------------------------
def _loss_alb(flatten_mipmap, init):
    """train_rnr.py:596-608 with loss_alb_weight 1."""
    total = 0
    for a, b in ((3, 6), (0, 3)):
        tex = flatten_mipmap(a, b)
        mask = (tex != init[..., a:b].to(tex.dtype)).any(dim=-1, keepdim=True).to(tex.dtype)
        assert float(mask.min()) == 1.0
        total = total + ((tex * mask).sum(dim=(0, 1, 2)) / mask.sum(dim=(0, 1, 2)) - 0.5).abs().sum() / 3
    return total


def test_image_loss_reaches_the_texture_through_the_ray_renderer():
    """TextureMapper(32, 16, 4, apply_sh=True) -> albedo slices -> RayRenderer(seperate_albedo=True) on an 11 x 23 probe -> L1 of
    the alpha-weighted central crop, plus loss_alb on flatten_mipmap; 2 views of 24 x 24, 5 + 3 rays.  Reference: the same chain
    in float64 through shade64.  The targets sit 0.05 .. 0.5 away from the float64 frame and the albedo means 0.1 or more from
    0.5, so float32 and float64 agree on every sign.  Bound on .grad of level l, texel t, channel c, as a sum of:
      * the albedo gradients the ray renderer's backward hands over carry tol_albedo = 2 EPS |g_out| (n_group + 15)
        (test_gpu_ray_backward._check_backward; lp_scale_factor 1) plus 2 EPS |g_out| 2 for torch's float32 1 / n and alpha
        product in g_out (ltt <= 2): 2 EPS |g_out| (n_group + 17); scattered through the exact adjoint: sum tol_albedo |w|;
      * the texture scatter itself: (n_t + 6) EPS A_t with A_t from |float64 albedo gradient|;
      * loss_alb, torch's float32 ops: a texel of level l collects at most (2 S / S_l + 2)^2 bilinear-upsampling contributions
        of one sign, each a weight (3 EPS), a product, the division by the count and by 3: ((2 S / S_l + 2)^2 + 8) EPS |G_alb|;
      * autograd's float32 sum of the two paths: EPS (|G_render| + |G_alb|) (1 + the above, second order dropped).
    Channels >= 6 get nothing from either path: exactly 0 on every level."""
    import network
    from oracle import shade64 as o64
    N, H, W, R, nd, S, C = 2, 24, 24, 8, 3, 32, 16
    ns = R - nd
    sizes = tb.level_sizes(S, 4)
    tm = _mapper(7)
    rr = network.RayRenderer(None, network.Interpolater())
    rng = np.random.default_rng(70)
    uv, sh, _ = tb.seam_scene(71, N, H, W, C)
    rays_uv, rays_lt, lp, _, _ = [T(t) for t in _renderer_inputs(rng, 3, R, N, H, W, 1)]
    alpha = T((rng.random((N, 1, H, W)) > 0.3).astype(np.float32))
    alpha_c = alpha[:, :, 5:-5, 5:-5]

    def chain64(tex64):
        neural = o64.texture_mapper(tex64, uv, sh, 6)
        out = o64.ray_renderer(neural[:, 3:6], rays_uv, rays_lt, lp, albedo_diffuse=neural[:, :3], num_ray_diffuse=nd,
                               seperate_albedo=True)[0]
        return neural, out

    tex64 = [p.detach().cpu().to(D).requires_grad_(True) for p in tm.textures]
    neural64, out64 = chain64(tex64)
    sign = T(np.where(rng.random(out64.shape) < 0.5, -1.0, 1.0))
    target = (out64.detach() + sign * T(0.05 + 0.45 * rng.random(out64.shape))).float()

    def flatten64(a, b):
        out = None
        for lvl, p in enumerate(tex64):
            t = p[..., a:b]
            if lvl > 0:
                t = torch.nn.functional.interpolate(t.permute(0, 3, 1, 2), size=(S, S), mode='bilinear').permute(0, 2, 3, 1)
            out = t if out is None else out + t
        return out

    init = tm.tex_flatten_mipmap_init.cpu()
    loss_rn64 = ((out64[:, :, 5:-5, 5:-5] * alpha_c.to(D)) - (target.to(D)[:, :, 5:-5, 5:-5] * alpha_c.to(D))).abs().mean()
    assert float(((out64.detach() - target.to(D)).abs()).min()) > 1e-3
    for a, b in ((0, 3), (3, 6)):
        assert float((flatten64(a, b).detach().mean(dim=(0, 1, 2)) - 0.5).abs().min()) > 0.1
    G_render = torch.autograd.grad(loss_rn64, tex64, retain_graph=True)
    g_neural = torch.autograd.grad(loss_rn64, neural64, retain_graph=True)[0]
    G_alb = torch.autograd.grad(_loss_alb(flatten64, init), tex64)

    # the GPU chain
    d = lambda t: t.to(DEV)
    neural = tm(d(uv), d(sh), sh_start_ch=6)
    out = rr(neural[:, 3:6], d(rays_uv), d(rays_lt), lp=d(lp), albedo_diffuse=neural[:, :3], num_ray_diffuse=nd, seperate_albedo=True)[0]
    a_c = d(alpha_c)
    l1 = torch.nn.L1Loss()
    loss_rn = l1((out[:, :, 5:-5, 5:-5] * a_c).contiguous().view(-1).float(), (d(target)[:, :, 5:-5, 5:-5] * a_c).reshape(-1).float())
    loss = loss_rn + _loss_alb(tm.flatten_mipmap, tm.tex_flatten_mipmap_init)
    assert abs(float(loss.detach()) - float((loss_rn64 + _loss_alb(flatten64, init)).detach())) < 1e-5
    loss.backward()

    g_out = torch.zeros(N, 3, H, W, dtype=D)
    g_out[:, :, 5:-5, 5:-5] = alpha_c.to(D) / out64[:, :, 5:-5, 5:-5].numel()
    tol_neural = torch.zeros(N, C, H, W, dtype=D)
    tol_neural[:, 0:3] = 2 * EPS * g_out * (nd + 17)
    tol_neural[:, 3:6] = 2 * EPS * g_out * (ns + 17)
    _, A_tol = tb.tap_stats(uv, sh, tol_neural.float(), sizes, C, 6)
    n_t, A_t = tb.tap_stats(uv, sh, g_neural.float(), sizes, C, 6)
    worst = 0.0
    for l, p in enumerate(tm.textures):
        got = p.grad[0].cpu()
        assert tuple(p.grad.shape) == (1, sizes[l], sizes[l], C)
        assert float(got[..., 6:].abs().max()) == 0.0
        ref = (G_render[l] + G_alb[l])[0]
        tol = (A_tol[l] * (1 + 8 * EPS) + (n_t[l].to(D) + 6) * EPS * A_t[l] + ((2 * S / sizes[l] + 2) ** 2 + 8) * EPS * G_alb[l][0].abs()
               + EPS * (G_render[l][0].abs() + G_alb[l][0].abs()) * (1 + 1e-3))
        err = (got.to(D) - ref).abs()
        assert float(ref[..., :6].abs().max()) > 0.0 and float(G_render[l].abs().max()) > 0.0
        ratio = float((err / tol.clamp(min=1e-300))[..., :6].max())
        worst = max(worst, ratio)
        assert (err <= tol).all(), 'level %d: worst error / bound = %.3f' % (l, ratio)
    print('end to end: worst error / bound = %.3f' % worst)
