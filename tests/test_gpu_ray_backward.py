"""-m gpu: the HIP backward of the ray renderer (rnr_ray_renderer_backward), rnr_sh_reconstruct_backward, rnr_ray_transport and
what is built on them (autograd wiring of network.RayRenderer / LightingSH, RNRPipeline.light_transport, fit_sh_lighting),
against torch.autograd through the float64 oracle/shade64.py (pinned by tests/test_ray_backward_yardstick_cpu.py).

Tolerances are bounds derived from the arithmetic in units of EPS = 2^-24, as in tests/test_gpu_shade_sweep.py (every float32
+, -, *, / adds <= 1 EPS relative), never from a measured error; the one exception, the fit's FIT_RTOL, says so."""
import math

import numpy as np
import pytest
import torch

from test_gpu_shade_sweep import RAY_CASES, RENDERER_CASES, _ray_scene, _renderer_inputs

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EPS = 2.0 ** -24
D = torch.float64


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def _nan(*shape):
    return torch.full(shape, float('nan'), dtype=torch.float32, device=DEV)


def _dev(t):
    return None if t is None else t.to(DEV)


# ------------------------------------------------------------------------------------------------
# the float64 side
# ------------------------------------------------------------------------------------------------
def _oracle_grads(uv, lt, lp, a_s, a_d, nd, no_alb, sep, s, g):
    """torch.autograd through shade64.ray_renderer with float64 leaves: the gradients of sum_k <g_k, output_k> in
    (rays_lt, lp, albedo_specular, albedo_diffuse); g: six upstream gradients, None = zero."""
    from oracle import shade64 as o64
    leaves = [t.to(D).clone().requires_grad_(True) for t in (lt, lp, a_s, a_d)]
    outs = o64.ray_renderer(leaves[2], uv, leaves[0], leaves[1], albedo_diffuse=leaves[3], num_ray_diffuse=nd,
                            no_albedo=no_alb, seperate_albedo=sep, lp_scale_factor=s)
    loss = sum((o * gi.to(D)).sum() for o, gi in zip(outs, g) if gi is not None and o.requires_grad)
    grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    return [torch.zeros_like(l) if gr is None else gr for l, gr in zip(leaves, grads)]


def _tap_counts(uv, lp_shape):
    """n_t: how many (pixel, ray, tap) contributions with a non-zero weight reach texel t of grad_lp [lp_n,Hl,Wl], from the
    float32 coordinates min(u Wl, Wl - 1), min(v Hl, Hl - 1) through rnr_oracle.bilinear_taps (the kernel's expressions)."""
    from oracle import rnr_oracle as orc
    lp_n, Hl, Wl = lp_shape[:3]
    uv = uv.to(torch.float32)
    sx = (uv[..., 0, :] * float(Wl)).clamp(max=Wl - 1)
    sy = (uv[..., 1, :] * float(Hl)).clamp(max=Hl - 1)
    (x0, y0, x1, y1), (w00, w10, w01, w11) = orc.bilinear_taps(Hl, Wl, sx, sy)
    view = torch.arange(uv.shape[0]).reshape(-1, 1, 1, 1).expand_as(x0) if lp_n > 1 else torch.zeros_like(x0)
    n = torch.zeros(lp_n * Hl * Wl, dtype=torch.int64)
    for xx, yy, w in ((x0, y0, w00), (x0, y1, w10), (x1, y0, w01), (x1, y1, w11)):
        idx = ((view * Hl + yy) * Wl + xx)[w != 0]
        n += torch.bincount(idx.reshape(-1), minlength=n.numel())
    return n.reshape(lp_n, Hl, Wl)


def _hip_backward(uv, lt, lp, a_s, a_d, nd, no_alb, sep, s, g):
    """rnr_ray_renderer_backward on NaN-filled output buffers -> (grad_rays_lt, grad_lp, grad_albedo_specular,
    grad_albedo_diffuse) on the host."""
    from rnr_amd import _lib, ops
    N, R, C, H, W = lt.shape
    d = [_dev(t.contiguous()) for t in (uv, lt, lp, a_s, a_d)]
    gd = [_dev(t) for t in g]
    g_lt, g_lp, g_as, g_ad = _nan(N, R, C, H, W), _nan(*lp.shape), _nan(N, C, H, W), _nan(N, C, H, W)
    P = ops._ptr
    _lib.check(_lib.load().rnr_ray_renderer_backward(
        P(d[0]), P(d[1]), P(d[2]), lp.shape[0], lp.shape[1], lp.shape[2], P(d[3]), P(d[4]), C, R, nd, int(no_alb), int(sep), float(s),
        *[P(t) for t in gd], P(g_lt), P(g_as), P(g_ad), P(g_lp), N, H, W, ops._stream()))
    torch.cuda.synchronize()
    return g_lt.cpu(), g_lp.cpu(), g_as.cpu(), g_ad.cpu()


def _check_backward(uv, lt, lp, a_s, a_d, nd, no_alb, sep, s, g):
    """Bounds, with s = lp_scale_factor, |lp| <= 1, 0 <= lt <= 2, albedo in [0, 1], ns = R - nd, and for an output element
    M_s = |g_ltt_specular| + (|g_out| + |g_out_specular|) a_s,  M_d likewise (the heads of the adjoint with |g| for g):
      G_p: two sums, one product (3 EPS of M) and the division by the ray count: 4 EPS M / n.
      grad_rays_lt = G_p colour: the colour carries 9 EPS s (test_ray_renderer_vs_float64) and is <= s, the product 1 EPS:
        <= 14 EPS s M / n  -> 15.
      grad_albedo = G_o ltt (+ the diffuse term): ltt carries (n + 12) 2 s EPS and is <= 2 s, G_o 1 EPS, the product 1, the sum
        of the two terms 1:  2 s EPS ((|g_out| + |g_out_spec|) (ns + 15) + (|g_out| + |g_out_diff|) (nd + 15)).
      grad_lp, texel t: each contribution G_col w s carries G_p's 4 EPS, the product and the sum of G_col 2, the weight 3, two
        products 2 (11 <= 16 EPS of its magnitude), and the atomic sum of n_t of them in any order n_t EPS of the sum of their
        magnitudes A_t:  (n_t + 16) EPS A_t, A_t = the float64 adjoint with |g| in place of g (every other factor is >= 0).
        (Measured on an MI355X the worst texel of these tests reaches 0.17 of it; the ratio is printed.)  A_t = 0: exactly 0."""
    R, C = lt.shape[1], lt.shape[2]
    ns = R - nd
    ref = _oracle_grads(uv, lt, lp, a_s, a_d, nd, no_alb, sep, s, g)
    gabs = [None if t is None else t.abs() for t in g]
    mag = _oracle_grads(uv, lt, lp, a_s, a_d, nd, no_alb, sep, s, gabs)
    got_lt, got_lp, got_as, got_ad = _hip_backward(uv, lt, lp, a_s, a_d, nd, no_alb, sep, s, g)
    for name, t in (('grad_rays_lt', got_lt), ('grad_lp', got_lp), ('grad_albedo_specular', got_as), ('grad_albedo_diffuse', got_ad)):
        assert torch.isfinite(t).all(), '%s: %d values not written' % (name, int((~torch.isfinite(t)).sum()))
    z = lambda t: torch.zeros(a_s.shape, dtype=D) if t is None else t.abs().to(D)
    go, gos, god, gls, gld, _ = [z(t) if i < 5 else None for i, t in enumerate(g)]
    one = torch.ones_like(a_s, dtype=D)
    alb_s = one if no_alb else a_s.to(D)
    alb_d = one if no_alb else (a_d.to(D) if sep else a_s.to(D))
    M_s = gls + (go + gos) * alb_s
    M_d = (gld + (go + god) * alb_d) if nd > 0 else torch.zeros_like(M_s)
    tol_lt = torch.cat([(15 * EPS * s * M_s / ns)[:, None].expand(-1, ns, -1, -1, -1),
                        (15 * EPS * s * M_d / max(nd, 1))[:, None].expand(-1, nd, -1, -1, -1)], 1)
    err = (got_lt.double() - ref[0]).abs()
    assert (err <= tol_lt).all(), ('grad_rays_lt', float((err / tol_lt.clamp(min=1e-300)).max()))
    t_s, t_d = 2 * s * EPS * (go + gos) * (ns + 15), (2 * s * EPS * (go + god) * (nd + 15) if nd > 0 else torch.zeros_like(go))
    if no_alb:
        assert float(got_as.abs().max()) == 0.0 and float(got_ad.abs().max()) == 0.0
    else:
        own = sep
        err = (got_as.double() - ref[2]).abs()
        assert (err <= (t_s if own else t_s + t_d)).all(), ('grad_albedo_specular', float(err.max()))
        err = (got_ad.double() - ref[3]).abs()
        assert (err <= (t_d if own else torch.zeros_like(t_d))).all(), ('grad_albedo_diffuse', float(err.max()))
    n_t = _tap_counts(uv, lp.shape)[..., None].to(D)
    A = mag[1]
    err = (got_lp.double() - ref[1]).abs()
    tol_lp = (n_t + 16) * EPS * A
    print('grad_lp: worst error / bound = %.3f, adds per texel up to %d, %d texels untouched'
          % (float((err / tol_lp.clamp(min=1e-300))[A > 0].max()), int(n_t.max()), int((A == 0).sum())))
    assert (err <= tol_lp).all(), ('grad_lp', float((err / tol_lp.clamp(min=1e-300))[A > 0].max()))
    assert float(got_lp[A == 0].abs().max() if (A == 0).any() else 0.0) == 0.0


# ------------------------------------------------------------------------------------------------
# 1. gradients against the float64 autograd
# ------------------------------------------------------------------------------------------------
def _case_inputs(case, only_g_out):
    C, R, nd, lp_per_view, no_alb, sep, s = case
    rng = np.random.default_rng(C * 100 + R)
    N, H, W = 2, 9, 13
    uv, lt, lp, a_s, a_d = [T(t) for t in _renderer_inputs(rng, C, R, N, H, W, N if lp_per_view else 1)]
    g = [T(rng.standard_normal((N, C, H, W)).astype(np.float32)) for _ in range(5)]
    g.append(T(rng.standard_normal((N, R, C, H, W)).astype(np.float32)))
    if only_g_out:
        g = [g[0], None, None, None, None, None]
    return uv, lt, lp, a_s, a_d, nd, no_alb, sep, s, g


_case_id = lambda c: 'C%d_R%d_nd%d_lpN%d_noalb%d_sep%d_s%g' % c


@pytest.mark.parametrize('case', RENDERER_CASES, ids=_case_id)
def test_ray_renderer_backward_vs_float64_autograd(case):
    """Both kernel forms (tiled: C <= 4 and R <= 64; one lane per (pixel, channel) otherwise), R = 64 and 65, lp shared and per
    view, no_albedo, seperate_albedo, lp_scale_factor != 1, n_diff = 0, on 2 views of 9 x 13 (117-pixel views straddle the
    64-pixel workgroups) with an 11 x 23 probe and the uv -1, 0, 1, 3 / Wl, nextafter(1), -1e-7 on the first pixels.
    Upstream gradients standard normal for all six outputs.  Output buffers start as NaN.  Bounds: _check_backward."""
    _check_backward(*_case_inputs(case, False))


@pytest.mark.parametrize('case', [RENDERER_CASES[0], RENDERER_CASES[2]], ids=_case_id)
def test_ray_renderer_backward_g_out_only(case):
    """The same with an upstream gradient for `out` alone, the other five NULL (what an image loss gives), on one shape of
    each kernel form."""
    _check_backward(*_case_inputs(case, True))


def test_ray_renderer_backward_untouched_texels_stay_zero():
    """A 40 x 80 probe under 234 pixels of 2 rays: most texels receive nothing and must hold exactly 0 (grad_lp starts as NaN
    and is cleared by the entry point), the others meet the bound.  (On the 11 x 23 probe above every texel is touched.)"""
    rng = np.random.default_rng(40)
    N, H, W, C, R, nd = 2, 9, 13, 3, 2, 1
    uv, lt, lp, a_s, a_d = [T(t) for t in _renderer_inputs(rng, C, R, N, H, W, 1, lp_hw=(40, 80))]
    g = [T(rng.standard_normal((N, C, H, W)).astype(np.float32)), None, None, None, None, None]
    assert int((_tap_counts(uv, lp.shape) == 0).sum()) > 1000
    _check_backward(uv, lt, lp, a_s, a_d, nd, False, True, 1.0, g)


def test_ray_renderer_argument_errors_launch_nothing():
    """ops.ray_renderer refuses, before the entry point is called (the message is the shim's own), what would make the forward
    kernels read out of bounds: N = 2 views of 3 x 5, R = 2, C = 3; rays_uv of R + 1 rays, a probe of C + 1 channels, a probe
    batch of 3.  The same operands with matching shapes pass."""
    from rnr_amd import ops
    N, H, W, R, C = 2, 3, 5, 2, 3
    z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=DEV)
    lt, a_s = z(N, R, C, H, W), z(N, C, H, W)
    assert ops.ray_renderer(z(N, H, W, 2, R), lt, z(1, 4, 8, C), a_s)[0].shape == (N, C, H, W)
    for uv, lp in ((z(N, H, W, 2, R + 1), z(1, 4, 8, C)), (z(N, H, W, 2, R), z(1, 4, 8, C + 1)), (z(N, H, W, 2, R), z(3, 4, 8, C))):
        with pytest.raises(RuntimeError, match='ray_renderer: rays_uv .* do not match rays_lt'):
            ops.ray_renderer(uv, lt, lp, a_s)


def test_forward_entry_points_refuse_empty_sizes_and_launch_nothing():
    """rnr_ray_renderer with num_views = 0 and with lp_h = 0, rnr_texture_mapper with num_views = 0: each returns an error code,
    names the sizes in rnr_last_error, and leaves the NaN-filled output buffers as they were (no launch); the same calls with
    the true sizes succeed and write every element."""
    from rnr_amd import _lib, ops
    L, P = _lib.load(), ops._ptr
    N, H, W, R, C = 2, 3, 5, 2, 3
    rng = np.random.default_rng(5)
    uv, lt, lp, a_s, a_d = [_dev(T(t)) for t in _renderer_inputs(rng, C, R, N, H, W, 1)]
    untouched = lambda bufs: all(bool(torch.isnan(t).all()) for t in bufs)

    def render(num_views, lp_h):
        outs = [_nan(N, C, H, W) for _ in range(5)] + [_nan(N, R, C, H, W)]
        rc = L.rnr_ray_renderer(P(uv), P(lt), P(lp), 1, lp_h, lp.shape[2], P(a_s), P(a_d), C, R, 1, 0, 1, 1.0, *[P(t) for t in outs],
                                num_views, H, W, ops._stream())
        torch.cuda.synchronize()
        return rc, outs
    for num_views, lp_h in ((0, lp.shape[1]), (N, 0)):
        rc, outs = render(num_views, lp_h)
        assert rc != 0 and untouched(outs) and 'rnr_ray_renderer: bad sizes' in L.rnr_last_error().decode(), (num_views, lp_h)
    rc, outs = render(N, lp.shape[1])
    assert rc == 0 and all(bool(torch.isfinite(t).all()) for t in outs)

    tex = [_dev(T(rng.random((s, s, 4)).astype(np.float32))) for s in (8, 4)]
    ptrs, sizes = ops._level_tables(tex, [8, 4])
    uv_map = _dev(T(rng.random((N, H, W, 2)).astype(np.float32)))

    def texture(num_views):
        out = _nan(N, 4, H, W)
        rc = L.rnr_texture_mapper(P(uv_map), P(None), ptrs, sizes, 2, 4, 0, P(out), num_views, H, W, ops._stream())
        torch.cuda.synchronize()
        return rc, out
    rc, out = texture(0)
    assert rc != 0 and untouched([out]) and 'rnr_texture_mapper: bad sizes' in L.rnr_last_error().decode()
    rc, out = texture(N)
    assert rc == 0 and bool(torch.isfinite(out).all())


# ------------------------------------------------------------------------------------------------
# 2. contention
# ------------------------------------------------------------------------------------------------
def test_ray_renderer_backward_contention_2x2_probe():
    """One view of 32 x 32 pixels, 13 + 13 rays, a 2 x 2 probe: every one of the 26 624 rays adds to the same four texels
    (about 26 000 adds per texel and channel).  Same bound, one run."""
    rng = np.random.default_rng(2)
    N, H, W, R, nd, C = 1, 32, 32, 26, 13, 3
    uv = T(rng.random((N, H, W, 2, R)).astype(np.float32))
    lt = T((rng.random((N, R, C, H, W)) * 2).astype(np.float32))
    lp = T(rng.random((1, 2, 2, C)).astype(np.float32))
    a_s, a_d = [T(rng.random((N, C, H, W)).astype(np.float32)) for _ in range(2)]
    g = [T(rng.standard_normal((N, C, H, W)).astype(np.float32)) for _ in range(5)]
    g.append(T(rng.standard_normal((N, R, C, H, W)).astype(np.float32)))
    _check_backward(uv, lt, lp, a_s, a_d, nd, False, True, 1.0, g)


# ------------------------------------------------------------------------------------------------
# 3. rnr_sh_reconstruct_backward
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nb', [1, 9, 121])
@pytest.mark.parametrize('nc', [1, 3, 7])
def test_sh_reconstruct_backward_ragged_sample_counts(nb, nc):
    """grad_coeff = basis^T g against float64, sample counts that are not multiples of the 256 threads.  rnr_sh_fit's kernel
    without the scaling: a lane sums ceil(ns / 256) products in sequence, then an 8-level tree:
    (ceil(ns / 256) + 8 + 1) EPS of sum |b g| (test_sh_fit_reconstruct_ragged_sample_counts without the scaling's 3)."""
    from rnr_amd import ops
    rng = np.random.default_rng(nb * 10 + nc)
    for ns in (1, 63, 65, 257, 1000):
        basis = T((rng.random((ns, nb)) * 2 - 1).astype(np.float32))
        g = T(rng.standard_normal((ns, nc)).astype(np.float32))
        got = ops.sh_reconstruct_backward(basis.to(DEV), g.to(DEV)).cpu()
        assert got.shape == (nb, nc)
        ref = basis.double().t() @ g.double()
        mag = basis.double().abs().t() @ g.double().abs()
        assert ((got.double() - ref).abs() <= (math.ceil(ns / 256) + 9) * EPS * mag + 1e-30).all(), ns


# ------------------------------------------------------------------------------------------------
# 4. wiring: network.LightingSH -> network.RayRenderer -> loss.backward()
# ------------------------------------------------------------------------------------------------
def _wiring_scene(fix_params=False):
    import network
    rng = np.random.default_rng(4)
    N, H, W, R, nd, C = 2, 9, 13, 8, 3, 3
    l_dir = T(rng.standard_normal((3, 50)).astype(np.float32))
    l_dir = l_dir / l_dir.norm(dim=0, keepdim=True)
    coeff0 = T((rng.standard_normal((9, 3)) * 0.3 + 0.2).astype(np.float32))
    lighting = network.LightingSH(l_dir, lmax=2, init_coeff=coeff0.clone(), fix_params=fix_params, lp_recon_h=16, lp_recon_w=32).to(DEV)
    rr = network.RayRenderer(lighting, network.Interpolater())
    uv, lt, _, a_s, a_d = [T(t) for t in _renderer_inputs(rng, C, R, N, H, W, 1, lp_hw=(16, 32))]
    g = T(rng.standard_normal((N, C, H, W)).astype(np.float32))
    return lighting, rr, coeff0, uv, lt, a_s, a_d, nd, g


def test_lighting_sh_coeff_grad_through_ray_renderer():
    """coeff.grad of loss = <g, out> through LightingSH.reconstruct_lp and RayRenderer.forward, against the float64 chain
    shade64.sh_reconstruct -> shade64.ray_renderer.  Composed bound: grad_coeff[b, c] = sum_t basis[t, b] grad_lp[t, c]; the
    scatter leaves (n_t + 16) EPS A_t on grad_lp (test 1), rnr_sh_reconstruct_backward adds (ceil(512 / 256) + 9) EPS of
    sum_t |basis| |grad_lp| with |grad_lp| <= A_t:  EPS sum_t |basis[t, b]| A_t[c] (n_t + 27).
    Under torch.no_grad() the outputs carry no grad_fn and equal the grad-mode outputs bit for bit; fix_params=True builds no
    graph; a rays_uv that requires grad raises NotImplementedError."""
    from oracle import shade64 as o64
    lighting, rr, coeff0, uv, lt, a_s, a_d, nd, g = _wiring_scene()
    call = lambda uv_t: rr(a_s.to(DEV), uv_t, lt.to(DEV), lighting_idx=0, albedo_diffuse=a_d.to(DEV), num_ray_diffuse=nd,
                           seperate_albedo=True)
    outs = call(uv.to(DEV))
    assert all(o.grad_fn is not None for o in outs[:6]) and outs[6].requires_grad
    (outs[0] * g.to(DEV)).sum().backward()
    got = lighting.coeff.grad.cpu()
    assert got.shape == (1, 9, 3)
    basis = lighting.basis_val_recon.cpu()

    def chain(gg):
        c64 = coeff0.to(D).clone().requires_grad_(True)
        lp64 = o64.sh_reconstruct(basis, c64).reshape(1, 16, 32, 3)
        lp64.retain_grad()
        out = o64.ray_renderer(a_s, uv, lt, lp64, albedo_diffuse=a_d, num_ray_diffuse=nd, seperate_albedo=True)[0]
        (out * gg.to(D)).sum().backward()
        return c64.grad, lp64.grad
    ref, _ = chain(g)
    _, A = chain(g.abs())
    n_t = _tap_counts(uv, (1, 16, 32))[..., None].to(D)
    tol = EPS * torch.einsum('tb,tc->bc', basis.double().abs(), (A * (n_t + 27)).reshape(-1, 3))
    err = (got[0].double() - ref).abs()
    print('coeff.grad: worst error / bound = %.3f' % float((err / tol).max()))
    assert (err <= tol).all(), float((err / tol).max())
    with torch.no_grad():
        quiet = call(uv.to(DEV))
    assert all(o.grad_fn is None and not o.requires_grad for o in quiet)
    assert all(torch.equal(a, b) for a, b in zip(quiet, outs))
    with pytest.raises(NotImplementedError, match='rays_uv'):
        call(uv.to(DEV).requires_grad_())


def test_lighting_sh_fix_params_builds_no_graph():
    lighting, rr, _, uv, lt, a_s, a_d, nd, _ = _wiring_scene(fix_params=True)
    outs = rr(a_s.to(DEV), uv.to(DEV), lt.to(DEV), lighting_idx=0, albedo_diffuse=a_d.to(DEV), num_ray_diffuse=nd, seperate_albedo=True)
    assert all(o.grad_fn is None and not o.requires_grad for o in outs)


# ------------------------------------------------------------------------------------------------
# 5. rnr_ray_transport
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', [RAY_CASES[0], RAY_CASES[2], RAY_CASES[3]],
                         ids=lambda c: 'rays%d+%d_alb%d%d_lp%dx%d_%dx%dx%d' % (c[:2] + c[2] + c[5] + c[6:]))
def test_ray_transport_unpacks_the_fused_ray_stage(case):
    """15-pixel views across one workgroup; the product layout (c_pad 112, c_out_pad 80) on 99 pixels; both 16-lane halves full.
    raw is NaN on background pixels (what a skipped out-layer tile may leave).  Outputs (buffers start as NaN): all finite;
    background uv = -1 and rays_lt = 0; foreground uv within 4e-7 of shade64.spherical_uv of the stored directions (polynomial
    atan2 / acos: test_gpu_shade_sweep._colour_tol's angle budget without torch's own 2.4e-7 rad); rays_lt within
    fast_tanh_plus1f's 30 EPS * 2 of tanh(raw + bias) + 1; the albedos exact copies.
    Identity: ops.ray_renderer on the unpacked tensors against ops.ray_render on the packed ones, same probe: identical taps
    and identical rays_lt bits, so they differ by the blend (Taps::blend against the FMA chain, each <= 8 EPS max|lp| from
    exact: 16, times lt <= 2: 32), the products lt * colour (2 EPS of 2 max|lp|: 4) and the group sums and means
    (16-lane tree 4 + reciprocal mean 2 against four partial sums 4 + their sum 4 + division 1: 15 EPS of 2 max|lp|: 30):
    66 per group, the albedo products 4 more: 70; two groups and the final adds: 148 -> 160 EPS max|lp|."""
    from oracle import shade64 as o64
    from rnr_amd import ops
    ns, nd, alb, extra, cop, lp_hw, N, H, W = case
    rng = np.random.default_rng(ns * 100 + nd)
    net_in, raw, bias, alpha, lp = _ray_scene(rng, ns, nd, alb, extra, cop, lp_hw, N, H, W)
    R = ns + nd
    raw = raw.copy()
    raw[alpha == 0] = np.nan
    bufs = (_nan(N, H, W, 2, R), _nan(N, R, 3, H, W), _nan(N, 3, H, W), _nan(N, 3, H, W))
    d = [T(t).to(DEV) for t in (raw, bias, net_in, alpha, lp)]
    uv, lt, a_s, a_d = ops.ray_transport(d[0], d[1], d[2], d[3], ns, nd, albedo_diff_ch=alb[0], albedo_spec_ch=alb[1], out=bufs)
    assert uv is bufs[0] and lt is bufs[1]
    uvc, ltc = uv.cpu(), lt.cpu()
    assert all(torch.isfinite(t).all() for t in (uvc, ltc, a_s.cpu(), a_d.cpu()))
    bg = T(alpha) == 0
    assert bg.any() and (uvc[bg] == -1).all() and (ltc.permute(0, 3, 4, 1, 2)[bg] == 0).all()
    dirs = T(net_in)[..., :3 * R].reshape(N, H, W, R, 3).transpose(-1, -2)
    assert float((uvc.double() - o64.spherical_uv(dirs, -2))[~bg].abs().max()) <= 4e-7
    y = torch.nan_to_num(T(raw)[..., :3 * R].double()) + T(bias)[:3 * R].double()
    lt_ref = (torch.tanh(y) + 1.0).reshape(N, H, W, R, 3)
    assert float((ltc.permute(0, 3, 4, 1, 2).double() - lt_ref)[~bg].abs().max()) <= 60 * EPS
    base = 3 * R + 6
    assert torch.equal(a_s.cpu(), T(net_in)[..., base + alb[1]:base + alb[1] + 3].permute(0, 3, 1, 2))
    assert torch.equal(a_d.cpu(), T(net_in)[..., base + alb[0]:base + alb[0] + 3].permute(0, 3, 1, 2))
    unpacked = ops.ray_renderer(uv, lt, d[4][None].contiguous(), a_s, a_d, nd, False, True, 1.0)[0].cpu()
    packed = ops.ray_render(d[0], d[1], d[2], d[3], d[4], ns, nd, albedo_diff_ch=alb[0], albedo_spec_ch=alb[1]).cpu()
    assert torch.isfinite(packed).all()
    assert float((unpacked.double() - packed.double()).abs().max()) <= 160 * EPS * float(np.abs(lp).max())


# ------------------------------------------------------------------------------------------------
# 6. RNRPipeline.light_transport / LightTransport
# ------------------------------------------------------------------------------------------------
def test_light_transport_renders_any_probe_without_the_unet(monkeypatch):
    """64 x 64, two views of the small scene, skip_background_tiles=True (the out layer leaves the background tiles unwritten).
    transport.render(lp) against pipe.render under the same probe: within test 5's identity bound; a second probe renders
    without another U-Net pass (calls of UNetPlan.forward counted); pipe.render afterwards does not disturb the transport's
    tensors (it owns them); fuse_ray=True refuses."""
    from rnr_amd import scene
    from rnr_amd.pipeline import RNRPipeline
    from rnr_amd.unet import UNetPlan
    sc = scene.tiny_scene(img_size=64, nf0=4, tex_size=32, tex_ch=16, nlat=16, nlon=32, seed=0)
    mk = lambda **kw: RNRPipeline(sc['mesh'], 64, sc['textures'], sc['unet_sd'], sc['pivots_spec'], sc['pivots_diff'], sc['lp'],
                                  nf0=4, max_views=2, device=DEV, skip_background_tiles=True, **kw)
    pipe = mk()
    calls = []
    fwd = UNetPlan.forward
    monkeypatch.setattr(UNetPlan, 'forward', lambda self, *a, **k: (calls.append(1), fwd(self, *a, **k))[1])
    v = {k: T(x).to(DEV) for k, x in scene.spiral_views(64, [5, 300]).items()}
    args = (v['proj'], v['pose'], v['proj_inv'], v['R_inv'])
    tr = pipe.light_transport(*args)
    assert len(calls) == 1
    kept = [t.clone() for t in (tr.rays_uv, tr.rays_lt, tr.albedo_specular, tr.albedo_diffuse, tr.alpha)]
    assert all(torch.isfinite(t).all() for t in kept) and (tr.alpha == 0).any() and (tr.alpha > 0).any()
    lp1 = torch.as_tensor(sc['lp'], dtype=torch.float32).reshape(20, 40, 3)
    lp2 = T(np.random.default_rng(6).random((1, 20, 40, 3)).astype(np.float32))
    for lp in (lp1, lp2):
        n0 = len(calls)
        got = tr.render(lp.to(DEV))
        assert len(calls) == n0 and got.shape == (2, 3, 64, 64) and got.grad_fn is None
        pipe.set_light_probe(lp)
        ref = pipe.render(*args)
        assert float((got - ref).abs().max()) <= 160 * EPS * float(lp.abs().max())
        assert float(ref.abs().max()) > 0.05
    assert all(torch.equal(a, b) for a, b in zip(kept, (tr.rays_uv, tr.rays_lt, tr.albedo_specular, tr.albedo_diffuse, tr.alpha)))
    with pytest.raises(ValueError, match='fuse_ray'):
        mk(fuse_ray=True).light_transport(*args)


# ------------------------------------------------------------------------------------------------
# 7. the fit against the same loop in float64
# ------------------------------------------------------------------------------------------------
FIT_RTOL = 9.2e-7          # 4 x the worst step's relative deviation measured on an MI355X (2.3e-7), see the test's docstring


def _fit_scene():
    rng = np.random.default_rng(7)
    N, H, W, ns, nd, C = 2, 9, 11, 13, 13, 3
    R = ns + nd
    uv = rng.random((N, H, W, 2, R)).astype(np.float32)
    lt = (rng.random((N, R, C, H, W)) * 2).astype(np.float32)
    alpha = (rng.random((N, H, W)) > 0.25).astype(np.float32)
    uv[alpha == 0] = -1.0
    lt = lt * alpha[:, None, None]
    a_s, a_d = [rng.random((N, C, H, W)).astype(np.float32) for _ in range(2)]
    # a lighting spectrum that decays with the order, as captured probes do: the l = 0 term carries most of the energy
    crng = np.random.default_rng(7)
    coeff_true = np.zeros((9, 3), np.float32)
    coeff_true[0] = 1.5 + 0.2 * crng.standard_normal(3)
    coeff_true[1:4] = 0.2 * crng.standard_normal((3, 3))
    coeff_true[4:] = 0.1 * crng.standard_normal((5, 3))
    return [T(t) for t in (uv, lt, a_s, a_d, alpha, coeff_true)], nd


def _fit_float64(basis, uv, lt, a_s, a_d, alpha, coeff_true, nd, steps):
    """The loop of fit_sh_lighting in float64: targets at coeff_true, plain gradient descent from 0.1 with step 0.8 / L,
    L from 8 power iterations on the Hessian of the (quadratic) loss.  -> (targets, step, losses [steps + 1])."""
    from oracle import shade64 as o64
    w = (alpha > 0)[:, None].expand(-1, 3, -1, -1).to(D)
    w = w / w.sum()

    def frames(c):
        lp = o64.sh_reconstruct(basis, c).reshape(1, 16, 32, 3)
        return o64.ray_renderer(a_s, uv, lt, lp, albedo_diffuse=a_d, num_ray_diffuse=nd, seperate_albedo=True)[0]
    targets = frames(coeff_true.to(D)).detach()

    def grad(c):
        c = c.clone().requires_grad_(True)
        d = frames(c) - targets
        loss = (d * d * w).sum()
        return torch.autograd.grad(loss, c)[0], float(loss.detach())
    zero = torch.zeros(9, 3, dtype=D)
    g0, _ = grad(zero)
    v = torch.from_numpy(np.random.default_rng(8).standard_normal((9, 3)))
    for _ in range(8):                      # the loss is quadratic: H v = grad(v) - grad(0)
        v = v / v.norm()
        hv = grad(v)[0] - g0
        L, v = float(hv.norm()), hv
    step = 0.8 / L
    c = torch.full((9, 3), 0.1, dtype=D)
    losses = []
    for _ in range(steps):
        g, l = grad(c)
        losses.append(l)
        c = c - step * g
    losses.append(grad(c)[1])
    return targets, step, losses


def test_fit_sh_lighting_follows_the_float64_loop():
    """2 views of 9 x 11, 13 + 13 rays, a 16 x 32 probe, lmax 2; targets from the oracle at a known coeff*; plain SGD with step
    0.8 / L (L: 8 power iterations on the oracle's Hessian) from the 0.1 fill, 10 steps.  Required: the GPU losses fall
    monotonically, the last is below 1/50 of the first (the float64 loop itself has to show that with margin), and each is
    within FIT_RTOL of the float64 loop's loss at that step.
    FIT_RTOL is not derived: the worst step's relative deviation measured on an MI355X is 2.3e-7 (float64 losses
    0.2719 -> 0.001437, the GPU's the same to the digits shown), and 4 x that, 9.2e-7, is allowed because the arrival order of
    the atomic adds changes the rounding from run to run and box to box.  A deviation above 1e-3 would mean a bug, not
    rounding.  The deviation is printed on every run."""
    from rnr_amd.lighting import SHLighting, fit_sh_lighting
    from rnr_amd.pipeline import LightTransport
    (uv, lt, a_s, a_d, alpha, coeff_true), nd = _fit_scene()
    sh = SHLighting(2, DEV, 16, 32)
    steps = 10
    targets, step, ref = _fit_float64(sh.basis_recon.cpu(), uv, lt, a_s, a_d, alpha, coeff_true, nd, steps)
    assert all(b < a for a, b in zip(ref, ref[1:])) and ref[-1] < ref[0] / 100, ref
    tr = LightTransport(uv.to(DEV), lt.to(DEV), a_s.to(DEV), a_d.to(DEV), alpha.to(DEV), nd)
    coeff, losses = fit_sh_lighting(tr, targets.float().to(DEV), sh, steps=steps, make_optimizer=lambda p: torch.optim.SGD(p, lr=step))
    assert losses.is_cuda and losses.shape == (steps + 1,) and coeff.shape == (9, 3) and not coeff.requires_grad
    got = losses.cpu().double().tolist()
    dev = max(abs(a - b) / b for a, b in zip(got, ref))
    print('fit: float64 losses %.4g -> %.4g, GPU %.4g -> %.4g, worst relative deviation %.3g' % (ref[0], ref[-1], got[0], got[-1], dev))
    assert all(b < a for a, b in zip(got, got[1:])), got
    assert got[-1] < got[0] / 50, got
    assert dev <= FIT_RTOL, dev
