"""-m gpu: the shading kernels (shade.hip) against the float64 reference oracle/shade64.py, swept over the parameters the
kernels branch on: texture channel counts on both sides of shade_inputs_kernel's early-texture threshold (C <= 24 / C >= 28),
ray counts, sh_start_ch, texture level counts and sizes that are not powers of two, pixel counts that are not multiples of a
workgroup (ragged tails, workgroups straddling views of different cameras), padding channels, background pixels (face index
-1), uv on and just outside the texture edges, ray directions on the seam and at the poles, both ray-renderer API kernels.

Tolerances are bounds derived from the arithmetic, in units of EPS = 2^-24 (half an ulp of 1), never from a measured error:
  * every float32 +, -, *, / (correctly rounded) or sqrt adds <= 1 EPS relative;
  * normalize3_fast (v_rsq_f32, 1 ulp): 3 squares + 2 adds (5 EPS on |a|^2, 2.5 on 1/|a|), rsq 2 EPS, the product 1 EPS:
    <= 6 EPS per component, <= 10 EPS as a vector norm.  A unit vector computed from an input with vector error d over
    |a| leaves with d / |a| + 10 EPS (to first order only the part of d perpendicular to a survives normalisation).
  * a cross or dot product of unit vectors with errors d1, d2 carries d1 + d2 + 5 EPS;
  * fast_atan2f: polynomial error 3e-8 rad, rcp 1 ulp; fast_acosf: polynomial error 8e-8 rad (shade.hip);
  * fast_tanh_plus1f: exp2 and rcp 1 ulp each on |2.885 y| <= 12: <= 30 EPS absolute on tanh(y) + 1 in [0, 2];
  * a mean as a product with a reciprocal (1 ulp) instead of a division: 2 EPS.
Integer tap indices are compared bit for bit wherever they come from the same float32 expressions (interpolate_bilinear);
elsewhere their equality is implied by the value bounds (a wrong tap moves a value by a texel difference, orders above them).
"""
import math
import types

import numpy as np
import pytest
import torch

# the seeded scenes and the case tables live in oracle/shade_scenes.py, shared with the guard-band table
from oracle.shade_scenes import (RAY_CASES, RENDERER_CASES, SEAM_DIRS, SHADE_CASES, _proj_inv, _ray_scene,  # noqa: F401
                                 _renderer_inputs, _rotations, _shade_scene, _unit)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EPS = 2.0 ** -24


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def _maxerr(got, ref, mask=None):
    d = (got.detach().cpu().double() - ref.double()).abs()
    return _absmax(d[mask] if mask is not None else d)


def _absmax(t):
    """max |t| (0 for an empty tensor)."""
    return float(t.abs().max()) if t.numel() else 0.0


# ------------------------------------------------------------------------------------------------
# rnr_shade_inputs
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', SHADE_CASES, ids=lambda c: 'C%d_rays%d+%d_sh%d_L%d_%dx%dx%d' % (c[:4] + (len(c[4]),) + c[5:8]))
def test_shade_inputs_sweep_vs_float64(case):
    """rnr_shade_inputs with every optional output, vs shade64.shade_inputs.

    Bounds (module docstring; |n x t| >= 0.85 |n| by construction, the camera ray has norm >= 1):
      normal N: 10; B = normalize(N x T): (10 + 2 + 5) / 0.85 + 10 = 30; T' = normalize(B x N): 30 + 10 + 5 + 10 = 55.
      view dir: camera ray 3 EPS * 2 per component (10 as a vector), normalised 20; R_inv product 10 more, normalised: 40.
      tangent-space view: dots 55 + 30 + 10 + 40 + 5, normalised: 150.
      specular ray: s = 2 p.v: 2 (150 + 3) = 306; l = s p - v: 306 + 150 + 5 = 461, normalised 471 (x alpha, exact);
        d = TBN l: 95 (columns) + 471 + 5, normalised: 581 -> 600 EPS.  Diffuse ray d = TBN p: 95 + 5 + 10 -> 120 EPS.
      SH basis (from the view dir normalised once more: 50): 1.09 * 2 * 50 + 3 -> 120 EPS.
      texture channels, L levels of |texel| <= 1: weights 3, blend 4 products + 3 adds (7 EPS of sum |I w| <= 1), level
        sum (L - 1) adds of magnitude <= L: (7 L + L^2) EPS; SH channels: that times |sh| <= 1.1, plus 120 L (the basis
        error times |texture| <= L) and the product's rounding (1.1 L): 1.1 (7 L + L^2) + 122 L.
      rays_uv from the kernel's own float32 directions (net_in): ocml atan2f / acosf (<= 2 ulp of <= pi: 4.8e-7 rad), / pi
        and + 0.5: (4.8e-7 / pi + 2 * 6e-8) -> 4e-7 absolute.
    Exact: the copied normal, the padding channels (0), neural_img == the texture channels of net_in bit for bit."""
    from oracle import shade64 as o64
    from rnr_amd import ops
    C, ns, nd, sh_start, levels, N, H, W, extra = case
    rng = np.random.default_rng(C * 1000 + ns * 10 + nd)
    sc = _shade_scene(rng, C, levels, N, H, W)
    ps = T(_unit(rng, ns).T.astype(np.float32)) if ns else torch.zeros(3, 0)
    pd = T(_unit(rng, nd).T.astype(np.float32)) if nd else torch.zeros(3, 0)
    ps[2] = ps[2].abs()
    pd[2] = pd[2].abs()
    R = ns + nd
    c_in = 3 * R + 6 + C
    c_pad = (c_in + 3) // 4 * 4 + extra
    d = {k: T(v).to(DEV) for k, v in sc.items() if k != 'tex'}
    gb = {'face_index_map': d['fim'], 'alpha': d['alpha'], 'uv_map': d['uv'], 'normal_map': d['normal']}
    tex = [T(t).to(DEV) for t in sc['tex']]
    net_in = torch.full((N, H, W, c_pad), float('nan'), device=DEV)
    neural = torch.full((N, C, H, W), float('nan'), device=DEV)
    out = ops.shade_inputs(gb, types.SimpleNamespace(num_faces=len(sc['tangents'])), d['proj_inv'], d['R_inv'], tex, ps, pd,
                           sh_start, c_pad=c_pad, want_rays_uv=True, want_sh=True, net_in=net_in, tangents=d['tangents'],
                           neural_img=neural)
    torch.cuda.synchronize()
    ni = net_in.cpu()
    assert not torch.isnan(ni).any() and _absmax(ni[..., c_in:]) == 0.0
    nimg = neural.cpu()
    assert not torch.isnan(nimg).any(), 'neural_img left unwritten at %d of %d values' % (int(torch.isnan(nimg).sum()), nimg.numel())
    assert torch.equal(nimg, ni[..., 3 * R + 6:c_in].permute(0, 3, 1, 2))
    ref = o64.shade_inputs(T(sc['fim']), T(sc['alpha']), T(sc['uv']), T(sc['normal']), T(sc['tangents']), T(sc['proj_inv']),
                           T(sc['R_inv']), [T(t) for t in sc['tex']], ps, pd, sh_start)
    rn = ref['net_in']
    L = len(levels)
    assert _maxerr(ni[..., :3 * ns], rn[..., :3 * ns]) <= 600 * EPS
    assert _maxerr(ni[..., 3 * ns:3 * R], rn[..., 3 * ns:3 * R]) <= 120 * EPS
    assert torch.equal(ni[..., 3 * R:3 * R + 3], T(sc['normal']))
    assert _maxerr(ni[..., 3 * R + 3:3 * R + 6], rn[..., 3 * R + 3:3 * R + 6]) <= 40 * EPS
    tol_tex = torch.full((C,), (7 * L + L * L) * EPS)
    if sh_start >= 0:
        tol_tex[sh_start:sh_start + 9] = (1.1 * (7 * L + L * L) + 122 * L) * EPS
    err_tex = (ni[..., 3 * R + 6:c_in].double() - rn[..., 3 * R + 6:]).abs().amax(dim=(0, 1, 2))
    assert (err_tex <= tol_tex).all(), (err_tex / EPS, tol_tex / EPS)
    assert _maxerr(out['sh_basis_map'], ref['sh_basis_map']) <= 120 * EPS
    # rays_uv vs the spherical mapping of the kernel's own directions
    dirs_k = ni[..., :3 * R].reshape(N, H, W, R, 3).transpose(-1, -2)
    a = T(sc['alpha']).double()[..., None, None]
    uv_ref = o64.spherical_uv(dirs_k, -2) * a - (a == 0).double()
    assert _maxerr(out['rays_uv'], uv_ref) <= 4e-7


# ------------------------------------------------------------------------------------------------
# rnr_ray_render / rnr_ray_weights
# ------------------------------------------------------------------------------------------------
def _lp_gradient(lp):
    """Largest change of the probe between texels a bilinear footprint spans (the Lipschitz constant per texel)."""
    g = 0.0
    for ax in (0, 1):
        g = max(g, float(np.abs(np.diff(lp, axis=ax)).max()) if lp.shape[ax] > 1 else 0.0)
    return 2 * g


def _colour_tol(lp):
    """Env-map colour difference between the kernel's uv (fast_atan2f / fast_acosf, rcp, FMA) and the reference's float32
    torch.atan2 / acos uv of the same direction.  Angle: polynomial 3e-8, rcp and product 1.8e-7 (a <= 1), pi/2 - r and
    pi - r roundings 2.4e-7, torch's atan2f 2.4e-7: 7e-7 rad; |du| <= 7e-7 / 2pi + roundings of u on both sides (1.5e-7)
    <= 2.6e-7.  acos: polynomial 8e-8, sqrt and product 3e-7, pi - r 1.2e-7, torch's acosf 2.4e-7: 7.4e-7 rad;
    |dv| <= 7.4e-7 / pi + 1.2e-7 <= 3.6e-7.  Both -> 5e-7; the tap
    coordinate moves by Wl |du| + Hl |dv| texels, the bilinear colour by that times the per-texel gradient (the mapping is
    continuous away from the seam, where the sign bits decide alike), plus the blend's own 8 EPS of max |lp|."""
    lh, lw = lp.shape[0], lp.shape[1]
    return (lw + lh) * 5e-7 * _lp_gradient(lp) + 8 * EPS * float(np.abs(lp).max())


@pytest.mark.parametrize('case', RAY_CASES, ids=lambda c: 'rays%d+%d_alb%d%d_lp%dx%d_%dx%dx%d' % (c[:2] + c[2] + c[5] + c[6:]))
def test_ray_render_sweep_vs_float64(case):
    """rnr_ray_render vs shade64.ray_render (the same float32 directions through torch.atan2 / acos, float64 after the taps).

    Per ray (tanh + 1) * colour: 30 EPS * |colour| + 2 * colour tolerance + 2 EPS; the 16-lane sums (4 adds, 4 EPS of the
    sum of |terms| <= 2 n max|lp|) and the reciprocal mean (2 EPS) keep the bound per group at 2 (colour tol) + 40 EPS
    max|lp|; times albedo <= 1, two groups and the final add: 4 (colour tol) + 82 EPS max|lp|.
    The first pixels carry seam (z = +-0, x < 0) and pole directions on every ray: their env-map taps are column W-1 / 0
    exactly as torch.atan2's sign-bit semantics put them."""
    from oracle import shade64 as o64
    from rnr_amd import ops
    ns, nd, alb, extra, cop, lp_hw, N, H, W = case
    rng = np.random.default_rng(ns * 100 + nd)
    net_in, raw, bias, alpha, lp = _ray_scene(rng, ns, nd, alb, extra, cop, lp_hw, N, H, W)
    img = torch.full((N, 3, H, W), float('nan'), device=DEV)
    ops.ray_render(T(raw).to(DEV), T(bias).to(DEV), T(net_in).to(DEV), T(alpha).to(DEV), T(lp).to(DEV), ns, nd,
                   albedo_diff_ch=alb[0], albedo_spec_ch=alb[1], image=img)
    ref, _, _ = o64.ray_render(T(raw), T(bias), T(net_in), T(alpha), T(lp), ns, nd, alb[0], alb[1])
    tol = 4 * _colour_tol(lp) + 82 * EPS * float(np.abs(lp).max())
    got = img.cpu()
    assert not torch.isnan(got).any()
    seam = torch.zeros(N * H * W, dtype=torch.bool)
    seam[:len(SEAM_DIRS)] = True
    seam = seam.reshape(N, 1, H, W).expand_as(got)
    assert _maxerr(got, ref, seam) <= tol, 'seam / pole directions: %g > %g' % (_maxerr(got, ref, seam), tol)
    assert _maxerr(got, ref) <= tol
    assert _absmax(got.permute(0, 2, 3, 1)[T(alpha) == 0]) == 0.0


@pytest.mark.parametrize('case', [c for c in RAY_CASES if c[1] <= 15],
                         ids=lambda c: 'rays%d+%d_alb%d%d_lp%dx%d_%dx%dx%d' % (c[:2] + c[2] + c[5] + c[6:]))
def test_ray_weights_sweep_vs_float64_and_ray_render(case):
    """rnr_ray_weights: W vs shade64.ray_weights (bound: colour tolerance + 4 EPS max|lp| from the product with the albedo and
    the reciprocal mean), the padding columns up to c_w exactly 0 (the buffer starts as NaN), and the frame identity
    image = sum_r (tanh(y + b) + 1) W summed on the host in float64 against rnr_ray_render on the same inputs: the same taps
    (same code), so the two differ by fast_tanh_plus1f (30 EPS) and their roundings (2 + 2 products, reciprocal mean 2,
    16-lane sum 4): per group <= 40 EPS * 2 max|lp|, 2 groups + add: 162 EPS max|lp|."""
    from oracle import shade64 as o64
    from rnr_amd import ops
    ns, nd, alb, extra, cop, lp_hw, N, H, W = case
    rng = np.random.default_rng(ns * 100 + nd)
    net_in, raw, bias, alpha, lp = _ray_scene(rng, ns, nd, alb, extra, cop, lp_hw, N, H, W)
    R = ns + nd
    c_w = (3 * R + 3) // 4 * 4 + 4
    w = torch.full((N, H, W, c_w), float('nan'), device=DEV)
    ops.ray_weights(T(net_in).to(DEV), T(alpha).to(DEV), T(lp).to(DEV), ns, nd, c_w, albedo_diff_ch=alb[0],
                    albedo_spec_ch=alb[1], out=w)
    wc = w.cpu()
    assert float(wc[..., 3 * R:].abs().max()) == 0.0           # NaN compares false: any unwritten column fails here
    assert not torch.isnan(wc).any()
    ref = o64.ray_weights(T(net_in), T(alpha), T(lp), ns, nd, alb[0], alb[1])
    lpmax = float(np.abs(lp).max())
    assert _maxerr(wc[..., :3 * R], ref) <= _colour_tol(lp) + 4 * EPS * lpmax
    img = ops.ray_render(T(raw).to(DEV), T(bias).to(DEV), T(net_in).to(DEV), T(alpha).to(DEV), T(lp).to(DEV), ns, nd,
                         albedo_diff_ch=alb[0], albedo_spec_ch=alb[1]).cpu()
    y = T(raw[..., :3 * R]).double() + T(bias[:3 * R]).double()
    host = ((torch.tanh(y) + 1.0) * wc[..., :3 * R].double()).reshape(N, H, W, R, 3).sum(-2).permute(0, 3, 1, 2)
    assert _maxerr(img, host) <= 162 * EPS * lpmax


# ------------------------------------------------------------------------------------------------
# drop-in operators
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C,levels,sh_start', [(1, [9, 4], None), (3, [33, 17, 9], None), (9, [20, 11, 6, 3, 2], 0),
                                               (30, [37, 18, 9], 21), (30, [37, 18, 9], None)])
def test_texture_mapper_channels_vs_float64(C, levels, sh_start):
    """rnr_texture_mapper (the any-channel kernel of TextureMapper) for C = 1, 3, 9, 30, SH on and off, 2 views of 7 x 13 with
    edge uv.  Bound: (7 L + L^2) EPS (blend and level sum of |texel| <= 1) + L EPS |sh| for the SH product (sh given)."""
    from oracle import shade64 as o64
    from rnr_amd import ops
    rng = np.random.default_rng(C * 7 + len(levels))
    sc = _shade_scene(rng, C, levels, 2, 7, 13)
    tex = [T(t) for t in sc['tex']]
    sh = T((rng.random((2, 7, 13, 9)) * 2 - 1).astype(np.float32)) if sh_start is not None else None
    out = ops.texture_mapper([t.to(DEV) for t in tex], T(sc['uv']).to(DEV), sh.to(DEV) if sh is not None else None,
                             sh_start if sh_start is not None else 3)
    ref = o64.texture_mapper(tex, T(sc['uv']), sh, sh_start if sh_start is not None else -1)
    L = len(levels)
    assert _maxerr(out, ref) <= (7 * L + L * L + L) * EPS
    if C == 30 and sh_start is not None:           # and through the drop-in module (TextureMapper(37, 30, 3): 37, 18, 9)
        import network
        tm = network.TextureMapper(37, 30, 3, apply_sh=True)
        for p, t in zip(tm.textures, tex):
            p.data.copy_(t[None])
        tm.to(DEV)
        got = tm(T(sc['uv']).to(DEV), sh.to(DEV), sh_start_ch=sh_start)
        assert _maxerr(got, ref) <= (7 * L + L * L + L) * EPS


def _frames(rng, n):
    """Orthonormal float32 TBN frames [n,3,3]."""
    return _rotations(rng, n)


@pytest.mark.parametrize('reflect', [True, False])
@pytest.mark.parametrize('R', [1, 13, 32])
def test_ray_sampler_vs_float64(reflect, R):
    """rnr_ray_sampler (RaySampler.forward; correctly rounded normalize3), alpha 0 and 1, on 3 x 5 x 7 pixels.
    Bounds: reflect l = normalize(2 (p.v) p - v): 2 (3 + 1) + 3 + 5 (vector), normalised with a correctly rounded sqrt and
    divisions (4 EPS a component, 7 as a vector): 23; d = TBN l: 23 + 5 + 7 -> 40 EPS (diffuse: 20).  uv from the kernel's
    own directions: 4e-7 (ocml atan2f / acosf, see test_shade_inputs_sweep_vs_float64)."""
    from oracle import shade64 as o64
    from rnr_amd import ops
    rng = np.random.default_rng(R * 2 + reflect)
    N, H, W = 3, 5, 7
    piv = _unit(rng, R).T.astype(np.float32)
    piv[2] = np.abs(piv[2])
    tbn = _frames(rng, N * H * W).reshape(N, H, W, 3, 3)
    vt = _unit(rng, N, H, W).astype(np.float32)
    alpha = (rng.random((N, H, W, 1)) > 0.3).astype(np.float32)
    d, uv, dt = ops.ray_sampler(reflect, T(piv), T(tbn).to(DEV), T(vt).to(DEV), T(alpha).to(DEV))
    rd, _, rdt = o64.ray_sampler(reflect, T(piv), T(tbn), T(vt), T(alpha)[..., 0])
    assert _maxerr(d, rd) <= (40 if reflect else 20) * EPS
    if reflect:
        assert _maxerr(dt, rdt) <= 23 * EPS
    a = T(alpha).double()[..., None]
    assert _maxerr(uv, o64.spherical_uv(d.cpu(), -2) * a - (a == 0).double()) <= 4e-7


@pytest.mark.parametrize('case', RENDERER_CASES, ids=lambda c: 'C%d_R%d_nd%d_lpN%d_noalb%d_sep%d_s%g' % c)
def test_ray_renderer_vs_float64(case):
    """rnr_ray_renderer through network.RayRenderer, both kernels, every output incl. rays_color.  The taps come from the same
    float32 products u * Wl, v * Hl on both sides.  Bounds with s = lp_scale_factor, |lp| <= 1, |lt| <= 2, albedo <= 1:
    colour: (lp * s) 1 EPS, weights 3, 4 products + 3 adds: 9 EPS s; ltt over a group of n rays: (n + 1) EPS of
    sum |lt colour| <= 2 n s plus 2 * 9 EPS s, division 1 EPS: (n + 12) 2 s EPS; out: times albedo (1 EPS), the sum of the
    two groups (1 EPS)."""
    import network
    from oracle import shade64 as o64
    C, R, nd, lp_per_view, no_alb, sep, s = case
    rng = np.random.default_rng(C * 100 + R)
    N, H, W = 2, 9, 13                       # 117 pixels a view: ragged 64-pixel workgroups straddling the views
    uv, lt, lp, a_s, a_d = _renderer_inputs(rng, C, R, N, H, W, N if lp_per_view else 1)
    rr = network.RayRenderer(None, network.Interpolater())
    out = rr(T(a_s).to(DEV), T(uv).to(DEV), T(lt).to(DEV), lp=T(lp).to(DEV), albedo_diffuse=T(a_d).to(DEV), num_ray_diffuse=nd,
             no_albedo=no_alb, seperate_albedo=sep, lp_scale_factor=s)
    ref = o64.ray_renderer(T(a_s), T(uv), T(lt), T(lp), albedo_diffuse=T(a_d), num_ray_diffuse=nd, no_albedo=no_alb,
                           seperate_albedo=sep, lp_scale_factor=s)
    n = max(R - nd, nd)
    t_col, t_lt = 9 * EPS * s, (n + 12) * 2 * s * EPS
    tols = [2 * t_lt + 3 * EPS * 4 * s, t_lt + 2 * EPS * 2 * s, t_lt + 2 * EPS * 2 * s, t_lt, t_lt, t_col]
    for k, (a, b, tol) in enumerate(zip(out[:6], ref, tols)):
        assert _maxerr(a, b) <= tol, (k, _maxerr(a, b), tol)


def test_ray_renderer_kernels_agree():
    """The tiled kernel (C <= 4, R <= 64) and the one-lane-per-(pixel, channel) kernel on the same data: channels 0..2 of a C = 5
    call (generic) against a C = 3 call (tiled).  Each is within the float64 bound of test_ray_renderer_vs_float64; so they
    are within twice that of each other."""
    from rnr_amd import ops
    rng = np.random.default_rng(5)
    N, H, W, R, nd = 2, 9, 13, 26, 13
    uv, lt, lp, a_s, a_d = _renderer_inputs(rng, 5, R, N, H, W, 1)
    run = lambda c: ops.ray_renderer(T(uv).to(DEV), T(lt[:, :, :c].copy()).to(DEV), T(lp[..., :c].copy()).to(DEV),
                                     T(a_s[:, :c].copy()).to(DEV), T(a_d[:, :c].copy()).to(DEV), nd, False, True, 1.0)
    o3, o5 = run(3), run(5)
    t_lt = (13 + 12) * 2 * EPS
    for k, tol in enumerate([2 * t_lt + 12 * EPS, t_lt + 4 * EPS, t_lt + 4 * EPS, t_lt, t_lt, 9 * EPS]):
        a, b = o3[k].cpu(), (o5[k][:, :, :3] if k == 5 else o5[k][:, :3]).cpu()
        assert _maxerr(a, b) <= 2 * tol, k


def test_face_tangents_tbn_map_edge_faces_vs_float64():
    """get_TBN_map (drop-in: face_tangents + tbn_map kernels, correctly rounded normalize3) on faces with mirrored UV
    (negative determinant: clamped to 1e-8, the tangent keeps f > 0), zero-area UV triangles (all three texcoords equal: a
    zero tangent and zero T, B — exactly, on both sides — or collinear: f = 1e8) and face index -1.
    Bound per face: the tangent's difference vector d2y e1 - d1y e2 carries 4 EPS of k = |d2y||e1| + |d1y||e2|, so its
    direction (k / |.|) 4 EPS + 2 (the product with f) + 7 (normalisation); then B = normalize(N x T) and T' = normalize(B x N) as in
    test_shade_inputs_sweep_vs_float64 with |n x t| >= 0.85 |n| and 7 EPS normalisations."""
    import render
    from oracle import shade64 as o64
    rng = np.random.default_rng(11)
    nf = 24
    fv = rng.standard_normal((nf, 3, 3)).astype(np.float32)
    fvt = rng.random((nf, 3, 2)).astype(np.float32)
    fvt[4:8, :, 0] = 1.0 - fvt[4:8, :, 0]                      # mirrored islands
    fvt[8:10] = fvt[8:10, :1]                                   # all three texcoords equal: zero tangent
    fvt[10:12, 2] = 2 * fvt[10:12, 1] - fvt[10:12, 0]           # collinear texcoords: (near-)zero determinant
    N, H, W = 2, 6, 11
    fim = rng.integers(0, nf, (N, H, W)).astype(np.int32)
    fim[:, 0, :3] = -1
    fim[0, 1, :2] = 8                                           # zero-tangent faces on some pixels
    tan64 = o64.face_tangents(T(fv), T(fvt)).numpy()
    t = tan64[fim % nf]
    r = _unit(rng, N, H, W)
    perp = r - (r * t).sum(-1, keepdims=True) * t
    perp /= np.linalg.norm(perp, axis=-1, keepdims=True)
    nrm = (perp + 0.6 * (rng.random((N, H, W, 1)) * 2 - 1) * t).astype(np.float32)
    tbn = render.get_TBN_map(T(nrm).to(DEV), T(fim).to(DEV), faces_v=T(fv).to(DEV), faces_texcoord=T(fvt).to(DEV), plain=True)
    ref = o64.tbn_map(T(nrm), T(fim), T(tan64))
    e1, e2 = fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 0]
    d1, d2 = fvt[:, 1] - fvt[:, 0], fvt[:, 2] - fvt[:, 0]
    vec = d2[:, 1:2].astype(np.float64) * e1 - d1[:, 1:2] * e2
    k = np.abs(d2[:, 1]) * np.linalg.norm(e1, axis=1) + np.abs(d1[:, 1]) * np.linalg.norm(e2, axis=1)
    nz = np.linalg.norm(vec, axis=1) > 0
    tau = np.where(nz, 4 * k / np.maximum(np.linalg.norm(vec, axis=1), 1e-30) + 9, 0.0)      # EPS units, per face
    assert (tau[nz] < 1e4).all()                                                            # well-conditioned data
    tp = T(tau[fim % nf])
    b_tol = (7 + tp + 5) / 0.85 + 7
    t_tol = b_tol + 7 + 5 + 7
    err = (tbn.cpu().double() - ref).abs()
    assert (err[..., 2] <= 7 * EPS).all()
    assert (err[..., 1].amax(-1) <= b_tol * EPS).all()
    assert (err[..., 0].amax(-1) <= t_tol * EPS).all()
    zero = T(np.isin(fim % nf, [8, 9]))
    assert zero.any() and float(tbn.cpu()[zero][..., :2].abs().max()) == 0.0


def test_view_dir_map_three_views_vs_float64():
    """get_view_dir_map with 3 different cameras in one call (view_dir_map_kernel, correctly rounded normalize3): camera ray
    3 EPS * 2 on x and y (z = -1 exactly): 8.5 as a vector, normalised (7): 15.5 <= 17; R_inv product 3 EPS * sqrt 3 per
    component (9 as a vector), normalised: 31.5 <= 34 EPS."""
    import camera
    from oracle import shade64 as o64
    rng = np.random.default_rng(3)
    H, W = 7, 10
    pi, ri = _proj_inv(rng, 3, H, W), _rotations(rng, 3)
    vd, vdc = camera.get_view_dir_map((H, W), T(pi).to(DEV), T(ri).to(DEV))
    rvd, rvdc = o64.view_dir_map((H, W), T(pi), T(ri))
    assert _maxerr(vdc, rvdc) <= 17 * EPS and _maxerr(vd, rvd) <= 34 * EPS


def test_interpolate_bilinear_edges():
    """rnr_interpolate_bilinear at x, y in {-0.0, 0, W-1, just beyond W-1, negative, interior}: taps bit-exact with the float32
    expressions of misc.py (rnr_oracle.bilinear_taps), values within 3 (weights) + 7 (blend) EPS of float64 (|data| <= 1)."""
    from oracle import rnr_oracle as orc
    from oracle import shade64 as o64
    from rnr_amd import ops
    rng = np.random.default_rng(9)
    H, W, C = 6, 9, 5
    data = (rng.random((H, W, C)) * 2 - 1).astype(np.float32)
    vals = lambda n: np.array([-0.0, 0.0, n - 1, np.nextafter(np.float32(n - 1), np.float32(n)), -0.5, -np.float32(1e-7), 2.5,
                               np.nextafter(np.float32(n - 1), np.float32(0)), 1.0, n - 0.5], np.float32)
    xs, ys = np.meshgrid(vals(W), vals(H), indexing='ij')
    x, y = T(xs.ravel().copy()), T(ys.ravel().copy())
    out, taps = ops.interpolate_bilinear(T(data).to(DEV), x.to(DEV), y.to(DEV), want_taps=True)
    (x0, y0, x1, y1), _ = orc.bilinear_taps(H, W, x, y)
    assert torch.equal(taps.cpu(), torch.stack([x0, y0, x1, y1], -1).int())
    assert _maxerr(out, o64.bilinear(T(data), x, y)) <= 10 * EPS


@pytest.mark.parametrize('nb', [1, 9, 121])
@pytest.mark.parametrize('nc', [1, 3, 7])
def test_sh_fit_reconstruct_ragged_sample_counts(nb, nc):
    """rnr_sh_fit / rnr_sh_reconstruct with sample counts that are not multiples of the 256-thread fit or the 64-row
    reconstruction tile.  sh_fit: a lane sums ceil(ns / 256) products in sequence, then an 8-level tree and the 4 pi / ns
    scaling (3 roundings): (ceil(ns / 256) + 8 + 4) EPS of (4 pi / ns) sum |s b|.  sh_reconstruct: nb products and adds in
    sequence: (nb + 1) EPS of sum |b c|.  Too many basis functions / channels for the LDS tile raise before any launch."""
    from oracle import shade64 as o64
    from rnr_amd import _lib, ops
    rng = np.random.default_rng(nb * 10 + nc)
    for ns in (1, 63, 65, 257, 1000):
        basis = T((rng.random((ns, nb)) * 2 - 1).astype(np.float32))
        samples = T((rng.random((ns, nc)) * 2 - 1).astype(np.float32))
        coeff = T((rng.random((nb, nc)) * 2 - 1).astype(np.float32))
        fit = ops.sh_fit(samples.to(DEV), basis.to(DEV))
        mag = (basis.double().abs().t() @ samples.double().abs()) * (4 * math.pi / ns)
        assert ((fit.cpu().double() - o64.sh_fit(samples, basis)).abs() <= (math.ceil(ns / 256) + 12) * EPS * mag + 1e-30).all(), ns
        rec = ops.sh_reconstruct(basis.to(DEV), coeff.to(DEV))
        mag = basis.double().abs() @ coeff.double().abs()
        assert ((rec.cpu().double() - o64.sh_reconstruct(basis, coeff)).abs() <= (nb + 1) * EPS * mag + 1e-30).all(), ns
    if nb == 121:
        with pytest.raises(_lib.RnrError, match='LDS'):
            ops.sh_reconstruct(torch.zeros(100, 121, device=DEV), torch.zeros(121, 100, device=DEV))
