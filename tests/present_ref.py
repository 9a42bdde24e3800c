"""Reference for the presenter tests (test_present_cpu.py, test_gpu_present.py), composed from what oracle/ already pins:
float32 world view directions (rnr_oracle.view_dir_map), negated, through float32 torch.atan2 / acos
(rnr_oracle.spherical_mapping, as shade64.ray_render does for its rays), scaled and clamped in float32, the colour from
shade64.bilinear in float64, the bytes by the numpy rule of quantise().  Plus the cameras, probes and tolerances the tests share.
Test infrastructure, not product; CPU only."""
import functools

import numpy as np
import torch

EPS = 2.0 ** -24

# sizes [N,H,W] of the background cases: 2 views of 7 x 13 (odd H W: one pixel per thread), 1 view of 16 x 32 (four per thread)
SIZES = [(2, 7, 13), (1, 16, 32)]
PROBES = [(5, 9), (100, 200), (1, 1)]
CAMERAS = ['plus_x', 'seeded']
# seeds of the 'seeded' camera per size, chosen by test_present_cpu.py::test_seeded_cameras_meet_the_preconditions' rule: the
# view crosses the seam, comes near a pole, and no pixel is closer to either than the preconditions allow
SEEDS = {(2, 7, 13): 3, (1, 16, 32): 124}
POLE_MIN = 0.05         # sqrt(d.x^2 + d.z^2) of every background direction d = -view_dir
SEAM_MIN = 1e-4         # |d.z| wherever d.x < 0


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def quantise(v):
    """q(v) = saturate_u8(round_half_even(float32(v) * float32(255))), NaN -> 0, +inf -> 255, -inf -> 0; any shape -> uint8."""
    v = np.asarray(v, np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        t = v * np.float32(255)
    out = np.zeros(v.shape, np.uint8)
    fin = np.isfinite(t)
    out[fin] = np.clip(np.rint(t[fin]), 0, 255).astype(np.uint8)
    out[np.isposinf(t)] = 255
    return out              # NaN and -inf stay 0


def to_bytes(img, rgb=False):
    """float [N,3,H,W] -> the presenter's uint8 [N,H,W,3]: channel-last, B,G,R unless rgb."""
    q = quantise(np.asarray(img)).transpose(0, 2, 3, 1)
    return np.ascontiguousarray(q if rgb else q[..., ::-1])


def quantiser_values():
    """Every v = fl((k + 0.5) / 255) whose float32 product with 255 is exactly k + 0.5 (ties: even and odd k, so half-even
    differs from half-up), their float32 neighbours, and the special values."""
    k = np.arange(255)
    v = ((k + 0.5) / 255).astype(np.float32)
    tie = v * np.float32(255) == (k + 0.5).astype(np.float32)
    v, k = v[tie], k[tie]
    assert (k % 2 == 0).any() and (k % 2 == 1).any()
    one = np.float32(1)
    special = np.array([0.0, -0.0, 1.0, np.nextafter(np.float32(0), -one), -1e-3, np.nextafter(one, np.float32(2)), 1.002, -3.0, 7.0,
                        np.inf, -np.inf, np.nan], np.float32)
    return np.concatenate([v, np.nextafter(v, np.float32(-1)), np.nextafter(v, np.float32(2)), special]).astype(np.float32)


def probe(lh, lw, seed=0, n=1):
    """Light probes [n, lh, lw, 3], smooth but NOT periodic in u (a ramp of 0.3 across the seam), built the way
    test_gpu_shade_sweep._ray_scene builds its probe."""
    rng = np.random.default_rng(1000 * lh + lw + seed)
    vv, uu = np.meshgrid((np.arange(lh) + 0.5) / lh, (np.arange(lw) + 0.5) / lw, indexing='ij')
    out = []
    for i in range(n):
        lp = np.stack([0.5 + 0.2 * np.sin(2 * np.pi * (uu + (k + i) / 3)) * np.cos(np.pi * vv) + 0.3 * uu - 0.1 * k * vv
                       for k in range(3)], -1).astype(np.float32)
        out.append(lp + (rng.random(lp.shape) * 0.05).astype(np.float32))
    return np.stack(out)


def _rotation(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    return (q * np.sign(np.diag(r))).astype(np.float32)


def cameras(name, N, H, W, seed=None):
    """(proj_inv, R_inv) [N,3,3] float32.  Every K^-1 has |terms| <= 1 on x, y and z = 1, like test_gpu_shade_sweep._proj_inv (the
    camera ray has norm >= 1): the direction bounds of that module hold.
    'plus_x': looks along +x with a 90-degree field (view 1: a narrower field, off-centre): d = -view_dir = (1, -y, x) / |.| with
              |x| <= 1, |y| <= 1: u in [0.375, 0.625], sqrt(d.x^2 + d.z^2) >= 0.707.
    'seeded': a seeded rotation behind the same wide field (SEEDS): crosses the seam, comes near a pole."""
    pi = np.zeros((N, 3, 3), np.float32)
    ri = np.zeros((N, 3, 3), np.float32)
    rng = np.random.default_rng(SEEDS[(N, H, W)] if seed is None else seed)
    for i in range(N):
        f = W / 2.0 * (1.0 + 0.3 * i)
        cx, cy = W / 2.0 + 0.75 * i, H / 2.0 - 0.5 * i
        pi[i] = [[1 / f, 0, -cx / f], [0, 1 / f, -cy / f], [0, 0, 1]]
        ri[i] = [[0, 0, 1], [0, -1, 0], [1, 0, 0]] if name == 'plus_x' else _rotation(rng)
    return pi, ri


def directions(proj_inv, R_inv, H, W):
    """d = -view_dir_world, float32 [N,H,W,3] (torch.neg flips the sign bit)."""
    from oracle import rnr_oracle as orc
    world, _ = orc.view_dir_map((H, W), T(proj_inv), T(R_inv))
    return -world


def tap_coords(d, lh, lw):
    """float32 (x, y) = (min(u Wl, Wl - 1), min(v Hl, Hl - 1)) of float32 directions d [...,3]."""
    from oracle import rnr_oracle as orc
    uv = orc.spherical_mapping(d, dim=-1)
    return (uv[..., 0] * float(lw)).clamp(max=lw - 1), (uv[..., 1] * float(lh)).clamp(max=lh - 1)


def background(proj_inv, R_inv, lp, H, W):
    """test_rnr.py:386-391: lp [lp_n, Hl, Wl, 3] (lp_n = 1 or N) -> (float64 colour [N,H,W,3], float32 directions)."""
    from oracle import shade64 as o64
    d = directions(proj_inv, R_inv, H, W)
    lp = T(lp)
    x, y = tap_coords(d, lp.shape[1], lp.shape[2])
    col = torch.stack([o64.bilinear(lp[0 if lp.shape[0] == 1 else i], x[i], y[i]) for i in range(d.shape[0])])
    return col, d


@functools.lru_cache(maxsize=None)
def case(cam, size, lp_hw, per_view):
    """A background case, computed once: dict with proj_inv, R_inv, lp [lp_n,Hl,Wl,3], ref (float64 [N,H,W,3], left unchanged by
    the tests), d (float32 directions)."""
    N, H, W = size
    pi, ri = cameras(cam, N, H, W)
    lp = probe(lp_hw[0], lp_hw[1], n=N if per_view else 1)
    ref, d = background(pi, ri, lp, H, W)
    return {'proj_inv': pi, 'R_inv': ri, 'lp': lp, 'ref': ref, 'd': d}


def lp_gradient(lp):
    """Largest change of a probe between texels a bilinear footprint spans (test_gpu_shade_sweep._lp_gradient)."""
    g = 0.0
    for ax in (-3, -2):
        g = max(g, float(np.abs(np.diff(lp, axis=ax)).max()) if lp.shape[ax] > 1 else 0.0)
    return 2 * g


def colour_tol(lp, d, fused):
    """Per-pixel bound [N,H,W] on |kernel colour - background()|, derived, in the form of test_gpu_shade_sweep._colour_tol:
    (tap movement in texels) x (probe gradient per texel) + the blend's rounding.

    Direction.  Kernel and reference both compute the view direction in float32 with correctly rounded operations; each is
    within 34 EPS (vector norm) of the true unit vector (test_view_dir_map_three_views_vs_float64: camera ray 8.5, normalised
    15.5, R_inv product 9 more, normalised 31.5), the fused kernel's v_rsq normalisations within 40 EPS
    (test_shade_inputs_sweep_vs_float64): delta = 68 EPS stand-alone, 74 EPS fused.  The error is not confined to the tangent
    plane, so azimuth AND polar angle see it divided by rho = sqrt(d.x^2 + d.z^2): d(atan2(z, x)) <= delta / rho,
    d(acos(y)) = dy / sqrt(1 - y^2) <= delta / rho.
    Mapping, stand-alone (ocml atan2f / acosf vs torch's, each <= 2 ulp of pi = 2.4e-7 rad): 4.8e-7 rad; fused (fast_atan2f /
    fast_acosf vs torch's): 7e-7 / 7.4e-7 rad (_colour_tol).  u = angle / 2 pi + 1/2 with roundings on both sides 1.5e-7,
    v = angle / pi with 1.2e-7 (_colour_tol).
    Tap coordinate: Wl du + Hl dv, plus the float32 products u Wl, v Hl on both sides (Wl + Hl) 2 EPS; min(., Wl - 1) does not
    stretch it; the mapping is continuous away from the seam, where SEAM_MIN >> delta keeps the sign of z.
    Blend: float32 weights 3 EPS, 4 products + 3 adds 7 EPS (test_interpolate_bilinear_edges): 10 EPS max|lp|."""
    lh, lw = lp.shape[-3], lp.shape[-2]
    dd = d.double()
    rho = (dd[..., 0] ** 2 + dd[..., 2] ** 2).sqrt()
    delta = (74 if fused else 68) * EPS
    a_u, a_v = (7e-7, 7.4e-7) if fused else (4.8e-7, 4.8e-7)
    du = (delta / rho + a_u) / (2 * np.pi) + 1.5e-7
    dv = (delta / rho + a_v) / np.pi + 1.2e-7
    move = lw * du + lh * dv + 2 * EPS * (lw + lh)
    return move * lp_gradient(lp) + 10 * EPS * float(np.abs(lp).max())


def preconditions(d):
    """(share of pixels violating a precondition, min rho, crosses the seam?) of float32 directions d."""
    dd = d.double()
    rho = (dd[..., 0] ** 2 + dd[..., 2] ** 2).sqrt()
    bad = (rho < POLE_MIN) | ((dd[..., 0] < 0) & (dd[..., 2].abs() < SEAM_MIN))
    behind = dd[..., 0] < 0
    crosses = bool((behind & (dd[..., 2] > 0)).any() and (behind & (dd[..., 2] < 0)).any())
    return float(bad.double().mean()), float(rho.min()), crosses
