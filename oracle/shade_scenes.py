"""The seeded scenes and case tables of the shading kernels' tests (tests/test_gpu_shade_sweep.py sweeps them against float64,
oracle/shade_guard_cases.py builds the guard-band table on them).  Plain numpy; nothing here touches the library."""
import numpy as np


def _unit(rng, *shape):
    v = rng.standard_normal(shape + (3,))
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _rotations(rng, n):
    out = []
    for _ in range(n):
        q, r = np.linalg.qr(rng.standard_normal((3, 3)))
        out.append(q * np.sign(np.diag(r)))
    return np.stack(out).astype(np.float32)


def _proj_inv(rng, n, H, W):
    """K^-1 of pinhole cameras with focal length >= max(H, W): every term of -(K^-1 (col + .5, row + .5, 1)) is <= 1 in
    magnitude and the z component is -1, so the camera ray has norm >= 1 and its three-term sums carry <= 3 EPS * 2."""
    out = np.zeros((n, 3, 3), np.float32)
    for i in range(n):
        f = max(H, W) * (1.0 + rng.random())
        cx, cy = W * rng.random(), H * rng.random()
        out[i] = [[1 / f, 0, -cx / f], [0, 1 / f, -cy / f], [0, 0, 1]]
    return out


# (C, n_spec, n_diff, sh_start_ch, texture level sizes, N, H, W, extra padding channels); 3 (ns + nd) + 6 = 0 mod 4
SHADE_CASES = [
    (4, 1, 1, -1, [5], 3, 7, 9, 0),                             # smallest rays, 1 level; 189 pixels: ragged tail, 3 views
    (16, 13, 13, 6, [37, 19, 10, 2], 3, 7, 9, 4),               # the product's ray layout, uneven levels down to S = 2
    (24, 5, 1, 0, [40, 31, 23, 17, 11, 7, 3, 2], 2, 11, 13, 0),  # C = 24: the last early-texture case; 8 levels
    (28, 2, 0, 19, [45], 1, 10, 10, 8),                         # C = 28: the first fallback case; no diffuse rays
    (48, 16, 14, 39, [30, 21, 12, 5], 2, 9, 9, 12),             # fallback loop, SH on the last 9 channels
    (24, 32, 30, 15, [16, 8], 3, 5, 7, 0),                      # MAX_RAYS specular rays; 105 pixels
    (28, 13, 13, 0, [64, 32, 16, 8], 2, 16, 16, 12),            # power-of-two levels, whole workgroups only
]


def _shade_scene(rng, C, levels, N, H, W, nf=7):
    """A G-buffer of random maps: faces with random unit tangents, normals at >= ~60 degrees from their face's tangent
    (|n x t| >= 0.85 |n|: the cross products stay well conditioned), background pixels with face index -1 (wrapping to the
    last face, render.py:152) and alpha 0, uv uniform plus exact edge values."""
    tan = _unit(rng, nf).astype(np.float32)
    fim = rng.integers(0, nf, (N, H, W)).astype(np.int32)
    bg = rng.random((N, H, W)) < 0.25
    fim[bg] = -1
    alpha = (~bg).astype(np.float32)
    t = tan[fim % nf].astype(np.float64)
    r = _unit(rng, N, H, W)
    perp = r - (r * t).sum(-1, keepdims=True) * t
    perp /= np.linalg.norm(perp, axis=-1, keepdims=True)
    nrm = (perp + 0.6 * (rng.random((N, H, W, 1)) * 2 - 1) * t) * (0.5 + 1.5 * rng.random((N, H, W, 1)))
    uv = rng.random((N, H, W, 2)).astype(np.float32)
    s0 = levels[0]
    special = np.array([0.0, 1.0, 1.0 / (s0 - 1), (s0 - 2) / (s0 - 1), np.nextafter(np.float32(1), np.float32(2)),
                        -np.float32(1e-7), 0.5], np.float32)
    flat = uv.reshape(-1, 2)
    k = min(flat.shape[0], 4 * len(special))
    idx = rng.choice(flat.shape[0], k, replace=False)
    flat[idx, 0] = np.resize(special, k)
    flat[idx, 1] = np.resize(special[::-1], k)
    tex = [(rng.random((s, s, C)) * 2 - 1).astype(np.float32) for s in levels]
    return {'fim': fim, 'alpha': alpha, 'uv': uv, 'normal': nrm.astype(np.float32), 'tangents': tan, 'tex': tex,
            'proj_inv': _proj_inv(rng, N, H, W), 'R_inv': _rotations(rng, N)}


# (n_spec, n_diff, (albedo_diff_ch, albedo_spec_ch), extra c_pad, c_out_pad or None, (lp_h, lp_w), N, H, W)
RAY_CASES = [
    (1, 0, (0, 3), 0, None, (2, 3), 3, 3, 5),            # 15-pixel views: one 32-pixel workgroup spans three views
    (16, 0, (3, 0), 4, None, (100, 200), 2, 6, 6),       # 72 pixels: ragged; albedo channels swapped
    (13, 13, (0, 3), 0, 80, (16, 32), 1, 9, 11),         # the product's rays and c_out_pad 80 (c_pad 92) on 99 pixels
    (16, 16, (3, 0), 8, 100, (7, 13), 3, 4, 5),          # both 16-lane halves full; 20-pixel views
    (7, 3, (0, 3), 12, 36, (100, 200), 2, 7, 9),
    (16, 15, (0, 3), 0, None, (9, 17), 2, 5, 7),         # ray_weights' limit (nd <= 15)
]

SEAM_DIRS = [(-1.0, 0.0, -0.0), (-1.0, 0.0, 0.0), (-0.6, 0.8, -0.0), (0.0, 1.0, 0.0), (0.0, -1.0, 0.0), (-0.0, 1.0, 0.0),
             (-0.0, -1.0, -0.0), (1.0, 0.0, -0.0)]


def _ray_scene(rng, ns, nd, alb, extra, cop, lp_hw, N, H, W):
    """net_in with unit ray directions (seam / pole directions on every ray of the first pixels), albedo in [0, 1] at the
    given channels, background pixels, a light probe that is smooth but NOT periodic in u (a ramp of 0.3 across the seam:
    column 0 and column W-1 differ)."""
    R = ns + nd
    adch, asch = alb
    ni_need = (3 * R + 6 + max(adch, asch) + 3 + 3) // 4 * 4
    c_pad = ni_need + extra
    c_out = cop or (3 * R + 3) // 4 * 4
    net_in = np.zeros((N, H, W, c_pad), np.float32)
    dirs = _unit(rng, N, H, W, R).astype(np.float32)
    flat = dirs.reshape(-1, R, 3)
    for i, s in enumerate(SEAM_DIRS):
        flat[i, :] = s
    net_in[..., :3 * R] = dirs.reshape(N, H, W, 3 * R)
    net_in[..., 3 * R:3 * R + 6] = rng.standard_normal((N, H, W, 6))
    net_in[..., 3 * R + 6:] = rng.random((N, H, W, c_pad - 3 * R - 6))
    raw = (rng.standard_normal((N, H, W, c_out)) * 1.2).astype(np.float32)
    raw.reshape(-1, c_out)[:len(SEAM_DIRS)] = 0.0
    bias = (rng.standard_normal(c_out) * 0.1).astype(np.float32)
    alpha = (rng.random((N, H, W)) > 0.3).astype(np.float32)
    alpha.reshape(-1)[:len(SEAM_DIRS)] = 1.0
    lh, lw = lp_hw
    vv, uu = np.meshgrid((np.arange(lh) + 0.5) / lh, (np.arange(lw) + 0.5) / lw, indexing='ij')
    lp = np.stack([0.5 + 0.2 * np.sin(2 * np.pi * (uu + k / 3)) * np.cos(np.pi * vv) + 0.3 * uu - 0.1 * k * vv
                   for k in range(3)], -1).astype(np.float32)
    lp += (rng.random(lp.shape) * 0.05).astype(np.float32)
    return net_in, raw, bias, alpha, lp


# (C, R, n_diff, lp batch N?, no_albedo, seperate_albedo, lp_scale_factor) -> tiled kernel iff C <= 4 and R <= 64
RENDERER_CASES = [
    (3, 13, 5, False, False, True, 1.0),      # tiled
    (3, 64, 32, True, True, False, 1.0),      # tiled, R at its limit, lp per view, no albedo
    (3, 65, 20, True, False, False, 0.7),     # generic kernel with C = 3 (R > 64)
    (5, 13, 0, False, True, False, 1.0),      # generic (C > 4), no diffuse rays
    (8, 7, 3, True, False, True, 2.5),        # generic, lp per view, separate albedo, scaled probe
]


def _renderer_inputs(rng, C, R, N, H, W, lp_n, lp_hw=(11, 23)):
    uv = rng.random((N, H, W, 2, R)).astype(np.float32)
    flat = uv.reshape(-1, 2, R)
    special = np.array([-1.0, 0.0, 1.0, 3.0 / lp_hw[1], np.nextafter(np.float32(1), np.float32(2)), -np.float32(1e-7)], np.float32)
    for i, s in enumerate(special):
        flat[i, :, :] = s
    lt = (rng.random((N, R, C, H, W)) * 2).astype(np.float32)
    lp = rng.random((lp_n,) + lp_hw + (C,)).astype(np.float32)
    a_s = rng.random((N, C, H, W)).astype(np.float32)
    a_d = rng.random((N, C, H, W)).astype(np.float32)
    return uv, lt, lp, a_s, a_d
