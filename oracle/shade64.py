"""ORACLE (test infrastructure, not product): float64 evaluation of the shading operators, for tests that compare the HIP
kernels with a high-precision reference at shapes and parameters the reference-generated fixtures do not cover.

Restated from the reference's semantics (the same reference lines rnr_oracle.py cites), in the same two parts the kernels have:
  * the INTEGER tap indices and the validity mask of every bilinear fetch come from the float32 coordinate expressions the
    reference evaluates (u*(S-1), (S-1) - v*(S-1), clamp(u*W, max=W-1), floor, the [0, W-1] test).  The kernels claim the
    same bits for them (shade.hip is built with -ffp-contract=off), so these stay float32 here: rnr_oracle.bilinear_taps.
  * everything after the taps is float64: bilinear weights (from the same float32 coordinates), the blend, the level sum, the
    SH factor, normalisation, cross products, ray reflection, the spherical mapping of ray directions, ray sums and means.

Inputs are torch CPU tensors (float32 as the kernels receive them); outputs are float64 unless stated.
test_oracle_golden.py::test_shade64_* pins this module against rnr_oracle (float32) and the reference-generated fixtures.
"""
import math

import torch

from . import rnr_oracle as orc

D = torch.float64


def normalize(x, dim=-1):
    """torch.nn.functional.normalize in float64: x / max(||x||, 1e-12)."""
    x = x.to(D)
    return x / x.norm(dim=dim, keepdim=True).clamp(min=1e-12)


def bilinear(data, x, y):
    """misc.py:5-42 with float32 coordinates x, y [...]: taps and mask from float32, weights and blend in float64.
    data [H,W,C] -> [...,C] float64."""
    H, W = data.shape[0], data.shape[1]
    x = x.to(torch.float32)
    y = y.to(torch.float32)
    (x0, y0, x1, y1), _ = orc.bilinear_taps(H, W, x, y)
    valid = ((x >= 0) & (x <= W - 1) & (y >= 0) & (y <= H - 1)).to(D)
    xd, yd = x.to(D), y.to(D)
    x0w = (x0 - (x0 == x1).long()).to(D)
    y0w = (y0 - (y0 == y1).long()).to(D)
    x1f, y1f = x1.to(D), y1.to(D)
    w00 = (x1f - xd) * (y1f - yd) * valid
    w10 = (x1f - xd) * (yd - y0w) * valid
    w01 = (xd - x0w) * (y1f - yd) * valid
    w11 = (xd - x0w) * (yd - y0w) * valid
    d = data.to(D)
    return (d[y0, x0] * w00[..., None] + d[y1, x0] * w10[..., None] +
            d[y0, x1] * w01[..., None] + d[y1, x1] * w11[..., None])


def texture_mapper(textures, uv_map, sh_basis_map=None, sh_start_ch=3):
    """network.py:67-91.  textures: list of [1,S,S,C] or [S,S,C]; uv_map [N,H,W,2] float32; sh_basis_map [N,H,W,9] (any
    dtype, applied in float64) or None -> [N,C,H,W] float64."""
    uv = uv_map.to(torch.float32)
    out = None
    for tex in textures:
        t = tex.reshape(tex.shape[-3], tex.shape[-2], tex.shape[-1])
        s = t.shape[0]
        x = uv[..., 0] * (s - 1)                 # float32, one rounding each: the kernel's u * sm1 ...
        y = (s - 1) - uv[..., 1] * (s - 1)       # ... and sm1 - v * sm1 (no contraction)
        lvl = bilinear(t, x, y).permute(0, 3, 1, 2)
        out = lvl if out is None else out + lvl
    if sh_basis_map is not None and sh_start_ch >= 0:
        out = out.clone()
        out[:, sh_start_ch:sh_start_ch + 9] *= sh_basis_map.to(D).permute(0, 3, 1, 2)
    return out


def face_tangents(faces_v, faces_vt):
    """render.py:135-147 in float64 (det clamped at 1e-8, negative dets too).  faces_v [nf,3,3], faces_vt [nf,3,2]."""
    v, vt = faces_v.to(D), faces_vt.to(D)
    e1, e2 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    d1, d2 = vt[:, 1] - vt[:, 0], vt[:, 2] - vt[:, 0]
    f = 1.0 / (d1[:, 0] * d2[:, 1] - d2[:, 0] * d1[:, 1]).clamp(min=1e-8)
    return normalize(f[:, None] * (d2[:, 1:2] * e1 - d1[:, 1:2] * e2))


def tbn_map(normal_map, face_index_map, tangents):
    """render.py:152-166 given per-face tangents [nf,3] -> [N,H,W,3,3], columns (T, B, N); index -1 wraps to the last face."""
    tan = normalize(tangents)[face_index_map.long()]
    n = normalize(normal_map)
    b = normalize(torch.cross(n, tan, dim=-1))
    t = normalize(torch.cross(b, n, dim=-1))
    return torch.stack([t, b, n], dim=-1)


def view_dir_map(img_hw, proj_inv, R_inv):
    """camera.py:5-32 -> (world [N,H,W,3], camera [N,H,W,3]) in float64 (pixel centres col + 0.5, row + 0.5)."""
    H, W = int(img_hw[0]), int(img_hw[1])
    vv, uu = torch.meshgrid(torch.arange(H, dtype=D) + 0.5, torch.arange(W, dtype=D) + 0.5, indexing='ij')
    pix = torch.stack([uu, vv, torch.ones_like(uu)], -1)                          # [H,W,3]
    cam = normalize(-torch.einsum('nij,hwj->nhwi', proj_inv.to(D), pix))
    world = normalize(torch.einsum('nij,nhwj->nhwi', R_inv.to(D), cam))
    return world, cam


def spherical_uv(d, dim=-2):
    """render.py:87-102 in float64: u = atan2(z, x) / 2pi + 1/2, v = acos(y) / pi (torch.atan2 sign-bit semantics)."""
    d = d.to(D)
    x, y, z = d.select(dim, 0), d.select(dim, 1), d.select(dim, 2)
    return torch.stack((torch.atan2(z, x) * 0.5 / math.pi + 0.5, torch.acos(y.clamp(-1.0, 1.0)) / math.pi), dim=dim)


def ray_sampler(reflect, pivots, tbn, view_tangent, alpha):
    """network.py:445-472 in float64.  pivots [3,R]; tbn [...,3,3]; view_tangent [...,3]; alpha [...] ->
    (dirs [...,3,R], uv [...,2,R], dirs_tangent [...,3,R])."""
    p = pivots.to(D)
    a = alpha.to(D)[..., None, None]
    if reflect:
        v = view_tangent.to(D)[..., None]
        lt = normalize((p * v).sum(-2, keepdim=True) * 2.0 * p - v, dim=-2) * a
    else:
        lt = p.expand(tbn.shape[:-2] + p.shape)
    dirs = normalize(torch.matmul(tbn.to(D), lt), dim=-2)
    uv = spherical_uv(dirs, -2) * a - (a == 0).to(D)
    return dirs, uv, lt


def sh_basis2(dirs):
    """Real SH basis, lmax 2 (rnr_oracle.sh_basis) of float64 directions [...,3] -> [...,9] float64."""
    shp = dirs.shape[:-1]
    return torch.from_numpy(orc.sh_basis(2, dirs.reshape(-1, 3).to(D).numpy())).reshape(shp + (9,))


def shade_inputs(fim, alpha, uv_map, normal_map, tangents, proj_inv, R_inv, textures, pivots_spec, pivots_diff, sh_start_ch):
    """test_rnr.py:303-356 (what rnr_shade_inputs writes) in float64 from float32 G-buffer maps and per-face tangents.
    Returns net_in [N,H,W,3R+6+C] (channel-last, as the kernel writes it), rays_uv [N,H,W,2,R], neural_img [N,C,H,W],
    sh_basis_map [N,H,W,9]."""
    N, H, W = fim.shape
    tbn = tbn_map(normal_map, fim, tangents)
    vd, _ = view_dir_map((H, W), proj_inv, R_inv)
    vt = normalize(torch.einsum('nhwji,nhwj->nhwi', tbn, vd))
    sh = sh_basis2(vd)
    neural = texture_mapper(textures, uv_map, sh if sh_start_ch >= 0 else None, sh_start_ch)
    d_s, uv_s, _ = ray_sampler(True, pivots_spec, tbn, vt, alpha)
    d_d, uv_d, _ = ray_sampler(False, pivots_diff, tbn, vt, alpha)
    dirs = torch.cat((d_s, d_d), -1)                                              # [N,H,W,3,R]
    R = dirs.shape[-1]
    net_in = torch.cat((dirs.transpose(-1, -2).reshape(N, H, W, 3 * R), normal_map.to(D), vd,
                        neural.permute(0, 2, 3, 1)), -1)
    return {'net_in': net_in, 'rays_uv': torch.cat((uv_s, uv_d), -1), 'neural_img': neural, 'sh_basis_map': sh,
            'rays_dir': dirs}


def ray_renderer(albedo_specular, rays_uv, rays_lt, lp, albedo_diffuse=None, num_ray_diffuse=0, no_albedo=False,
                 seperate_albedo=False, lp_scale_factor=1.0):
    """network.py:481-527 in float64.  rays_uv [N,H,W,2,R] float32 (its float32 products u*W, v*H, clamped, give the taps);
    rays_lt [N,R,C,H,W]; lp [1 or N,Hl,Wl,C].  Returns (out, out_specular, out_diffuse, ltt_specular, ltt_diffuse,
    rays_color)."""
    uv = rays_uv.to(torch.float32)
    n_spec = uv.shape[-1] - num_ray_diffuse
    lp = lp.to(D) * float(lp_scale_factor)
    Hl, Wl = lp.shape[1], lp.shape[2]
    sx = (uv[..., 0, :] * float(Wl)).clamp(max=Wl - 1)
    sy = (uv[..., 1, :] * float(Hl)).clamp(max=Hl - 1)
    if lp.shape[0] == 1:
        color = bilinear(lp[0], sx, sy)
    else:
        color = torch.stack([bilinear(lp[i], sx[i], sy[i]) for i in range(lp.shape[0])])
    color = color.permute(0, 3, 4, 1, 2)                                          # [N,R,C,H,W]
    lt = rays_lt.to(D)
    a_s = albedo_specular.to(D)
    lt_s = (lt[:, :n_spec] * color[:, :n_spec]).sum(1) / n_spec
    out_s = lt_s if no_albedo else a_s * lt_s
    if num_ray_diffuse > 0:
        lt_d = (lt[:, n_spec:] * color[:, n_spec:]).sum(1) / num_ray_diffuse
        alb_d = albedo_diffuse.to(D) if (seperate_albedo and albedo_diffuse is not None) else a_s
        out_d = lt_d if no_albedo else alb_d * lt_d
    else:
        lt_d = torch.zeros_like(lt_s)
        out_d = torch.zeros_like(out_s)
    return out_s + out_d, out_s, out_d, lt_s, lt_d, color


def ray_render(raw, bias, net_in, alpha, lp, num_spec, num_diff, albedo_diff_ch=0, albedo_spec_ch=3):
    """What rnr_ray_render computes (out-layer bias + tanh, rays_lt = (y*0.5+0.5)*2, RayRenderer with separate albedo;
    network.py:253, 481-527; test_rnr.py:357-359) from channel-last float32 tensors: raw [N,H,W,c_out_pad],
    net_in [N,H,W,c_pad] (ray directions 3R, normal 3, view 3, then the albedo channels), alpha [N,H,W], lp [Hl,Wl,3].
    The ray uv come from the float32 directions through float32 torch.atan2 / acos (spherical_mapping, as the reference
    computes them); taps from there in float32, the rest in float64.  Returns (image [N,3,H,W] float64, rays_lt, rays_uv)."""
    N, H, W, _ = net_in.shape
    R = num_spec + num_diff
    dirs = net_in[..., :3 * R].reshape(N, H, W, R, 3).to(torch.float32)
    uv = orc.spherical_mapping(dirs, dim=-1).transpose(-1, -2)                    # [N,H,W,2,R] float32
    a = alpha.to(torch.float32)[..., None, None]
    uv = uv * a - (a == 0).to(torch.float32)
    y = raw[..., :3 * R].to(D) + bias[:3 * R].to(D)
    lt = (torch.tanh(y) + 1.0).reshape(N, H, W, R, 3).permute(0, 3, 4, 1, 2)      # [N,R,3,H,W]
    base = 3 * R + 6
    alb_d = net_in[..., base + albedo_diff_ch:base + albedo_diff_ch + 3].permute(0, 3, 1, 2)
    alb_s = net_in[..., base + albedo_spec_ch:base + albedo_spec_ch + 3].permute(0, 3, 1, 2)
    img = ray_renderer(alb_s, uv, lt, lp.reshape(1, lp.shape[-3], lp.shape[-2], 3), albedo_diffuse=alb_d,
                       num_ray_diffuse=num_diff, seperate_albedo=True)[0]
    bg = (alpha == 0)[:, None].expand_as(img)
    img = torch.where(bg, torch.zeros_like(img), img)                            # background: exactly 0 (uv = -1 masks every tap)
    return img, lt, uv


def ray_weights(net_in, alpha, lp, num_spec, num_diff, albedo_diff_ch=0, albedo_spec_ch=3):
    """What rnr_ray_weights computes: W[p][3r+c] = albedo_group(r)[p][c] * env colour(ray r)[c] / rays in the group, 0 on
    background pixels; float64 [N,H,W,3R] with the ray uv of ray_render."""
    N, H, W, _ = net_in.shape
    R = num_spec + num_diff
    dirs = net_in[..., :3 * R].reshape(N, H, W, R, 3).to(torch.float32)
    uv = orc.spherical_mapping(dirs, dim=-1).transpose(-1, -2)
    a = alpha.to(torch.float32)[..., None, None]
    uv = uv * a - (a == 0).to(torch.float32)
    Hl, Wl = lp.shape[-3], lp.shape[-2]
    sx = (uv[..., 0, :] * float(Wl)).clamp(max=Wl - 1)
    sy = (uv[..., 1, :] * float(Hl)).clamp(max=Hl - 1)
    col = bilinear(lp.reshape(Hl, Wl, 3), sx, sy)                                # [N,H,W,R,3]
    base = 3 * R + 6
    alb_d = net_in[..., base + albedo_diff_ch:base + albedo_diff_ch + 3].to(D)[..., None, :]
    alb_s = net_in[..., base + albedo_spec_ch:base + albedo_spec_ch + 3].to(D)[..., None, :]
    w = torch.cat((alb_s * col[..., :num_spec, :] / num_spec,
                   alb_d * col[..., num_spec:, :] / max(num_diff, 1)), -2).reshape(N, H, W, 3 * R)
    return torch.where((alpha == 0)[..., None], torch.zeros_like(w), w)


def sh_fit(samples, basis):
    """sph_harm.py:74-88 in float64: samples [ns,nc], basis [ns,nb] -> [nb,nc]."""
    return basis.to(D).t() @ samples.to(D) * (4.0 * math.pi / samples.shape[0])


def sh_reconstruct(basis, coeff):
    """sph_harm.py:91-102 in float64: basis [ns,nb], coeff [nb,nc] -> [ns,nc]."""
    return basis.to(D) @ coeff.to(D)
