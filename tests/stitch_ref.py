"""float64 numpy restatement of the stitched light probe: stitch_lp.py's scatter with the semantics its fancy-index `+=` has
(per view a texel takes the LAST pixel in row-major order that maps to it and its count rises by one; views add up in float64
in view order), the background dilation, train_rnr.py:288-295's preparation and lines 296-311 composed from the oracle's
operators.  tests/golden/stitch_lp/make_stitch_golden.py pins `stitch` against the reference's own script bit for bit."""
import numpy as np

TIE_MARGIN = 1e-6        # a case is used only when no u * lp_w or v * lp_h comes closer to a rounding tie than this


def view_rays(proj_inv, R_inv, H, W):
    """stitch_lp.py:26-33 (camera2ray) given K^-1 and R^-1 [3,3] float64 -> unit directions [3,H,W]."""
    y, x = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing='ij')
    pos = np.stack((x, y, np.ones_like(x)), axis=0).reshape(3, -1)
    pos = np.dot(np.asarray(R_inv, np.float64), np.dot(np.asarray(proj_inv, np.float64), pos))
    return (pos / np.sqrt(np.sum(pos * pos, axis=0))[None]).reshape(3, H, W)


def texels(d, lp_h, lp_w):
    """stitch_lp.py:21-23, 145-147 for directions [3,n] -> (row [n], col [n], minimum distance from a rounding tie)."""
    fu = np.minimum((np.arctan2(d[2], d[0]) * 0.5 / np.pi + 0.5) * lp_w, lp_w - 1.0)
    fv = np.minimum((np.arccos(d[1]) * 1.0 / np.pi) * lp_h, lp_h - 1.0)
    tie = min((np.abs(f - np.floor(f) - 0.5).min() if f.size else 0.5) for f in (fu, fv))
    return np.round(fv).astype(np.int64), np.round(fu).astype(np.int64), float(tie)


def stitch(images, masks, proj_inv, R_inv, lp_h, lp_w):
    """images [N,H,W,3] float32, masks [N,H,W] bool (True = background), proj_inv / R_inv [N,3,3] float64 ->
    dict(lp [lp_h,lp_w,3] float32, mask bool, count int32, sum float64, winners [N, lp_h lp_w] int64 (the winning pixel's
    row-major index per view, -1 = none), tie (the minimum tie distance of the case))."""
    images, masks = np.asarray(images, np.float32), np.asarray(masks) != 0
    N, H, W = masks.shape
    T = lp_h * lp_w
    total = np.zeros((T, 3), np.float64)
    count = np.zeros(T, np.int32)
    winners = np.full((N, T), -1, np.int64)
    tie = 0.5
    for n in range(N):
        d = view_rays(proj_inv[n], R_inv[n], H, W)
        m = masks[n].reshape(-1)
        row, col, t = texels(d.reshape(3, -1)[:, m], lp_h, lp_w)
        tie = min(tie, t)
        np.maximum.at(winners[n], row * lp_w + col, np.flatnonzero(m))
        hit = winners[n] >= 0
        total[hit] += images[n].reshape(-1, 3)[winners[n][hit]].astype(np.float64)
        count[hit] += 1
    on = count > 0
    lp = np.zeros((T, 3), np.float64)
    lp[on] = total[on] / count[on][:, None].astype(np.float64)
    return {'lp': lp.astype(np.float32).reshape(lp_h, lp_w, 3), 'mask': on.reshape(lp_h, lp_w), 'count': count.reshape(lp_h, lp_w),
            'sum': total.reshape(lp_h, lp_w, 3), 'winners': winners, 'tie': tie}


def background_mask(alpha, radius):
    """alpha [N,H,W] -> uint8 [N,H,W]: 1 where no pixel with alpha > 0 lies within Chebyshev distance radius inside the image."""
    with np.errstate(invalid='ignore'):
        cov = np.asarray(alpha) > 0                  # NaN: not covered
    N, H, W = cov.shape
    rows = np.zeros_like(cov)
    for k in range(-radius, radius + 1):
        lo, hi = max(0, k), min(W, W + k)
        if lo < hi:
            rows[:, :, lo - k:hi - k] |= cov[:, :, lo:hi]
    out = np.zeros_like(cov)
    for k in range(-radius, radius + 1):
        lo, hi = max(0, k), min(H, H + k)
        if lo < hi:
            out[:, lo - k:hi - k] |= rows[:, lo:hi]
    return (~out).astype(np.uint8)


def prepare(lp, mask, gamma):
    """train_rnr.py:288-295 in float64: lp [h,w,3] float32, mask [h,w] -> dict(pow [h,w,3] float64: the unrounded power of the
    NaN-cleaned values; out [h,w,3] float64: float32(pow) where the mask is set and elsewhere the float64 mean of those
    float32 values (NaN for an empty mask))."""
    x = np.asarray(lp, np.float32).astype(np.float64)
    x[np.isnan(x)] = 0.0
    with np.errstate(invalid='ignore'):
        p = x if gamma == 1.0 else np.power(x, float(gamma))
    on = np.asarray(mask) != 0
    out = p.astype(np.float32).astype(np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        for c in range(3):
            out[~on, c] = out[on, c].sum() / np.float64(on.sum())
    return {'pow': p, 'out': out}


def lighting_init(lp, mask, count, num_view, l_dir, lmax, gamma, recon_h, recon_w):
    """train_rnr.py:288-311: the prepared probe, its area resizes (the oracle's INTER_AREA restatement, as
    tests/test_gpu_lighting.py uses it), the bilinear samples at l_dir [3,ns] and the SH fit, in float64 on the host."""
    import torch
    from oracle import rnr_oracle as orc
    H, W = mask.shape
    on = np.asarray(mask) != 0
    prep = prepare(lp, on, gamma)['out']
    maskf = on.astype(np.float32)[..., None]
    countf = (np.asarray(count).astype(np.float32) / np.float32(num_view))[..., None]
    d = torch.as_tensor(np.asarray(l_dir, np.float64))
    uv = orc.spherical_mapping(d)
    x = (uv[0] * float(W)).clamp(max=W - 1)
    y = (uv[1] * float(H)).clamp(max=H - 1)
    samples = orc.interpolate_bilinear(torch.from_numpy(prep), x, y)
    msamp = orc.interpolate_bilinear(torch.from_numpy(maskf.astype(np.float64)), x, y)[:, 0] == 1
    basis = torch.from_numpy(orc.sh_basis(lmax, d.t().numpy()))
    return {'lp': prep, 'lp_resize': orc.resize_area(prep.astype(np.float32), recon_h, recon_w).astype(np.float64),
            'mask_resize': orc.resize_area(maskf, recon_h, recon_w)[..., 0].astype(np.float64),
            'count_resize': orc.resize_area(countf, recon_h, recon_w)[..., 0].astype(np.float64),
            'l_samples_init': samples.numpy(), 'l_samples_init_mask': msamp.numpy(), 'basis': basis.numpy(),
            'coeff_init': orc.fit_sh_coeff(samples, basis).numpy()}


# ---- synthetic cameras and cases (shared by the golden generator and the tests) ---------------------------------------------
def look_at(eye, target, up):
    """World-to-camera rotation [3,3] of a camera at `eye` looking at `target` (x right, y down, z forward)."""
    eye, target, up = (np.asarray(v, np.float64) for v in (eye, target, up))
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(z, up)
    x /= np.linalg.norm(x)
    return np.stack((x, np.cross(z, x), z), axis=0)


def intrinsic(H, W, focal):
    return np.array([[focal * W, 0.0, W / 2.0], [0.0, focal * W, H / 2.0], [0.0, 0.0, 1.0]])


def random_cameras(rng, N, H, W, focal=(0.4, 0.9)):
    """N cameras on a jittered ring looking at the origin -> (K [N,3,3], R [N,3,3]) float64."""
    Ks, Rs = [], []
    for n in range(N):
        a = 2 * np.pi * (n + rng.uniform(-0.2, 0.2)) / max(N, 1) + rng.uniform(0, 2 * np.pi) * (N == 1)
        eye = np.array([3 * np.cos(a), rng.uniform(-1.5, 1.5), 3 * np.sin(a)])
        up = np.array([rng.uniform(-0.2, 0.2), 1.0, rng.uniform(-0.2, 0.2)])
        Rs.append(look_at(eye, rng.uniform(-0.3, 0.3, 3), up))
        Ks.append(intrinsic(H, W, rng.uniform(*focal)))
    return np.stack(Ks), np.stack(Rs)


def draw_case(seed, N, H, W, lp_h, lp_w, mask_kind='random', max_redraw=0):
    """A random stitch case whose tie distance is at least TIE_MARGIN -> dict(images [N,H,W,3] float32, masks [N,H,W] bool,
    proj_inv, R_inv [N,3,3] float64, ref = stitch(...), redraws).  The margin is a condition on the inputs: a draw below it is
    drawn again, at most max_redraw times."""
    for redraw in range(max_redraw + 1):
        rng = np.random.RandomState(seed * 1000 + redraw)
        K, R = random_cameras(rng, N, H, W)
        proj_inv, R_inv = np.linalg.inv(K), np.linalg.inv(R)
        images = rng.uniform(0.0, 4.0, (N, H, W, 3)).astype(np.float32)
        masks = {'all': np.ones((N, H, W), bool), 'none': np.zeros((N, H, W), bool), 'random': rng.rand(N, H, W) < 0.6}[mask_kind]
        ref = stitch(images, masks, proj_inv, R_inv, lp_h, lp_w)
        if ref['tie'] >= TIE_MARGIN:
            return {'images': images, 'masks': masks, 'proj_inv': proj_inv, 'R_inv': R_inv, 'ref': ref, 'redraws': redraw}
    raise AssertionError('no draw of case %d reached the tie margin in %d tries' % (seed, max_redraw + 1))
