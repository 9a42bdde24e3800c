"""The float64 yardstick of the loss tests: the ray chromaticity loss (network.py:391-411) and the cropped, alpha-weighted L1
(train_rnr.py:564-569, 581-585), restated step by step in torch float64 with autograd as the reference gradient, the closed-form
adjoint of include/rnr_hip.h next to it, the named cases and the bounds of tests/test_gpu_loss.py.

The yardstick states the PRODUCT's semantics where they deviate from the reference on purpose: a pixel with alpha w == 0 is
selected out (its rays are replaced by ones before the formula, so a NaN there reaches neither the loss nor the gradient); the
maps chrom and chrom_mean are formed from the rays as they are.
"""
import numpy as np
import torch

D = torch.float64
EPS = 1e-12                       # F.normalize's default
U = 2.0 ** -53
F32 = 2.0 ** -23


def T(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x))


# ------------------------------------------------------------------------------------------------
# chromaticity loss
# ------------------------------------------------------------------------------------------------
def pixel_weight(alpha, img):
    """alpha w [N,1,H,W] in float64, w = min(20 |img|, 1) or 1."""
    a = alpha.to(D)
    if img is None:
        return a
    return a * (img.to(D).norm(dim=1, keepdim=True) * 20).clamp(max=1.0)


def chrom_formula(x, alpha, img):
    """network.py:402-410 line by line on float64 tensors -> (loss, chrom, chrom_mean [N,1,3,H,W], chrom_diff [N,R,H,W])."""
    c = torch.nn.functional.normalize(x, dim=2)
    m = c.mean(dim=1)[:, None]
    mh = torch.nn.functional.normalize(m, dim=2)
    d = (1 - (c * mh).sum(2)) * alpha
    if img is not None:
        d = d * (img.norm(dim=1, keepdim=True) * 20).clamp(max=1.0)
    return d.sum() / alpha.sum() / d.shape[1], c, mh, d


def chrom(rays_lt, alpha, img=None, g=1.0):
    """The yardstick on float32 host tensors -> dict: loss, sum_alpha (floats), grad [N,R,3,H,W] = g dloss/drays_lt by autograd,
    chrom, chrom_mean, chrom_diff (float64 maps), aw [N,1,H,W]."""
    x = rays_lt.to(D)
    a = alpha.to(D)
    i = None if img is None else img.to(D)
    aw = pixel_weight(alpha, img)
    on = (aw != 0)[:, None]                                      # [N,1,1,H,W]
    xs = torch.where(on, x, torch.ones_like(x)).requires_grad_()
    loss, _, _, d = chrom_formula(xs, a, i)
    d = torch.where(on[:, :, 0], d, torch.zeros_like(d))
    loss = d.sum() / a.sum() / d.shape[1]
    if bool(torch.isfinite(loss)):
        grad, = torch.autograd.grad(loss * g, xs)
        grad = torch.where(on, grad, torch.zeros_like(grad))
    else:
        grad = None
    with torch.no_grad():
        _, c, mh, _ = chrom_formula(x, a, i)
    return {'loss': float(loss.detach()), 'sum_alpha': float(a.sum()), 'grad': grad, 'chrom': c, 'chrom_mean': mh, 'chrom_diff': d.detach(),
            'aw': aw}


def chrom_closed_form(rays_lt, alpha, img=None, g=1.0):
    """The adjoint as include/rnr_hip.h states it, in float64 -> (loss by the per-pixel sum alpha w (R - S . mh), grad,
    scale [N,R,1,H,W] = k (1 + |t|) / max(n_r, eps): what the cancelling projection's rounding is measured in)."""
    x = rays_lt.to(D)
    a = alpha.to(D)
    R = x.shape[1]
    aw = pixel_weight(alpha, img)[:, None]                       # [N,1,1,H,W]
    on = aw != 0
    x = torch.where(on, x, torch.ones_like(x))
    n = x.norm(dim=2, keepdim=True)
    nc = n.clamp(min=EPS)
    c = x / nc
    S = c.sum(1, keepdim=True)
    m = S / R
    M = m.norm(dim=2, keepdim=True)
    mh = m / M.clamp(min=EPS)
    pix = torch.where(on, aw * (R - (S * mh).sum(2, keepdim=True)), torch.zeros_like(aw))
    loss = pix.sum() / a.sum() / R
    k = g * aw / (a.sum() * R)
    t = torch.where(M >= EPS, (S - (S * mh).sum(2, keepdim=True) * mh) / M.clamp(min=EPS), S / EPS) / R
    gc = -k * (mh + t)
    gx = torch.where(n >= EPS, (gc - (gc * c).sum(2, keepdim=True) * c) / nc, gc / EPS)
    gx = torch.where(on, gx, torch.zeros_like(gx))
    scale = torch.where(on, k.abs() * (1 + t.norm(dim=2, keepdim=True)) / nc, torch.zeros_like(nc))
    return float(loss), gx, scale


def chrom_loss_tol(ref, R, pixels):
    """|loss - ref| allowed between two float64 evaluations (see tests/test_gpu_loss.py)."""
    cover = float(ref['aw'].sum()) / ref['sum_alpha'] if ref['sum_alpha'] > 0 else 0.0
    return (2 * R + 16) * U * cover + pixels * U * abs(ref['loss'])


def chrom_grad_tol(ref_grad, scale, R):
    """Per element: one float32 rounding of the result plus the float64 noise of the projection (see tests/test_gpu_loss.py)."""
    return F32 * ref_grad.abs() + 32 * (R + 8) * U * scale


ALPHAS = ('full', 'binary', 'fractional')
# 2 x 129 x 255 = 65790 pixels: 257 workgroups of 256, so the finalise loop over their records (256 threads) runs a second pass
CHROM_SHAPES = [(1, 1, 1, 1), (1, 2, 5, 13), (2, 9, 37, 29), (3, 26, 64, 64), (1, 39, 17, 66), (2, 3, 129, 255)]
CHROM_SHAPE_257 = CHROM_SHAPES[-1]
TAIL_START = 256 * 256            # the first pixel of workgroup 256, whose record only the second pass of a finalise loop reads
_ALPHA_SEEDS = ALPHAS + ('tail',)


def make_alpha(rng, kind, N, H, W):
    if kind == 'tail':            # non-zero only at flat pixel indices >= 65536: the loss and sum alpha come from record 256 alone
        assert N * H * W > TAIL_START
        a = np.zeros(N * H * W, np.float32)
        a[TAIL_START:] = (0.25 + 0.75 * rng.random(N * H * W - TAIL_START)).astype(np.float32)
        return a.reshape(N, 1, H, W)
    if kind == 'full':
        return np.ones((N, 1, H, W), np.float32)
    if kind == 'binary':
        a = (rng.random((N, 1, H, W)) > 0.4).astype(np.float32)
        a.reshape(-1)[0] = 1.0                                   # never empty
        return a
    a = (rng.random((N, 1, H, W)) * (rng.random((N, 1, H, W)) > 0.2)).astype(np.float32)
    a.reshape(-1)[0] = 0.75
    return a


def chrom_case(shape, alpha_kind, with_img):
    """Inputs as float32 host tensors: rays in [0.5, 2.5) per component (RenderingNet's (tanh + 1) range, away from 0), the
    photograph partly dark (|img| below and above 1/20, so that both sides of the clamp occur)."""
    N, R, H, W = shape
    rng = np.random.default_rng(1000 * R + 10 * H + _ALPHA_SEEDS.index(alpha_kind) + (5 if with_img else 0))
    rays = (0.5 + 2.0 * rng.random((N, R, 3, H, W))).astype(np.float32)
    alpha = make_alpha(rng, alpha_kind, N, H, W)
    img = (rng.random((N, 3, H, W)) * 0.06).astype(np.float32) if with_img else None
    return T(rays), T(alpha), T(img)


def degenerate_case():
    """N = 2, R = 5, 3 x 4: a zero ray (0,0,0), an all-zero pixel (0,1,1), a ray of 1e-20 (1,2,3), a pixel whose chromaticities
    cancel so that M = 0 (1,0,1), a black photograph pixel so that w = 0 (0,2,2), and a NaN ray under alpha = 0 (1,1,0).
    -> rays, alpha, img and the dict of the named pixels."""
    N, R, H, W = 2, 5, 3, 4
    rng = np.random.default_rng(7)
    x = (rng.random((N, R, 3, H, W)) * 2).astype(np.float32)
    x[0, 1, :, 0, 0] = 0
    x[0, :, :, 1, 1] = 0
    x[1, 2, :, 2, 3] = 1e-20
    x[1, 0, :, 0, 1] = -x[1, 1, :, 0, 1]
    x[1, 2:, :, 0, 1] = 0
    x[1, 3, 1, 1, 0] = np.nan
    a = (rng.random((N, 1, H, W)) > 0.3).astype(np.float32)
    for n, y, xx in ((0, 0, 0), (0, 1, 1), (1, 2, 3), (1, 0, 1), (0, 2, 2)):
        a[n, 0, y, xx] = 1
    a[1, 0, 1, 0] = 0
    img = (rng.random((N, 3, H, W)) * 0.06).astype(np.float32)
    img[0, :, 2, 2] = 0
    where = {'zero_ray': (0, 1, 0, 0), 'zero_pixel': (0, 1, 1), 'tiny_ray': (1, 2, 2, 3), 'cancel': (1, 0, 1), 'black': (0, 2, 2),
             'nan_masked': (1, 1, 0)}
    return T(x), T(a), T(img), where


# ------------------------------------------------------------------------------------------------
# cropped L1
# ------------------------------------------------------------------------------------------------
def l1(est, gt, alpha, border, g=1.0):
    """mean over the crop of |fl32(est alpha) - fl32(gt alpha)| in float64 -> (loss, grad [N,C,H,W] by autograd, count).  The
    float32 rounding of the products is carried as a constant offset, so autograd sees d fl32(est alpha) / d est = alpha."""
    e32, g32 = est * alpha, gt * alpha                           # float32 products, as the reference forms them
    e = est.to(D).requires_grad_()
    prod = e * alpha.to(D)
    prod = prod + (e32.to(D) - prod).detach()
    H, W = est.shape[2:]
    b = int(border)
    diff = (prod - g32.to(D))[:, :, b:H - b, b:W - b]
    loss = diff.abs().mean()
    grad, = torch.autograd.grad(loss * g, e)
    return float(loss.detach()), grad, diff.numel()


# partials257: 2 x 130 x 253 = 65780 pixels, 257 workgroups, border 0 so that the pixels of the last one lie in the crop;
# partials257_crop: 257 x 256 pixels are exactly 257 workgroups, the last one wholly inside the border
L1_CASES = {'one_pixel': ((1, 3, 11, 11), 5), 'two_views': ((2, 3, 24, 37), 5), 'one_channel': ((1, 1, 64, 64), 5),
            'no_border': ((2, 3, 9, 14), 0), 'partials257': ((2, 3, 130, 253), 0), 'partials257_crop': ((1, 1, 257, 256), 5)}
_L1_SEEDS = ('no_border', 'one_channel', 'one_pixel', 'two_views', 'partials257', 'partials257_crop')   # a case keeps its seed


def l1_case(name, alpha_kind='fractional'):
    """est, gt in [0, 1), one crop element with est == gt (the sign there is 0; its alpha is 1 unless the kind is `tail`, which
    stays zero before pixel 65536) -> float32 host tensors and the border."""
    (N, C, H, W), b = L1_CASES[name]
    rng = np.random.default_rng(_L1_SEEDS.index(name) + 40)
    est = rng.random((N, C, H, W)).astype(np.float32)
    gt = rng.random((N, C, H, W)).astype(np.float32)
    alpha = make_alpha(rng, alpha_kind, N, H, W)
    gt[0, 0, H // 2, W // 2] = est[0, 0, H // 2, W // 2]
    if alpha_kind != 'tail':
        alpha[0, 0, H // 2, W // 2] = 1.0
    return T(est), T(gt), T(alpha), b


def l1_tols(count, grad_ref):
    """loss: summation order only, count 2^-53 relative (+ one rounding of the division); gradient: one float32 rounding."""
    return (count + 4) * U, F32 * grad_ref.abs()
