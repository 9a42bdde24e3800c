"""Yardstick for the image-metric tests (test_metric_ref_cpu.py, test_gpu_metric.py): metric.compute_err_metrics (metric.py:19-84)
restated step by step in float64 numpy — zero both images outside mask == 1, the box from nonzero, the crops, the copy of
ground truth over the estimate's crop outside the mask, and THREE separate SSIM evaluations on the arrays the reference would
pass — plus the cases the tests share.  Written from the formulas; test infrastructure, not product; CPU only.

SSIM is the definition pytorch_msssim.ssim(X, Y, data_range=255, size_average=False) documents: per channel a separable 11-tap
Gaussian (sigma 1.5, weights normalised to sum 1, here in float64) as a valid convolution of X, Y, X^2, Y^2, XY;
C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2; map = (2 mu1 mu2 + C1) / (mu1^2 + mu2^2 + C1) * (2 s12 + C2) / (s1^2 + s2^2 + C2);
the mean over the map, then over the channels.  The library is not installed: parity with it is unpinned.  An image side
below 11 has no window: NaN here.

Where the reference fails (an empty mask has no box) the yardstick returns what include/rnr_hip.h defines: box 0 0 0 0 0 and
NaN in every _bb / _valid entry.
"""
import functools

import numpy as np

KEYS = ('mae', 'mae_bb', 'mae_valid', 'mse', 'mse_bb', 'mse_valid', 'psnr', 'psnr_bb', 'psnr_valid', 'ssim', 'ssim_bb', 'ssim_valid')
WIN = 11
C1, C2 = (0.01 * 255.0) ** 2, (0.03 * 255.0) ** 2


def gaussian_weights():
    k = np.arange(WIN, dtype=np.float64) - WIN // 2
    g = np.exp(-(k ** 2) / (2 * 1.5 ** 2))
    return g / g.sum()


def _valid_filter(a, w, rows_first=True):
    """a [H,W,C] float64 -> [H-10,W-10,C]: the 11 taps along one axis, then along the other."""
    def along(x, ax):
        n = x.shape[ax] - WIN + 1
        return sum(w[k] * np.take(x, range(k, k + n), axis=ax) for k in range(WIN))
    return along(along(a, 0), 1) if rows_first else along(along(a, 1), 0)


def ssim_map(x, y, rows_first=True):
    """x, y [H,W,C] float64 (H, W >= 11) -> the map [H-10,W-10,C]."""
    w = gaussian_weights()
    f = lambda a: _valid_filter(a, w, rows_first)
    mu1, mu2 = f(x), f(y)
    s11, s22, s12 = f(x * x) - mu1 * mu1, f(y * y) - mu2 * mu2, f(x * y) - mu1 * mu2
    return (2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1) * ((2 * s12 + C2) / (s11 + s22 + C2))


def ssim(x, y):
    """x, y [H,W,C] float64 -> the mean over the map per channel, then over the channels; NaN when a side is below 11."""
    if x.shape[0] < WIN or x.shape[1] < WIN:
        return np.nan
    return float(ssim_map(x, y).mean(axis=(0, 1)).mean())


def psnr(a, b, mask=None):
    """metric.py:7-16 in float64."""
    if mask is None:
        mse = np.mean((a / 255. - b / 255.) ** 2)
    else:
        mse = np.sum((a / 255. - b / 255.) ** 2 * mask) / mask.sum()
    if mse < 1.0e-10:
        return 100.0
    return 20 * np.log10(1.0 / np.sqrt(mse))


def err_metrics(img_est, img_gt, mask, compute_ssim=True):
    """One view: img_est, img_gt [H,W,3] float64 on the 0..255 scale, mask [H,W] -> (dict of KEYS, box (xmin, xmax+1, ymin,
    ymax+1, count)).  The arguments are copied first; everything after that follows metric.py:29-82 line by line."""
    img_est, img_gt = np.array(img_est, np.float64), np.array(img_gt, np.float64)
    with np.errstate(invalid='ignore'):
        mask = np.asarray(mask) == 1
    img_est[mask == 0] = 0
    img_gt[mask == 0] = 0
    mask3 = mask[:, :, np.newaxis].repeat(3, axis=2).astype(np.float64)
    nan = float('nan')
    out = dict.fromkeys(KEYS, nan)
    img_diff = np.abs(img_est - img_gt)
    out['mae'] = img_diff.mean()
    out['mse'] = (img_diff ** 2).mean()
    out['psnr'] = psnr(img_est, img_gt)
    if compute_ssim:
        out['ssim'] = ssim(img_est, img_gt)
    suby, subx = (mask3[:, :, 0] == 1).nonzero()
    if len(suby) == 0:
        return out, (0, 0, 0, 0, 0)
    x0, x1, y0, y1 = min(subx), max(subx) + 1, min(suby), max(suby) + 1
    img_est_bb, img_gt_bb = img_est[y0:y1, x0:x1, :], img_gt[y0:y1, x0:x1, :]
    img_diff_bb = img_diff[y0:y1, x0:x1, :]
    num_valid_ele = mask3.sum()
    out['mae_bb'] = img_diff_bb.mean()
    out['mae_valid'] = (img_diff * mask3).sum() / num_valid_ele
    out['mse_bb'] = (img_diff_bb ** 2).mean()
    out['mse_valid'] = (img_diff ** 2 * mask3).sum() / num_valid_ele
    out['psnr_bb'] = psnr(img_est_bb, img_gt_bb)
    out['psnr_valid'] = psnr(img_est, img_gt, mask=mask3)
    if compute_ssim:
        out['ssim_bb'] = ssim(img_est_bb, img_gt_bb)
        mask_bb_inverse = mask3[y0:y1, x0:x1, 0] != 1
        img_est_bb_modify = img_est_bb.copy()
        img_est_bb_modify[mask_bb_inverse] = img_gt_bb[mask_bb_inverse]
        out['ssim_valid'] = ssim(img_est_bb_modify, img_gt_bb)
    return out, (int(x0), int(x1), int(y0), int(y1), int(len(suby)))


def scaled(v, scale):
    """The kernel's input transform: float32(v * scale), ONE float32 product, widened to float64."""
    with np.errstate(invalid='ignore', over='ignore'):
        return (np.asarray(v, np.float32) * np.float32(scale)).astype(np.float64)


def batch(est, gt, mask, scale=1.0, compute_ssim=True):
    """est, gt [N,3,H,W] float32, mask [N,H,W] or None -> (out [N,12] float64 in KEYS order, box [N,5] int64)."""
    N, _, H, W = est.shape
    out, box = np.empty((N, 12)), np.empty((N, 5), np.int64)
    for i in range(N):
        m = np.ones((H, W), np.float32) if mask is None else mask[i]
        d, b = err_metrics(scaled(est[i], scale).transpose(1, 2, 0), scaled(gt[i], scale).transpose(1, 2, 0), m, compute_ssim)
        out[i] = [d[k] for k in KEYS]
        box[i] = b
    return out, box


# ------------------------------------------------------------------------------------------------------------------------
# shared cases
# ------------------------------------------------------------------------------------------------------------------------
def noise_images(N, H, W, seed):
    """Uniform noise on 0..255: (est, gt) [N,3,H,W] float32, independent."""
    rng = np.random.default_rng(seed)
    return ((rng.random((N, 3, H, W)) * 255).astype(np.float32), (rng.random((N, 3, H, W)) * 255).astype(np.float32))


def bright_images(N, H, W, seed):
    """Smooth and bright (238..252) with noise of +-0.5, the two images 0.3 apart on average: E[x^2] - mu^2 cancels from 6e4
    down to 0.1, which float32 moments do not survive."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W]
    base = 245 + 5 * np.sin(xx / 17.0 + np.arange(3)[:, None, None]) * np.cos(yy / 23.0) + np.arange(N)[:, None, None, None] * 0.5
    est = base + rng.random((N, 3, H, W)) - 0.5
    gt = base + 0.3 + rng.random((N, 3, H, W)) - 0.5
    return est.astype(np.float32), gt.astype(np.float32)


def rect_mask(H, W, y0, y1, x0, x1):
    m = np.zeros((H, W), np.float32)
    m[y0:y1, x0:x1] = 1
    return m


def blob_mask(H, W, seed):
    """A ragged blob whose box touches the top and the left border: a seeded random walk of discs, with holes."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W]
    m = np.zeros((H, W), bool)
    cy, cx = H * 0.3, W * 0.3
    for _ in range(12):
        m |= (yy - cy) ** 2 + (xx - cx) ** 2 < (0.12 * min(H, W) + 1) ** 2
        cy = np.clip(cy + rng.normal() * H * 0.12, 0, H * 0.7)
        cx = np.clip(cx + rng.normal() * W * 0.12, 0, W * 0.7)
    m[0, 1:4] = True
    m[2:5, 0] = True
    m &= rng.random((H, W)) > 0.1
    m[0, 2] = m[3, 0] = True
    return m.astype(np.float32)


def disc_mask(H, W):
    yy, xx = np.mgrid[:H, :W]
    return (((yy - H / 2) ** 2 + (xx - W / 2) ** 2) < (0.4 * min(H, W)) ** 2).astype(np.float32)


def four_masks(H, W, seed=5):
    """Full, a ragged blob, a single pixel, empty."""
    single = np.zeros((H, W), np.float32)
    single[H // 2, W // 3] = 1
    return np.stack([np.ones((H, W), np.float32), blob_mask(H, W, seed), single, np.zeros((H, W), np.float32)])


@functools.lru_cache(maxsize=None)
def case(name):
    """A named case, built once: dict est, gt [N,3,H,W] float32, mask [N,H,W] float32 or None, ref [N,12], box [N,5] (the
    tests leave all of them unchanged)."""
    if name == 'one_window':                       # 11 x 11, full mask: exactly one window
        est, gt = noise_images(1, 11, 11, 1)
        mask = np.ones((1, 11, 11), np.float32)
    elif name in ('10x13', '13x10'):               # no window: SSIM NaN, the rest finite
        H, W = (10, 13) if name == '10x13' else (13, 10)
        est, gt = noise_images(1, H, W, 2)
        mask = rect_mask(H, W, 1, H - 1, 2, W)[None]
    elif name == 'four_masks':                     # 37 x 29 (neither a multiple of 4), N = 4
        est, gt = noise_images(4, 37, 29, 3)
        mask = four_masks(37, 29)
    elif name == 'four_masks_bright':
        est, gt = bright_images(4, 37, 29, 4)
        mask = four_masks(37, 29)
    elif name == 'boxes':                          # boxes of exactly 11 x 11, 11 (high) x 12 (wide), 10 (high) x 40 (wide)
        est, gt = noise_images(3, 30, 45, 6)
        mask = np.stack([rect_mask(30, 45, 7, 18, 20, 31), rect_mask(30, 45, 19, 30, 0, 12), rect_mask(30, 45, 3, 13, 5, 45)])
    elif name == 'tiles':                          # 75 x 53: two full 32-window tiles + a remainder down, one + a remainder across
        est, gt = noise_images(2, 75, 53, 7)
        mask = np.stack([blob_mask(75, 53, 8), rect_mask(75, 53, 20, 70, 5, 50)])
    elif name == 'tiles_wide':                     # 53 x 85: two full tiles + a remainder across
        est, gt = bright_images(1, 53, 85, 9)
        mask = disc_mask(53, 85)[None]
    elif name == 'disc128':
        est, gt = bright_images(2, 128, 128, 10)
        mask = np.stack([disc_mask(128, 128)] * 2)
    elif name == 'no_mask':
        est, gt = noise_images(2, 21, 26, 11)
        mask = None
    # the smallest sizes at which a second-level loop of csrc/metric.hip runs a second pass (SECOND_PASS below); the data that
    # only the later pass sees decides the result
    elif name == 'wide300':                        # 13 x 300: sums_kernel's x loop runs twice (W > 256)
        est, gt = noise_images(2, 13, 300, 12)
        ragged = rect_mask(13, 300, 1, 13, 200, 290) * (np.random.default_rng(13).random((13, 300)) > 0.1)
        ragged[1, 200] = ragged[12, 289] = 1       # the box is rows 1..12, columns 200..289: it crosses column 256
        mask = np.stack([rect_mask(13, 300, 0, 13, 260, 300), ragged.astype(np.float32)])   # view 0: second x pass only
    elif name == 'bands256':                       # 2048 x 12: 256 bands of 8 rows, exactly one pass of view_box
        est, gt = noise_images(2, 2048, 12, 14)
        mask = np.stack([blob_mask(2048, 12, 15), rect_mask(2048, 12, 2040, 2048, 0, 12)])
    elif name == 'bands9':                         # 2049 x 12: band_rows 9, 228 bands, the last one 6 rows
        est, gt = noise_images(2, 2049, 12, 16)
        mask = np.stack([rect_mask(2049, 12, 2040, 2049, 0, 12), np.ones((2049, 12), np.float32)])   # view 0: a box 9 high
    elif name == 'tiles257':                       # 8203 x 13: 257 tiles per view (the last holds one row of windows), band_rows 33
        est, gt = noise_images(2, 8203, 13, 17)
        mask = np.stack([np.ones((8203, 13), np.float32), rect_mask(8203, 13, 8100, 8203, 0, 13)])
    else:
        raise KeyError(name)
    ref, box = batch(est, gt, mask)
    return {'est': est, 'gt': gt, 'mask': mask, 'ref': ref, 'box': box}


CASES = ['one_window', '10x13', '13x10', 'four_masks', 'four_masks_bright', 'boxes', 'tiles', 'tiles_wide', 'disc128', 'no_mask',
         'wide300', 'bands256', 'bands9', 'tiles257']

# name -> (H, W, Band records per view, Tile records per view) of the second-pass cases: what csrc/metric.hip's make_plan gives
# them (bands of max(8, ceil(H / 256)) rows, tiles of 32 x 32 windows).  test_metric_ref_cpu.py asserts these counts against
# rnr_image_metrics_workspace_bytes, so a case cannot drift off its threshold unnoticed.
SECOND_PASS = {'wide300': (13, 300, 2, 10), 'bands256': (2048, 12, 256, 64), 'bands9': (2049, 12, 228, 64),
               'tiles257': (8203, 13, 249, 257)}
BAND_BYTES, TILE_BYTES = 40, 16

# bounds of the GPU tests against this yardstick (both sides float64)
#   sums: n 2^-53 for n = 3 x 512^2 terms in any summation order = 8.7e-11
#   PSNR: 10 / ln 10 = 4.34 times the relative error of the mean squared error, in dB
#   SSIM: per window 2^-53 x ~100 operations x the cancellation's amplification 65025 / C2 = 1100 -> 1e-11 (two float64
#         evaluations with the filter passes in either order differ by ~1e-12, test_metric_ref_cpu.py); the mean adds n 2^-53
SUM_RTOL, PSNR_ATOL, SSIM_ATOL = 1e-10, 1e-9, 1e-9


def compare(got, box, ref, ref_box, label=''):
    """Assert got [N,12] / box [N,5] against the yardstick within the bounds; NaN must sit where the yardstick has NaN.
    Prints the figures first."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape
    nan_ok = bool((np.isnan(got) == np.isnan(ref)).all())
    with np.errstate(invalid='ignore', divide='ignore'):
        rel = np.abs(got[:, :6] - ref[:, :6]) / np.abs(ref[:, :6])
        rel[ref[:, :6] == got[:, :6]] = 0
        e_sum = np.nanmax(rel, initial=0.0)
        e_psnr = np.nanmax(np.abs(got[:, 6:9] - ref[:, 6:9]), initial=0.0)
        e_ssim = np.nanmax(np.abs(got[:, 9:] - ref[:, 9:]), initial=0.0)
    print('%s: sums rel %.3g (bound %g), psnr %.3g dB (%g), ssim %.3g (%g), NaN pattern equal: %s'
          % (label, e_sum, SUM_RTOL, e_psnr, PSNR_ATOL, e_ssim, SSIM_ATOL, nan_ok))
    assert nan_ok, (got, ref)
    assert e_sum <= SUM_RTOL and e_psnr <= PSNR_ATOL and e_ssim <= SSIM_ATOL, (e_sum, e_psnr, e_ssim)
    if box is not None:
        np.testing.assert_array_equal(np.asarray(box, np.int64), ref_box)
