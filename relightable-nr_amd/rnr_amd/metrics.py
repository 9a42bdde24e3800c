"""How good a frame is: the per-view error metrics of the reference's metric.compute_err_metrics_batch (metric.py:19-122) on the
device, from ops.image_metrics (rnr_image_metrics).  Nothing here copies to the host.

The SSIM is the definition include/rnr_hip.h states (11-tap Gaussian, sigma 1.5, valid convolution, data range 255), which is
what pytorch_msssim.ssim documents; that library is not available here, so parity with it is unpinned.
"""
from . import _lib, ops

# the twelve names, in the order of ops.image_metrics' columns (the RNR_METRIC_* enum)
KEYS = _lib.METRIC_KEYS


def _mask3(mask):
    """[N,H,W] float32 contiguous from [N,H,W] or [N,1,H,W] of any dtype (bool: True is valid)."""
    if mask is None:
        return None
    if mask.dim() == 4 and mask.shape[1] == 1:
        mask = mask[:, 0]
    return mask.float().contiguous()


def score_frames(frames, targets, mask, compute_ssim=True):
    """frames, targets [N,3,H,W] in [0,1] (device float32), mask [N,H,W] or [N,1,H,W] (valid where == 1) or None
    -> dict of the twelve KEYS, each a device [N] float64 tensor: the numbers train_rnr.py:627-633 reports per view
    (`* 255.0` is the kernel's scale).  With compute_ssim=False the three SSIM entries are NaN."""
    out = ops.image_metrics(frames.float().contiguous(), targets.float().contiguous(), _mask3(mask), scale=255.0,
                            compute_ssim=compute_ssim)
    return {k: out[:, i] for i, k in enumerate(KEYS)}
