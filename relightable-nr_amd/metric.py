"""Drop-in `metric` (reference: metric.py): psnr, compute_err_metrics, compute_err_metrics_batch with the reference's parameter
names, order and defaults, computed by the HIP kernels behind rnr_amd.ops.image_metrics.

Differences from the reference, all in INTEGRATION.md:
  - the arguments are NOT modified (the reference zeroes img_est and img_gt in place outside the mask, and copies ground truth
    into the estimate's crop);
  - device tensors are used where they are; numpy arrays and CPU tensors are uploaded (one copy each);
  - one host synchronisation per call, at the end, to hand numpy results back;
  - the numbers are float64 (the reference's SSIM is float32);
  - SSIM is the definition pytorch_msssim.ssim(X, Y, data_range=255, size_average=False) documents (include/rnr_hip.h states
    it); that library is not available here, so parity with it is unpinned.
Images are on the 0..255 scale, as the reference's callers pass them (train_rnr.py:627-633).  Without a GPU every function
raises RuntimeError: there is no CPU path.
"""
import numpy as np
import torch

from rnr_amd import metrics, ops


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError('metric: no GPU available, and there is no CPU fallback')
    return torch.device('cuda', torch.cuda.current_device())


def _upload(x, dev):
    """A float32 contiguous device tensor of x (numpy array, CPU or device tensor); never aliases memory this module writes."""
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    return t.detach().to(device=t.device if t.is_cuda else dev, dtype=torch.float32).contiguous()


def _host(out, box):
    """[N,12] float64 and [N,5] int32 device tensors -> numpy, with ONE copy (and so one synchronisation)."""
    both = torch.cat([out, box.double()], dim=1).cpu().numpy()
    return both[:, :12], both[:, 12:].astype(np.int64)


def _check_masks(box, first_view=0):
    for i in range(box.shape[0]):
        if box[i, 4] == 0:
            raise ValueError('metric: the mask of view %d has no pixel equal to 1 (no bounding box)' % (first_view + i))


def psnr(img1, img2, mask = None):
    """metric.py:7-16 for images [H,W,3] on the 0..255 scale: 100 if the mean squared error of img / 255 is below 1e-10, else
    -10 log10 of it; mask None (mean over the image), [H,W] or [H,W,3] with equal channels, 1 where valid (sum over the mask
    divided by its size).  Returns a float."""
    dev = _device()
    a, b = _upload(img1, dev), _upload(img2, dev)
    if a.dim() != 3 or a.shape[2] != 3 or b.shape != a.shape:
        raise ValueError('psnr: images must be [H,W,3], got %s and %s' % (tuple(a.shape), tuple(b.shape)))
    m = None
    if mask is not None:
        m = _upload(mask, a.device)
        if m.dim() == 3:
            if tuple(m.shape) != tuple(a.shape) or not bool((m == m[:, :, :1]).all()):
                raise ValueError('psnr: a [H,W,3] mask must have three equal channels')
            m = m[:, :, 0].contiguous()
        if tuple(m.shape) != tuple(a.shape[:2]):
            raise ValueError('psnr: mask must be [H,W] or [H,W,3], got %s' % (tuple(m.shape),))
        m = m[None]
    out = ops.image_metrics(a[None], b[None], m, compute_ssim=False, channels_last=True)
    return float(out[0, metrics.KEYS.index('psnr' if mask is None else 'psnr_valid')])


def compute_err_metrics(img_est, img_gt, mask, compute_ssim = True):
    """
    :param img_est: numpy.ndarray or torch.Tensor, (H, W, 3)
    :param img_gt: numpy.ndarray or torch.Tensor, (H, W, 3)
    :param mask: numpy.ndarray or torch.Tensor, (H, W)
    :return: dict of float (metric.py:19-84; no 'ssim*' keys unless compute_ssim)
    """
    dev = _device()
    est, gt = _upload(img_est, dev), _upload(img_gt, dev)
    m = _upload(mask, est.device)
    if est.dim() != 3 or est.shape[2] != 3:
        raise ValueError('compute_err_metrics: img_est must be (H, W, 3), got %s' % (tuple(est.shape),))
    out, box = ops.image_metrics(est[None], gt[None], m[None], compute_ssim=compute_ssim, channels_last=True, return_box=True)
    out, box = _host(out, box)
    _check_masks(box)
    n = 12 if compute_ssim else 9
    return {k: float(out[0, i]) for i, k in enumerate(metrics.KEYS[:n])}


def compute_err_metrics_batch(img_est, img_gt, mask, compute_ssim = True):
    """
    :param img_est: torch.Tensor, (N, 3, H, W)
    :param img_gt: torch.Tensor, (N, 3, H, W)
    :param mask: torch.Tensor, (N, 1, H, W)
    :return: dict (metric.py:87-122): per key an [N,1] float64 numpy array and key + '_mean'; with compute_ssim False the three
             SSIM entries stay [] and their means are NaN
    """
    dev = _device()
    est, gt = _upload(img_est, dev), _upload(img_gt, dev)
    m = _upload(mask, est.device)
    if est.dim() != 4 or est.shape[1] != 3:
        raise ValueError('compute_err_metrics_batch: img_est must be (N, 3, H, W), got %s' % (tuple(est.shape),))
    if m.dim() != 4 or m.shape[1] != 1:
        raise ValueError('compute_err_metrics_batch: mask must be (N, 1, H, W), got %s' % (tuple(m.shape),))
    out, box = ops.image_metrics(est, gt, m[:, 0].contiguous(), compute_ssim=compute_ssim, return_box=True)
    out, box = _host(out, box)
    _check_masks(box)
    err_metrics = {}
    for i, key in enumerate(metrics.KEYS):
        err_metrics[key] = np.ascontiguousarray(out[:, i:i + 1]) if (i < 9 or compute_ssim) else []
    for key in metrics.KEYS:          # the means behind the twelve keys, as the reference orders its dict
        err_metrics[key + '_mean'] = err_metrics[key].mean() if len(err_metrics[key]) else np.nan
    return err_metrics
