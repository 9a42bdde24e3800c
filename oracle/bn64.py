"""ORACLE (test infrastructure, not product): float64 BatchNorm statistics of a convolution's written output, for tests that
compare the statistics the convolution kernels of conv.hip publish (per-view sum / sum of squares) and the BatchNorm scale /
shift derived from them (bn_finalize_views, bn_finalize_kernel) with a high-precision reference.

The input is the float32 raw output the kernel actually WROTE (NHWC, channels padded), not a CPU convolution: the statistics
path is tested on its own, free of the convolution's rounding (the output itself is tested against float64 convolutions in
test_gpu_unet.py), and the benchmark's full layer sizes cost a few float64 reductions on the CPU.

Every operation is float64 on exact inputs: v and v^2 of a float32 v are exact in double, so s1 = sum v and s2 = sum v^2 carry
only float64 summation error; the mean and the biased variance are two-pass (no s2/n - mean^2 cancellation).
  scale = gamma / sqrt(var + eps),  shift = beta - mean * scale            (torch's train-mode batch_norm as an affine map)
  running <- (1 - momentum) * running + momentum * stat, with the UNBIASED variance n/(n-1) var   (torch.nn.BatchNorm2d)
test_oracle_golden.py::test_bn64_* pins this module to torch.nn.functional.batch_norm and torch.nn.BatchNorm2d in float64.
"""
import torch

D = torch.float64


def _affine(mean, var, gamma, beta, eps):
    scale = gamma.to(D) / torch.sqrt(var + float(eps))
    return scale, beta.to(D) - mean * scale


def per_view(out_raw, c_out, gamma, beta, eps=1e-5):
    """out_raw [N,H,W,C_pad] (float32, as written) -> dict of [N, c_out] float64 tensors: s1, s2, mean, var (biased, two-pass),
    scale, shift — BatchNorm over each view's (H, W) alone (UNetPlan bn_mode 'batch', rnr_bn_finalize*)."""
    v = out_raw[..., :c_out].to(D)
    n = v.shape[1] * v.shape[2]
    s1 = v.sum(dim=(1, 2))
    s2 = (v * v).sum(dim=(1, 2))
    mean = s1 / n
    var = ((v - mean[:, None, None]) ** 2).sum(dim=(1, 2)) / n
    scale, shift = _affine(mean, var, gamma, beta, eps)
    return {'s1': s1, 's2': s2, 'mean': mean, 'var': var, 'scale': scale, 'shift': shift, 'count': n}


def batch_all(out_raw, c_out, gamma, beta, eps=1e-5, running_mean=None, running_var=None, momentum=0.1):
    """The same over the whole batch (N, H, W) — torch's train-mode BatchNorm2d of one call (bn_mode 'batch_all',
    rnr_bn_finalize_batch): [c_out] tensors, plus the updated running_mean / running_var when they are given."""
    v = out_raw[..., :c_out].to(D).reshape(-1, c_out)
    n = v.shape[0]
    s1 = v.sum(dim=0)
    s2 = (v * v).sum(dim=0)
    mean = s1 / n
    var = ((v - mean) ** 2).sum(dim=0) / n
    scale, shift = _affine(mean, var, gamma, beta, eps)
    r = {'s1': s1, 's2': s2, 'mean': mean, 'var': var, 'scale': scale, 'shift': shift, 'count': n}
    if running_mean is not None:
        r['running_mean'] = (1.0 - momentum) * running_mean.to(D) + momentum * mean
    if running_var is not None:
        unbiased = var * n / (n - 1) if n > 1 else var
        r['running_var'] = (1.0 - momentum) * running_var.to(D) + momentum * unbiased
    return r
