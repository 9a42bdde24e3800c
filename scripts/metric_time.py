"""A/B timing of the image metrics (rnr_image_metrics) at a user's size: N views of S x S of the benchmark's scene, the
rendered frames against perturbed copies of themselves, mask = the coverage alpha.

  A  ops.image_metrics: three launches (sums and box, SSIM, finalise), float64 arithmetic, no temporaries, no host round trip;
     also timed with compute_ssim=False, so the SSIM launch's share is the difference;
  B  the same twelve numbers per view from torch ops on the same device, in float32 (only its time matters): masking by
     torch.where, grouped conv2d with the 11 x 11 Gaussian for the five moment maps, masked reductions, and the box from
     nonzero per view (a host round trip, as the reference's numpy does), the box SSIM as a mean over a part of the map.
Device events around windows of back-to-back calls (each window 0.2 s or more), a warm-up, A and B alternating in one process,
medians over the rounds (scripts/present_time.py's method and helpers).  The device's calibration (ops.calibrate_mfma_f32) is
printed beside the times: boxes of one pool differ by several per cent.

    python scripts/metric_time.py [--views 16] [--size 512] [--rounds 3] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'relightable-nr_amd'), os.path.join(ROOT, 'scripts')):
    if p not in sys.path:
        sys.path.insert(0, p)

from present_time import ab  # noqa: E402

DEV = 'cuda:0'


def torch_metrics(est, gt, mask, win):
    """B: est, gt [N,3,H,W] on the 0..255 scale, mask [N,H,W], win [3,1,11,11] -> [N,12] float32."""
    N, _, H, W = est.shape
    valid = (mask == 1)[:, None]
    x, y = torch.where(valid, est, 0.0), torch.where(valid, gt, 0.0)
    d = (x - y).abs()
    s1, s2 = d.sum((1, 2, 3)), (d * d).sum((1, 2, 3))
    count = valid.sum((1, 2, 3)).float()
    mom = torch.nn.functional.conv2d(torch.cat([x, y, x * x, y * y, x * y], 1), win.repeat(5, 1, 1, 1), groups=15)
    mu1, mu2, exx, eyy, exy = mom.split(3, 1)
    c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    smap = (2 * mu1 * mu2 + c1) / (mu1 * mu1 + mu2 * mu2 + c1) * (2 * (exy - mu1 * mu2) + c2) / (exx - mu1 * mu1 + eyy - mu2 * mu2 + c2)
    out = torch.empty(N, 12, device=est.device)
    psnr = lambda m: torch.where(m / 65025 < 1e-10, torch.full_like(m, 100.0), -10 * torch.log10(m / 65025))
    for i in range(N):
        ys, xs = valid[i, 0].nonzero(as_tuple=True)
        y0, y1, x0, x1 = int(ys.min()), int(ys.max()) + 1, int(xs.min()), int(xs.max()) + 1          # the host round trip
        n = torch.stack([torch.tensor(3.0 * H * W, device=est.device), torch.tensor(3.0 * (y1 - y0) * (x1 - x0), device=est.device), 3 * count[i]])
        out[i, 0:3] = s1[i] / n
        out[i, 3:6] = s2[i] / n
        out[i, 6:9] = psnr(s2[i] / n)
        out[i, 9] = smap[i].mean()
        out[i, 10] = out[i, 11] = smap[i, :, y0:y1 - 10, x0:x1 - 10].mean()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--views', type=int, default=16)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default=None, help='also write the result lines to this file')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('metric_time.py needs the GPU: a CPU run measures nothing')
    from rnr_amd import ops, scene, testing
    from rnr_amd.pipeline import RNRPipeline
    N, S = args.views, args.size
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ids = [int(i) for i in np.linspace(5, 700, N)]
    v = {k: torch.from_numpy(x).to(DEV) for k, x in scene.spiral_views(S, ids).items()}
    pipe = RNRPipeline(scene.uv_sphere(128, 256), S, testing.synthetic_textures(512, 24, 4, 0), testing.unet_state_dict(108, 78, 64, 5, 0),
                       testing.ray_pivots(6, 2, 5), testing.ray_pivots(6, 2, 10), None, nf0=64, max_views=N, device=DEV,
                       sh_coeff=torch.from_numpy(scene.synthetic_sh_coeff(2, 10, 1)), sh_lmax=10)
    frames = pipe.render(v['proj'], v['pose'], v['proj_inv'], v['R_inv'], keep_intermediates=True).clone()
    alpha = pipe.last['gb']['alpha'].clone()
    del pipe
    gen = torch.Generator(device=DEV).manual_seed(0)
    est = (frames.clamp(0, 1) * 255).contiguous()
    gt = (est + 6 * torch.randn(est.shape, device=DEV, generator=gen)).clamp(0, 255).contiguous()
    k = torch.arange(11, dtype=torch.float64) - 5
    g = torch.exp(-k * k / 4.5)
    g = g / g.sum()
    win = (g[:, None] * g[None, :]).float().to(DEV).expand(3, 1, 11, 11).contiguous()
    cal = ops.calibrate_mfma_f32(DEV)
    say('metric_time: %d views of %d x %d on %s; coverage %.1f %% of the pixels; calibration %.1f TFLOP/s (v_mfma_f32_32x32x2_f32, %d waves per SIMD)'
        % (N, S, S, torch.cuda.get_device_name(0), 100 * float((alpha == 1).float().mean()), cal['tflops'], cal['waves_per_simd']))
    out = torch.empty(N, 12, dtype=torch.float64, device=DEV)
    fa = lambda: ops.image_metrics(est, gt, alpha, out=out)
    fa0 = lambda: ops.image_metrics(est, gt, alpha, out=out, compute_ssim=False)
    fb = lambda: torch_metrics(est, gt, alpha, win)
    a, b = fa().clone(), fb().double()
    dev = (a - b).abs().amax(0)
    say('A (float64) vs B (float32), largest difference per column: ' + ' '.join('%s %.2g' % (n, float(x)) for n, x in zip(ops._lib.METRIC_KEYS, dev)))
    say('view 0: ' + ' '.join('%s %.6g' % (n, float(x)) for n, x in zip(ops._lib.METRIC_KEYS, a[0])))
    r = ab(fa, fb, args.rounds)
    say('A rnr_image_metrics      %8.4f ms (%.4f .. %.4f), host %.4f ms per call' % (r['a_ms'], r['a_spread'][0], r['a_spread'][1], r['a_host_ms']))
    say('B torch ops, float32     %8.4f ms (%.4f .. %.4f), host %.4f ms per call' % (r['b_ms'], r['b_spread'][0], r['b_spread'][1], r['b_host_ms']))
    say('B / A = %.1f; windows %.2f s / %.2f s, %d / %d calls each' % (r['b_ms'] / r['a_ms'], r['shortest_window_s'][0], r['shortest_window_s'][1],
                                                                       r['reps'][0], r['reps'][1]))
    r0 = ab(fa, fa0, args.rounds)
    say('A per launch: sums + finalise (compute_ssim=False) %.4f ms, with the SSIM launch %.4f ms: SSIM %.4f ms'
        % (r0['b_ms'], r0['a_ms'], r0['a_ms'] - r0['b_ms']))
    say(json.dumps({'metric_time': {'views': N, 'size': S, 'device': torch.cuda.get_device_name(0), 'calibration': cal, 'ab': r, 'split': r0}}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
