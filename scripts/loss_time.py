"""A/B timing of the two per-pixel training losses (csrc/loss.hip) at 1 and at N views of S x S with R rays, on the coverage alpha
of the benchmark's scene:

  A  ops.rays_chrom_loss / ops.rays_chrom_loss_backward and ops.masked_l1_loss / ops.masked_l1_loss_backward: one streaming pass
     each way (+ a one-workgroup finalise forward), float64 per pixel, no [N,R,...] temporaries, nothing synced with the host;
  B  the same formulas as torch ops in float32 on the same device (network.py:402-410; train_rnr.py:565-569, 584), forward under
     no_grad and forward + autograd backward, with torch's peak allocation above the inputs.
Device events around windows of back-to-back calls (each window 0.2 s or more), a warm-up, A and B alternating in one process,
medians over the rounds (scripts/present_time.py's helpers).  Byte floors from the layout, per pixel: the chromaticity forward
reads 3 R rays + alpha + 3 of the photograph = 82 floats at R = 26, its backward reads the same and writes 3 R = 160 floats; the
L1 forward reads 2 C + 1 = 7 floats per pixel, its backward writes C more = 10.  The floors are set against the copy rate that
scripts/micro/hbm_bw_probe.py measures on the same device, run first in a process of its own.

    python scripts/loss_time.py [--views 16] [--size 512] [--rays 26] [--rounds 3] [--out FILE]
"""
import argparse
import json
import os
import re
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'relightable-nr_amd'), os.path.join(ROOT, 'scripts')):
    if p not in sys.path:
        sys.path.insert(0, p)

from present_time import ab  # noqa: E402

DEV = 'cuda:0'


def torch_chrom(rays_lt, alpha, img):
    c = torch.nn.functional.normalize(rays_lt, dim=2)
    m = torch.nn.functional.normalize(c.mean(dim=1)[:, None], dim=2)
    d = (1 - (c * m).sum(2)) * alpha
    d = d * (img.norm(dim=1, keepdim=True) * 20).clamp(max=1.0)
    return d.sum() / alpha.sum() / d.shape[1]


def torch_l1(est, gt, alpha, b=5):
    a = alpha[:, :, b:-b, b:-b]
    return torch.nn.functional.l1_loss((est[:, :, b:-b, b:-b] * a).contiguous().view(-1), (gt[:, :, b:-b, b:-b] * a).reshape(-1))


def peak_above(fn):
    """torch's peak allocation during fn() above what was allocated before it, in bytes."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--views', type=int, default=16)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--rays', type=int, default=26)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default=None, help='also write the result lines to this file')
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    probe = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'micro', 'hbm_bw_probe.py')], capture_output=True, text=True,
                           timeout=300)
    m = re.search(r'copy \(read \+ write\) ([0-9.]+) TB/s', probe.stdout)
    if probe.returncode != 0 or not m:
        raise SystemExit('loss_time.py: scripts/micro/hbm_bw_probe.py failed:\n%s\n%s' % (probe.stdout, probe.stderr[-2000:]))
    copy_tbs = float(m.group(1))
    if not torch.cuda.is_available():
        raise SystemExit('loss_time.py needs the GPU: a CPU run measures nothing')
    from rnr_amd import ops, scene, testing
    from rnr_amd.pipeline import RNRPipeline
    N, S, R = args.views, args.size, args.rays
    say('loss_time: %d rays, %d x %d, on %s; hbm_bw_probe: %s' % (R, S, S, torch.cuda.get_device_name(0), probe.stdout.strip().splitlines()[0]))

    ids = [int(i) for i in np.linspace(5, 700, N)]
    v = {k: torch.from_numpy(x).to(DEV) for k, x in scene.spiral_views(S, ids).items()}
    pipe = RNRPipeline(scene.uv_sphere(128, 256), S, testing.synthetic_textures(512, 24, 4, 0), testing.unet_state_dict(108, 78, 64, 5, 0),
                       testing.ray_pivots(6, 2, 5), testing.ray_pivots(6, 2, 10), None, nf0=64, max_views=N, device=DEV,
                       sh_coeff=torch.from_numpy(scene.synthetic_sh_coeff(2, 10, 1)), sh_lmax=10)
    frames = pipe.render(v['proj'], v['pose'], v['proj_inv'], v['R_inv'], keep_intermediates=True).clone()
    alpha_all = pipe.last['gb']['alpha'].clone().reshape(N, 1, S, S).float().contiguous()
    del pipe
    torch.cuda.empty_cache()
    gen = torch.Generator(device=DEV).manual_seed(0)
    result = {'device': torch.cuda.get_device_name(0), 'copy_tb_s': copy_tbs, 'rays': R, 'size': S, 'views': {}}
    one = torch.ones(1, dtype=torch.float32, device=DEV)
    for n in sorted({1, N}):
        alpha = alpha_all[:n].contiguous()
        est = frames[:n].clamp(0, 1).contiguous()
        gt = (est + 0.03 * torch.randn(est.shape, device=DEV, generator=gen)).clamp(0, 1).contiguous()
        rays = (0.05 + 1.9 * torch.rand(n, R, 3, S, S, device=DEV, generator=gen)).contiguous()
        npix = n * S * S
        say('--- %d view%s: rays_lt %.1f MB, coverage %.1f %% of the pixels' % (n, '' if n == 1 else 's', rays.numel() * 4 / 1e6,
                                                                            100 * float((alpha > 0).float().mean())))
        row = {}
        # chromaticity loss
        out = ops.rays_chrom_loss(rays, alpha, gt)
        xr = rays.clone().requires_grad_()

        def torch_chrom_fb():
            xr.grad = None
            torch_chrom(xr, alpha, gt).backward()

        with torch.no_grad():
            t_loss = float(torch_chrom(rays, alpha, gt))
        torch_chrom_fb()
        g_hip = ops.rays_chrom_loss_backward(rays, alpha, gt, out, one)
        say('chromaticity loss: HIP (float64) %.9g, torch ops (float32) %.9g; gradient: largest |difference| %.3g of largest |g| %.3g'
            % (float(out[0]), t_loss, float((g_hip - xr.grad).abs().max()), float(g_hip.abs().max())))
        del g_hip
        peak = peak_above(torch_chrom_fb)
        with torch.no_grad():
            f = ab(lambda: ops.rays_chrom_loss(rays, alpha, gt), lambda: torch_chrom(rays, alpha, gt), args.rounds)
        b = ab(lambda: ops.rays_chrom_loss_backward(rays, alpha, gt, out, one), torch_chrom_fb, args.rounds)
        live = float((alpha > 0).float().mean())
        floor_f = npix * 4 * (4 + live * 3 * R) / (copy_tbs * 1e12) * 1e3
        floor_b = npix * 4 * (4 + live * 3 * R + 3 * R) / (copy_tbs * 1e12) * 1e3
        say('  A forward  %8.4f ms (%.4f .. %.4f)   floor %.4f ms: %d floats per covered pixel, 4 per other, at %.2f TB/s -> %.2f x the floor'
            % (f['a_ms'], f['a_spread'][0], f['a_spread'][1], floor_f, 3 * R + 4, copy_tbs, f['a_ms'] / floor_f))
        say('  A backward %8.4f ms (%.4f .. %.4f)   floor %.4f ms: %d floats per covered pixel, %d per other -> %.2f x the floor'
            % (b['a_ms'], b['a_spread'][0], b['a_spread'][1], floor_b, 6 * R + 4, 3 * R + 4, b['a_ms'] / floor_b))
        say('  B forward  %8.4f ms (%.4f .. %.4f)   forward + backward %8.4f ms (%.4f .. %.4f); peak allocation above the inputs %.1f MB'
            % (f['b_ms'], f['b_spread'][0], f['b_spread'][1], b['b_ms'], b['b_spread'][0], b['b_spread'][1], peak / 1e6))
        say('  forward + backward: A %.4f ms, B %.4f ms, B / A = %.1f' % (f['a_ms'] + b['a_ms'], b['b_ms'], b['b_ms'] / (f['a_ms'] + b['a_ms'])))
        row['chrom'] = {'forward': f, 'backward_vs_torch_forward_backward': b, 'torch_peak_bytes': peak, 'floor_ms': (floor_f, floor_b)}
        del xr, rays
        # cropped L1
        er = est.clone().requires_grad_()

        def torch_l1_fb():
            er.grad = None
            torch_l1(er, gt, alpha).backward()

        torch_l1_fb()
        o1 = ops.masked_l1_loss(est, gt, alpha, 5)
        g1 = ops.masked_l1_loss_backward(est, gt, alpha, 5, one)
        say('cropped L1: HIP (float64) %.9g, torch ops (float32) %.9g; gradient: largest |difference| %.3g of largest |g| %.3g'
            % (float(o1[0]), float(torch_l1(est, gt, alpha)), float((g1 - er.grad).abs().max()), float(g1.abs().max())))
        peak1 = peak_above(torch_l1_fb)
        with torch.no_grad():
            f1 = ab(lambda: ops.masked_l1_loss(est, gt, alpha, 5), lambda: torch_l1(est, gt, alpha), args.rounds)
        b1 = ab(lambda: ops.masked_l1_loss_backward(est, gt, alpha, 5, one), torch_l1_fb, args.rounds)
        fl_f, fl_b = npix * 4 * 7 / (copy_tbs * 1e12) * 1e3, npix * 4 * 10 / (copy_tbs * 1e12) * 1e3
        say('  A forward  %8.4f ms (%.4f .. %.4f)   floor %.4f ms (7 floats per pixel) -> %.1f x the floor; host %.4f ms per call'
            % (f1['a_ms'], f1['a_spread'][0], f1['a_spread'][1], fl_f, f1['a_ms'] / fl_f, f1['a_host_ms']))
        say('  A backward %8.4f ms (%.4f .. %.4f)   floor %.4f ms (10 floats per pixel) -> %.1f x the floor; host %.4f ms per call'
            % (b1['a_ms'], b1['a_spread'][0], b1['a_spread'][1], fl_b, b1['a_ms'] / fl_b, b1['a_host_ms']))
        say('  B forward  %8.4f ms (%.4f .. %.4f)   forward + backward %8.4f ms (%.4f .. %.4f); peak allocation above the inputs %.1f MB'
            % (f1['b_ms'], f1['b_spread'][0], f1['b_spread'][1], b1['b_ms'], b1['b_spread'][0], b1['b_spread'][1], peak1 / 1e6))
        say('  forward + backward: A %.4f ms, B %.4f ms, B / A = %.1f' % (f1['a_ms'] + b1['a_ms'], b1['b_ms'], b1['b_ms'] / (f1['a_ms'] + b1['a_ms'])))
        row['l1'] = {'forward': f1, 'backward_vs_torch_forward_backward': b1, 'torch_peak_bytes': peak1, 'floor_ms': (fl_f, fl_b)}
        result['views'][n] = row
        del er
        torch.cuda.empty_cache()
    say(json.dumps({'loss_time': result}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
