"""Timing of the texture mapper's backward (rnr_texture_mapper_backward) at a user's size: N views of 512 x 512 of the benchmark's
scene (uv sphere, about half of the pixels foreground) with the benchmark's textures (512 x 512 x 24, four levels, SH on channels
6..14).

  A, per lane   one lane per (pixel, channel), one global atomicAdd per tap and channel (texture_mapper_bwd_kernel);
  B, tile       a workgroup per 16 x 16-pixel tile that sums each level's texel footprint in LDS and flushes it with one global
                atomicAdd per entry (texture_mapper_bwd_tile_kernel).
Both are in the library; RNR_TEXTURE_BWD_FORM=a / b (read by the entry point on every call) forces one, so the two alternate in
one process.  Two upstream gradients: non-zero on every foreground pixel and channel (what a U-Net backward would hand over), and
non-zero on channels 0..5 only (the albedo gradients of the ray renderer's backward: today's case).
  yardstick     (--yardstick, 1 view) the same maths with torch ops on the same device: taps by torch indexing, the scatter by
                index_put_(accumulate=True) per level and tap: what a user would write without the kernel.  A script-local
                restatement.  Its first call is timed alone and the 16-view time is predicted from it, not run.
Device events around windows of back-to-back calls (each 0.2 s or more), a warm-up, the forms alternating within every round,
medians over the rounds.  The byte model: the non-zero contributions the backward sums, 4 B each, against the chip's rate for
well-shaped float atomics, about 1.3 TB/s.

    python scripts/texture_backward_time.py [--views 16 1] [--size 512] [--rounds 7] [--yardstick] [--out FILE (appended to)]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'relightable-nr_amd'), os.path.join(ROOT, 'scripts')):
    if p not in sys.path:
        sys.path.insert(0, p)

from present_time import sized_reps, window_ms  # noqa: E402

DEV = 'cuda:0'
TEX_SIZE, TEX_CH, LEVELS, SH_START = 512, 24, 4, 6


def torch_taps(uv, s):
    """TextureMapper.forward's taps (network.py:71-85, misc.py:5-42) of uv [N,H,W,2] on an s x s level: four flat texel indices
    and four weights, each [N,H,W]."""
    x = uv[..., 0] * (s - 1)
    y = (s - 1) - uv[..., 1] * (s - 1)
    valid = ((x >= 0) & (x <= s - 1) & (y >= 0) & (y <= s - 1)).float()
    x0, y0 = torch.floor(x).long(), torch.floor(y).long()
    x1, y1 = (x0 + 1).clamp(0, s - 1), (y0 + 1).clamp(0, s - 1)
    x0, y0 = x0.clamp(0, s - 1), y0.clamp(0, s - 1)
    x0w, y0w = (x0 - (x0 == x1).long()).float(), (y0 - (y0 == y1).long()).float()
    x1f, y1f = x1.float(), y1.float()
    idx = (y0 * s + x0, y1 * s + x0, y0 * s + x1, y1 * s + x1)
    w = ((x1f - x) * (y1f - y) * valid, (x1f - x) * (y - y0w) * valid, (x - x0w) * (y1f - y) * valid, (x - x0w) * (y - y0w) * valid)
    return idx, w


def torch_backward(uv, sh, g, sizes):
    """The texture gradients of <g, TextureMapper(uv, sh)> with torch ops: index_put_(accumulate=True) per level and tap."""
    C = g.shape[1]
    gf = g.clone()
    gf[:, SH_START:SH_START + 9] *= sh.permute(0, 3, 1, 2)
    gf = gf.permute(0, 2, 3, 1).reshape(-1, C)
    out = []
    for s in sizes:
        idx, w = torch_taps(uv, s)
        gl = torch.zeros(s * s, C, device=uv.device)
        for i, wi in zip(idx, w):
            gl.index_put_((i.reshape(-1),), gf * wi.reshape(-1, 1), accumulate=True)
        out.append(gl.reshape(s, s, C))
    return out


def contributions(uv, sh, g, sizes):
    """Non-zero contributions (g f) w over every level, tap and channel."""
    gf = g.clone()
    gf[:, SH_START:SH_START + 9] *= sh.permute(0, 3, 1, 2)
    nz_ch = (gf != 0).sum(1)                                     # [N,H,W] channels with something to add
    total = 0
    for s in sizes:
        _, w = torch_taps(uv, s)
        total += int(sum(((wi != 0).long() * nz_ch).sum() for wi in w))
    return total


def bench_gbuffer(N, S):
    """uv_map [N,S,S,2], alpha [N,S,S] and the SH basis map [N,S,S,9] of N spiral views of the benchmark's uv sphere."""
    import camera
    from rnr_amd import ops, scene
    mesh = scene.uv_sphere(128, 256)
    dm = ops.DeviceMesh(mesh['v'], mesh['vt'], mesh['vn'], mesh['f_v_idx'], mesh['f_vt_idx'], mesh['f_vn_idx'], DEV)
    ids = [int(i) for i in np.linspace(5, 700, N)]
    v = {k: torch.from_numpy(x).to(DEV) for k, x in scene.spiral_views(S, ids).items()}
    v_uvz = ops.project_vertices(dm.v, v['proj'], v['pose'][:, :3, :3].contiguous(), v['pose'][:, :3, 3].contiguous(), S)
    gb = ops.rasterize_gbuffer(dm, v_uvz, v['pose'], S, maps=['uv_map', 'alpha'])
    vd, _ = camera.get_view_dir_map((S, S), v['proj_inv'], v['R_inv'])
    sh = ops.sh_basis(vd.reshape(-1, 3).contiguous(), 2).reshape(N, S, S, 9)
    return gb['uv_map'].contiguous(), gb['alpha'].contiguous(), sh.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--views', type=int, nargs='+', default=[16, 1])
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--yardstick', action='store_true', help='time the torch formulation instead (first entry of --views, meant for 1)')
    ap.add_argument('--out', default=None, help='also append the result lines to this file')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('texture_backward_time.py needs the GPU: a CPU run measures nothing')
    from rnr_amd import ops
    S = args.size
    sizes = [int(np.round(TEX_SIZE / (2.0 ** l))) for l in range(LEVELS)]
    lines, results = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def hip(form, uv, sh, g):
        os.environ['RNR_TEXTURE_BWD_FORM'] = form
        return ops.texture_mapper_backward(uv, sh, g, sizes, SH_START)

    for N in (args.views[:1] if args.yardstick else args.views):
        uv, alpha, sh = bench_gbuffer(N, S)
        fg = (alpha > 0)[:, None]
        g_all = torch.from_numpy(np.random.default_rng(N).standard_normal((N, TEX_CH, S, S)).astype(np.float32)).to(DEV) * fg
        g_alb = g_all.clone()
        g_alb[:, 6:] = 0.0
        say('texture_backward_time: %d views of %d x %d, %.1f %% foreground, textures %s x %d channels, SH on channels %d..%d'
            % (N, S, S, 100 * float(fg.float().mean()), sizes, TEX_CH, SH_START, SH_START + 8))
        for name, g in (('all channels', g_all), ('channels 0..5', g_alb)):
            adds = contributions(uv, sh, g, sizes)
            floor_ms = adds * 4 / 1.3e12 * 1e3
            if args.yardstick:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch_backward(uv, sh, g, sizes[-1:])           # torch's own first-call set-up, on the smallest level
                torch.cuda.synchronize()
                e0.record()
                ref = torch_backward(uv, sh, g, sizes)
                e1.record()
                e1.synchronize()
                first = e0.elapsed_time(e1)
                agree = {}
                for form in ('a', 'b'):
                    got = hip(form, uv, sh, g)
                    agree[form] = max(float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30) for a, b in zip(got, ref))
                del ref
                reps = max(1, int(np.ceil(200.0 / first)))
                t = [window_ms(lambda: torch_backward(uv, sh, g, sizes), reps)[0] for _ in range(3 if first > 1e3 else args.rounds)]
                ms = statistics.median(t)
                say('  %-14s torch index_put_ backward: first call %.1f ms, then %.3f ms (%.3f .. %.3f, %d calls per window, %d windows); '
                    '16 views predicted %.0f ms, not run; max |HIP - torch| / max |grad|: A %.1e, B %.1e'
                    % (name, first, ms, min(t), max(t), reps, len(t), 16.0 / N * ms, agree['a'], agree['b']))
                results.append({'views': N, 'gradient': name, 'adds': adds, 'torch_ms': ms, 'torch_first_ms': first, 'agreement': agree})
                continue
            fns = {'A, per lane': lambda g=g: hip('a', uv, sh, g), 'B, tile': lambda g=g: hip('b', uv, sh, g)}
            for f in fns.values():
                for _ in range(3):
                    f()
            reps = {k: sized_reps(f, 0.2) for k, f in fns.items()}
            t = {k: [] for k in fns}
            for _ in range(args.rounds):
                for k, f in fns.items():
                    t[k].append(window_ms(f, reps[k])[0])
            for k in fns:
                assert reps[k] * min(t[k]) / 1e3 >= 0.9 * 0.2, (k, reps[k], t[k])
            r = {k: {'ms': statistics.median(v), 'min': min(v), 'max': max(v), 'reps': reps[k]} for k, v in t.items()}
            say('  %-14s %d float adds = %.3f GB (floor %.3f ms at 1.3 TB/s)' % (name, adds, adds * 4 / 1e9, floor_ms))
            for k in fns:
                say('    %-12s %9.4f ms  (%.4f .. %.4f, %d calls per window)  %.0f GB/s of contributions'
                    % (k, r[k]['ms'], r[k]['min'], r[k]['max'], r[k]['reps'], adds * 4 / r[k]['ms'] / 1e6))
            say('    A / B = %.2f' % (r['A, per lane']['ms'] / r['B, tile']['ms']))
            results.append({'views': N, 'gradient': name, 'adds': adds, 'floor_ms': floor_ms, 'times': r})
        del uv, alpha, sh, g_all, g_alb
        torch.cuda.empty_cache()
    os.environ.pop('RNR_TEXTURE_BWD_FORM', None)
    say(json.dumps({'texture_backward_time': {'size': S, 'device': torch.cuda.get_device_name(0), 'yardstick': args.yardstick, 'cases': results}}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
