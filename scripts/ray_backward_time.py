"""Timing of the ray renderer's backward (rnr_ray_renderer_backward) at a user's size: N views of 512 x 512 of the benchmark's
scene (uv sphere, 13 + 13 rays, about half of the pixels foreground) under its 100 x 200 SH light probe.

  forward     ops.ray_renderer on the LightTransport's tensors (no rays_color), what LightTransport.render launches;
  backward    ops.ray_renderer_backward for an image loss (g_out alone, grad_lp alone): the scatter-add of
              views x pixels x 26 rays x 4 taps x 3 channels contributions into the 100 x 200 x 3 probe with global float atomics,
              variant across a wave before the add (the shipped form); with --variant-lib a second build of the library (with
              scripts/experiments/ray_backward_atomic_per_tap.diff applied: one add per lane, tap and channel) is loaded next
              to the shipped one and timed in the same rounds;
  fit step    one step of lighting.fit_sh_lighting (SH reconstruct, forward, loss, backward, SH backward, Adam);
  yardstick   the same forward and backward written with torch ops on the same device (taps by torch indexing, the scatter by
              index_put_(accumulate=True)): what a user would write without the kernel.  A script-local restatement.
Device events around windows of back-to-back calls (each 0.2 s or more), a warm-up, the HIP variants alternating in one process,
medians over the rounds; the yardstick is timed after them, in windows sized from its first call (3 windows when a call takes over a
second).  The byte model: the contributions the backward sums, 4 B each (zero-weight taps and background pixels
contribute none), against the chip's rate for well-shaped float atomics, about 1.3 TB/s.

    python scripts/ray_backward_time.py [--views 1 16] [--size 512] [--rounds 7] [--variant-lib PATH] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'relightable-nr_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

from present_time import sized_reps, window_ms  # noqa: E402

DEV = 'cuda:0'


def torch_taps(uv, hl, wl):
    """misc.interpolate_bilinear's taps (misc.py:5-42) of rays_uv [N,H,W,2,R] on an hl x wl probe: four flat texel indices and
    four weights, each [N,H,W,R]."""
    x = (uv[..., 0, :] * float(wl)).clamp(max=wl - 1)
    y = (uv[..., 1, :] * float(hl)).clamp(max=hl - 1)
    valid = ((x >= 0) & (x <= wl - 1) & (y >= 0) & (y <= hl - 1)).float()
    x0, y0 = torch.floor(x).long(), torch.floor(y).long()
    x1, y1 = (x0 + 1).clamp(0, wl - 1), (y0 + 1).clamp(0, hl - 1)
    x0, y0 = x0.clamp(0, wl - 1), y0.clamp(0, hl - 1)
    x0w, y0w = (x0 - (x0 == x1).long()).float(), (y0 - (y0 == y1).long()).float()
    x1f, y1f = x1.float(), y1.float()
    idx = (y0 * wl + x0, y1 * wl + x0, y0 * wl + x1, y1 * wl + x1)
    w = ((x1f - x) * (y1f - y) * valid, (x1f - x) * (y - y0w) * valid, (x - x0w) * (y1f - y) * valid, (x - x0w) * (y - y0w) * valid)
    return idx, w


def torch_forward(tr, lp):
    """RayRenderer.forward (seperate_albedo=True) with torch ops -> (frames [N,3,S,S], what autograd would keep)."""
    hl, wl = lp.shape[0], lp.shape[1]
    idx, w = torch_taps(tr.rays_uv, hl, wl)
    flat = lp.reshape(-1, 3)
    col = sum(flat[i] * wi[..., None] for i, wi in zip(idx, w)).permute(0, 3, 4, 1, 2)          # [N,R,3,S,S]
    ns = col.shape[1] - tr.num_diff
    prod = tr.rays_lt * col
    out = tr.albedo_specular * (prod[:, :ns].sum(1) / ns) + tr.albedo_diffuse * (prod[:, ns:].sum(1) / tr.num_diff)
    return out, (idx, w)


def torch_backward(tr, lp, saved, g_out):
    """grad_lp of <g_out, frames> with torch ops: index_put_(accumulate=True) per tap."""
    idx, w = saved
    R = tr.rays_lt.shape[1]
    ns = R - tr.num_diff
    gp = torch.cat(((g_out * tr.albedo_specular / ns)[:, None].expand(-1, ns, -1, -1, -1),
                    (g_out * tr.albedo_diffuse / tr.num_diff)[:, None].expand(-1, tr.num_diff, -1, -1, -1)), 1)
    g_col = (gp * tr.rays_lt).permute(0, 3, 4, 1, 2).reshape(-1, 3)                              # [N S S R, 3]
    glp = torch.zeros(lp.shape[0] * lp.shape[1], 3, device=lp.device)
    for i, wi in zip(idx, w):
        glp.index_put_((i.reshape(-1),), g_col * wi.reshape(-1, 1), accumulate=True)
    return glp.reshape(lp.shape)


def rounds_of(fns, rounds, min_window_s=0.2):
    """Median / min / max ms per call of each function, the functions alternating within every round."""
    for f in fns.values():
        for _ in range(3):
            f()
    reps = {k: sized_reps(f, min_window_s) for k, f in fns.items()}
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            t[k].append(window_ms(f, reps[k])[0])
    for k in fns:
        assert reps[k] * min(t[k]) / 1e3 >= 0.9 * min_window_s, (k, reps[k], t[k])
    return {k: {'ms': statistics.median(v), 'min': min(v), 'max': max(v), 'reps': reps[k]} for k, v in t.items()}


def backward_with(lib, tr, lp4, g_out, grad_lp):
    """rnr_ray_renderer_backward of `lib` (the shipped build or the --variant-lib one): g_out alone in, grad_lp alone out."""
    from rnr_amd import _lib, ops
    N, R, C, S, _ = tr.rays_lt.shape
    P, null = ops._ptr, ctypes.c_void_p(0)
    rc = lib.rnr_ray_renderer_backward(P(tr.rays_uv), P(tr.rays_lt), P(lp4), 1, lp4.shape[1], lp4.shape[2], P(tr.albedo_specular),
                                       P(tr.albedo_diffuse), C, R, tr.num_diff, 0, 1, 1.0, P(g_out), null, null, null, null, null,
                                       null, null, null, P(grad_lp), N, S, S, ops._stream())
    if rc != 0:
        raise _lib.RnrError(lib.rnr_last_error().decode('utf-8', 'replace'))
    return grad_lp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--views', type=int, nargs='+', default=[1, 16])
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--variant-lib', default=None, help='a build of librnr_hip.so with one atomic add per tap (scripts/experiments), timed next to the shipped one')
    ap.add_argument('--out', default=None, help='also write the result lines to this file')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('ray_backward_time.py needs the GPU: a CPU run measures nothing')
    from rnr_amd import _lib, ops, scene, testing
    from rnr_amd.lighting import fit_sh_lighting
    from rnr_amd.pipeline import RNRPipeline
    S = args.size
    lines, results = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    shipped = _lib.load()
    variant = None
    if args.variant_lib:
        variant = ctypes.CDLL(os.path.abspath(args.variant_lib))
        variant.rnr_ray_renderer_backward.restype, variant.rnr_ray_renderer_backward.argtypes = _lib.SIGNATURES['rnr_ray_renderer_backward']
        variant.rnr_last_error.restype = ctypes.c_char_p
    ps, pd = testing.ray_pivots(6, 2, 5), testing.ray_pivots(6, 2, 10)
    yard_ms_per_view = None
    for N in args.views:
        print('... %d views: scene, U-Net pass, transport' % N, flush=True)
        pipe = RNRPipeline(scene.uv_sphere(128, 256), S, testing.synthetic_textures(512, 24, 4, 0), testing.unet_state_dict(108, 78, 64, 5, 0),
                           ps, pd, None, nf0=64, max_views=N, device=DEV, sh_coeff=torch.from_numpy(scene.synthetic_sh_coeff(2, 10, 1)),
                           sh_lmax=10)
        ids = [int(i) for i in np.linspace(5, 700, N)]
        v = {k: torch.from_numpy(x).to(DEV) for k, x in scene.spiral_views(S, ids).items()}
        tr = pipe.light_transport(v['proj'], v['pose'], v['proj_inv'], v['R_inv'])
        sh = pipe.sh_lighting
        coeff = pipe.sh_coeff[0].contiguous()
        lp = sh.light_probe(coeff)
        lp4 = lp[None].contiguous()
        del pipe
        torch.cuda.empty_cache()
        g_out = torch.from_numpy(np.random.default_rng(N).standard_normal((N, 3, S, S)).astype(np.float32)).to(DEV) * (tr.alpha > 0)[:, None]
        idx, w = torch_taps(tr.rays_uv, lp.shape[0], lp.shape[1])
        adds = 3 * int(sum(((wi != 0) & (tr.alpha > 0)[..., None]).sum() for wi in w))
        del idx, w
        fg = float((tr.alpha > 0).float().mean())
        glp_a, glp_b = torch.empty_like(lp4), torch.empty_like(lp4)
        say('ray_backward_time: %d views of %d x %d, %.1f %% foreground, 13 + 13 rays, probe %d x %d; %d float adds per backward = %.3f GB '
            '(%.2f ms at 1.3 TB/s)' % (N, S, S, 100 * fg, lp.shape[0], lp.shape[1], adds, adds * 4 / 1e9, adds * 4 / 1.3e12 * 1e3))
        fns = {'forward': lambda: ops.ray_renderer(tr.rays_uv, tr.rays_lt, lp4, tr.albedo_specular, tr.albedo_diffuse, tr.num_diff, False, True,
                                                   1.0, want_rays_color=False),
               'backward': lambda: backward_with(shipped, tr, lp4, g_out, glp_a)}
        if variant is not None:
            fns['backward, add per tap'] = lambda: backward_with(variant, tr, lp4, g_out, glp_b)
        r = rounds_of(fns, args.rounds)
        for k in fns:
            extra = '  %.0f GB/s of adds' % (adds * 4 / r[k]['ms'] / 1e6) if k.startswith('backward') else ''
            say('  %-22s %9.4f ms  (%.4f .. %.4f, %d calls per window)%s' % (k, r[k]['ms'], r[k]['min'], r[k]['max'], r[k]['reps'], extra))
        targets = tr.render(lp).clone()
        steps = 20
        fit = lambda: fit_sh_lighting(tr, targets, sh, steps=steps)
        fit()
        reps = sized_reps(fit, 0.2)
        r['fit step'] = {'ms': statistics.median(window_ms(fit, reps)[0] for _ in range(args.rounds)) / (steps + 1), 'reps': reps}
        say('  %-22s %9.4f ms  (fit_sh_lighting, lmax %d, Adam: %d steps per call, %d calls per window)'
            % ('fit step', r['fit step']['ms'], sh.lmax, steps, reps))
        del targets
        # the yardstick last, one call at a time: index_put_(accumulate=True) sorts the indices and then adds the duplicates of
        # one index one after the other, and every ray of a background pixel (weight 0) lands on texel 0 — a call can take
        # seconds.  It is skipped (and reported as not measured) where the previous, smaller scene predicts more than a minute.
        agree = {}
        predicted = yard_ms_per_view * N if yard_ms_per_view is not None else 0.0
        if predicted > 60e3:
            say('  torch forward / backward: NOT MEASURED at this size (%.0f s per call predicted from the smaller scene)' % (predicted / 1e3))
        else:
            say('  torch yardstick: first calls ...')
            fwd_ms = window_ms(lambda: torch_forward(tr, lp), 1)[0]
            out_t, saved = torch_forward(tr, lp)
            fwd_diff = float((fns['forward']()[0] - out_t).abs().max())
            del out_t
            say('  torch forward, first call %.1f ms; max |frame - torch| = %.1e' % (fwd_ms, fwd_diff))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ref = torch_backward(tr, lp, saved, g_out)
            e1.record()
            e1.synchronize()
            first_bwd = e0.elapsed_time(e1)
            scale = float(ref.abs().max())
            agree['backward'] = float((fns['backward']()[0] - ref).abs().max()) / scale
            if variant is not None:
                agree['backward, add per tap'] = float((fns['backward, add per tap']()[0] - ref).abs().max()) / scale
            del ref
            say('  torch backward, first call %.1f ms; max |grad_lp - torch| / max |grad_lp|: %s'
                % (first_bwd, ', '.join('%s %.1e' % kv for kv in agree.items())))
            yard_ms_per_view = first_bwd / N
            for name, f, first in (('torch forward', lambda: torch_forward(tr, lp), fwd_ms), ('torch backward', lambda: torch_backward(tr, lp, saved, g_out), first_bwd)):
                reps = max(1, int(np.ceil(200.0 / first)))
                n_rounds = args.rounds if first < 1e3 else 3
                t = []
                for i in range(n_rounds):
                    t.append(window_ms(f, reps)[0])
                r[name] = {'ms': statistics.median(t), 'min': min(t), 'max': max(t), 'reps': reps}
                say('  %-22s %9.4f ms  (%.4f .. %.4f, %d calls per window, %d windows)' % (name, r[name]['ms'], min(t), max(t), reps, n_rounds))
            say('  torch / HIP: forward %.1fx, backward %.1fx' % (r['torch forward']['ms'] / r['forward']['ms'], r['torch backward']['ms'] / r['backward']['ms']))
            del saved
        results.append({'views': N, 'foreground': fg, 'adds': adds, 'times': r, 'agreement': agree})
        del tr
        torch.cuda.empty_cache()
    say(json.dumps({'ray_backward_time': {'size': S, 'device': torch.cuda.get_device_name(0), 'cases': results}}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
