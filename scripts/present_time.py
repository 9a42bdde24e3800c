"""A/B timing of the presenter (rnr_present_u8) at a user's size: N views of S x S, 100 x 200 and 1600 x 3200 probes.

  A  ops.present_u8 in each mode — one launch, no temporaries;
  B  the same bytes from the existing drop-in operators and torch ops on the same device, the reference's own call sequence
     (test_rnr.py:377, 386-393): ops.view_dir_map -> render.spherical_mapping_batch -> clamp -> ops.interpolate_bilinear ->
     where -> * 255 -> round -> clamp -> to(uint8) -> flip.
Device events around windows of back-to-back calls (each window 0.2 s or more), a warm-up, A and B alternating in one
process, medians over the rounds.  The byte model is printed next to the times: the least traffic the result needs, so
bytes/s = model bytes / time (for B too: what it achieves of the useful traffic, not what it moves).
Then the step time of RNRPipeline(max_views=N) on the benchmark's scene with present='composite' against present=None,
alternating (skipped with --no-pipeline).

    python scripts/present_time.py [--views 16] [--size 512] [--rounds 7] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'relightable-nr_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

DEV = 'cuda:0'


def byte_model(mode, npix, lp):
    """Least bytes a call moves: 12 B/px of frame and 3 B/px out ('frame'), + 4 B/px of alpha ('composite'), 3 B/px out alone
    ('background'); the probe once on top (it stays L2-resident at 100 x 200 — 240 KB — and not at 1600 x 3200 — 61 MB)."""
    per_px = {'frame': 15, 'composite': 19, 'background': 3}[mode]
    return per_px * npix + (0 if mode == 'frame' else lp.numel() * 4)


def chain(image, alpha, proj_inv, R_inv, lp, mode):
    """B: the bytes of present_u8 from the drop-in operators and torch ops."""
    import render
    from rnr_amd import ops
    S = image.shape[-1]
    frame = image.permute(0, 2, 3, 1)
    if mode == 'frame':
        x = frame
    else:
        vd, _ = ops.view_dir_map((S, S), proj_inv, R_inv)
        uv = render.spherical_mapping_batch(-vd.transpose(1, -1)).transpose(1, -1)
        hl, wl = lp.shape[0], lp.shape[1]
        bg = ops.interpolate_bilinear(lp, (uv[..., 0] * float(wl)).clamp(max=wl - 1), (uv[..., 1] * float(hl)).clamp(max=hl - 1))
        x = bg if mode == 'background' else torch.where((alpha > 0)[..., None], frame, bg)
    return (x * 255.).round().clamp(0, 255).to(torch.uint8).flip(-1)


def window_ms(fn, reps):
    """(device ms per call, host ms per call) over a window of `reps` back-to-back calls between two device events; the host
    figure is the wall time of the enqueue loop alone: where it reaches the device figure, the host's launch rate sets the time."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    host = time.perf_counter() - t0
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps, host * 1e3 / reps


def sized_reps(fn, min_window_s):
    """Calls per window so that a window lasts min_window_s or more: grown from a short probe until a whole window has been
    seen to last that long (a 5-call probe alone is dominated by launch latency and undersizes the window)."""
    reps = 5
    while True:
        window_s = window_ms(fn, reps)[0] * reps / 1e3
        if window_s >= min_window_s:
            return reps
        reps = int(np.ceil(reps * 1.25 * min_window_s / max(window_s, 1e-6)))


def ab(fa, fb, rounds, min_window_s=0.2):
    """Medians (ms per call) of fa and fb, alternating; every window lasts min_window_s or more (asserted)."""
    for f in (fa, fb):
        for _ in range(3):
            f()
    reps = [sized_reps(f, min_window_s) for f in (fa, fb)]
    ta, tb, ha, hb = [], [], [], []
    for _ in range(rounds):
        d, h = window_ms(fa, reps[0]); ta.append(d); ha.append(h)
        d, h = window_ms(fb, reps[1]); tb.append(d); hb.append(h)
    windows = (reps[0] * min(ta) / 1e3, reps[1] * min(tb) / 1e3)
    assert min(windows) >= 0.9 * min_window_s, windows
    return {'a_ms': statistics.median(ta), 'b_ms': statistics.median(tb), 'a_spread': (min(ta), max(ta)), 'b_spread': (min(tb), max(tb)),
            'a_host_ms': statistics.median(ha), 'b_host_ms': statistics.median(hb), 'reps': reps, 'shortest_window_s': windows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--views', type=int, default=16)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--no-pipeline', action='store_true')
    ap.add_argument('--out', default=None, help='also write the result lines to this file')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('present_time.py needs the GPU: a CPU run measures nothing')
    from rnr_amd import ops, scene, testing
    N, S = args.views, args.size
    npix = N * S * S
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    rng = np.random.default_rng(0)
    ids = [int(i) for i in np.linspace(5, 700, N)]
    v = {k: torch.from_numpy(x).to(DEV) for k, x in scene.spiral_views(S, ids).items()}
    image = torch.from_numpy(rng.random((N, 3, S, S), dtype=np.float32)).to(DEV)
    yy, xx = np.mgrid[:S, :S]
    disk = (((yy - S / 2) ** 2 + (xx - S / 2) ** 2) < (0.4 * S) ** 2).astype(np.float32)       # about half of the pixels
    alphas = {'half covered': torch.from_numpy(np.broadcast_to(disk, (N, S, S)).copy()).to(DEV),
              'all background': torch.zeros(N, S, S, device=DEV)}
    probes = {'100x200': torch.as_tensor(testing.synthetic_light_probe(100, 200), dtype=torch.float32).reshape(100, 200, 3).contiguous().to(DEV)}
    big = torch.nn.functional.interpolate(probes['100x200'].permute(2, 0, 1)[None], size=(1600, 3200), mode='bilinear', align_corners=False)
    probes['1600x3200'] = big[0].permute(1, 2, 0).contiguous()
    say('present_time: %d views of %d x %d (%d pixels); byte model: frame 15 B/px, composite 19 B/px (%.1f MB), background 3 B/px, + the probe'
        % (N, S, S, npix, 19 * npix / 1e6))
    say('%-11s %-15s %-10s %9s %9s %7s %9s %9s %9s %9s  %s' % ('mode', 'alpha', 'probe', 'A ms', 'B ms', 'B/A', 'A GB/s', 'B GB/s', 'A host ms',
                                                             'windows s', 'A vs B bytes'))
    results = []
    cases = [('frame', 'half covered', '100x200')]
    for pn in probes:
        cases += [('composite', 'half covered', pn), ('composite', 'all background', pn), ('background', 'all background', pn)]
    for mode, an, pn in cases:
        alpha, lp = alphas[an], probes[pn]
        out = torch.empty(N, S, S, 3, dtype=torch.uint8, device=DEV)
        fa = lambda: ops.present_u8(image, alpha, v['proj_inv'], v['R_inv'], lp, mode=mode, out=out)
        fb = lambda: chain(image, alpha, v['proj_inv'], v['R_inv'], lp, mode)
        diff = (fa().int() - fb().int()).abs()
        r = ab(fa, fb, args.rounds)
        model = byte_model(mode, npix, lp)
        r.update(mode=mode, alpha=an, probe=pn, model_bytes=model, a_gbs=model / r['a_ms'] / 1e6, b_gbs=model / r['b_ms'] / 1e6,
                 max_byte_diff=int(diff.max()), share_bytes_differ=float((diff > 0).float().mean()))
        results.append(r)
        say('%-11s %-15s %-10s %9.4f %9.4f %7.1f %9.0f %9.0f %9.4f %4.2f/%4.2f  max %d, %.2e differ'
            % (mode, an, pn, r['a_ms'], r['b_ms'], r['b_ms'] / r['a_ms'], r['a_gbs'], r['b_gbs'], r['a_host_ms'], r['shortest_window_s'][0],
               r['shortest_window_s'][1], r['max_byte_diff'], r['share_bytes_differ']))
    pipe_res = None
    if not args.no_pipeline:
        from rnr_amd.pipeline import RNRPipeline
        ps, pd = testing.ray_pivots(6, 2, 5), testing.ray_pivots(6, 2, 10)
        mk = lambda present: RNRPipeline(scene.uv_sphere(128, 256), S, testing.synthetic_textures(512, 24, 4, 0),
                                         testing.unet_state_dict(108, 78, 64, 5, 0), ps, pd, None, nf0=64, max_views=N, device=DEV,
                                         sh_coeff=torch.from_numpy(scene.synthetic_sh_coeff(2, 10, 1)), sh_lmax=10, present=present)
        off, on = mk(None), mk('composite')
        a = (v['proj'], v['pose'], v['proj_inv'], v['R_inv'])
        r = ab(lambda: on.render(*a), lambda: off.render(*a), args.rounds, min_window_s=0.5)
        same = bool(torch.equal(on.render(*a), off.render(*a)))
        pipe_res = dict(r, float_frames_identical=same)
        say("RNRPipeline(max_views=%d) step: present='composite' %.3f ms (%.3f .. %.3f), present=None %.3f ms (%.3f .. %.3f): %+.3f ms, %+.2f %%; "
            'float frames identical: %s' % (N, r['a_ms'], r['a_spread'][0], r['a_spread'][1], r['b_ms'], r['b_spread'][0], r['b_spread'][1],
                                            r['a_ms'] - r['b_ms'], 100 * (r['a_ms'] / r['b_ms'] - 1), same))
    say(json.dumps({'present_time': {'views': N, 'size': S, 'device': torch.cuda.get_device_name(0), 'cases': results, 'pipeline': pipe_res}}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
