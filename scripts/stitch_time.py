"""Timing of the light-probe stitch (csrc/stitch.hip) at the size the reference's stitch_lp.py runs: 16 views of 512 x 512 of the
benchmark scene (its spiral cameras around the unit sphere; the coverage is the sphere's disc, the photographs' backgrounds are
the synthetic probe seen through rnr_env_background) into a 1600 x 3200 probe.

  LightProbeStitcher.add (background mask + the two stitch passes) and .result (finalize), then each entry point alone, with the
  bytes it moves (counted from the shapes and from the number of background pixels and winners of this input) against the
  copy rate scripts/micro/hbm_bw_probe.py measures in the same run;
  the numpy formulation of the same views (tests/stitch_ref.py: float64, what stitch_lp.py does per view) on this box's CPU,
  once, and whether the two agree.

Device events around windows of back-to-back calls (each --window s or more), a warm-up, medians over --rounds rounds with the
range next to them; the host's enqueue time per call stands beside each device time.

    python scripts/stitch_time.py [--views 16] [--size 512] [--rounds 5] [--window 0.2] [--out profiles/stitch_time.txt]
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'relightable-nr_amd'), os.path.join(ROOT, 'scripts'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

from present_time import sized_reps, window_ms  # noqa: E402

DEV = 'cuda:0'


def measure(fn, rounds, window):
    """(median device ms, min, max, median host ms) per call."""
    for _ in range(2):
        fn()
    reps = sized_reps(fn, window)
    t = [window_ms(fn, reps) for _ in range(rounds)]
    dev = [a for a, _ in t]
    return statistics.median(dev), min(dev), max(dev), statistics.median([b for _, b in t])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--views', type=int, default=16)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--lp_h', type=int, default=1600)
    ap.add_argument('--lp_w', type=int, default=3200)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--window', type=float, default=0.2)
    ap.add_argument('--out', default=None, help='also write the result lines to this file')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('stitch_time.py needs the GPU: a CPU run measures nothing')
    probe = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'micro', 'hbm_bw_probe.py')], capture_output=True, text=True,
                           timeout=300)
    m = re.search(r'copy \(read \+ write\) ([0-9.]+) TB/s', probe.stdout)
    if probe.returncode != 0 or not m:
        raise SystemExit('stitch_time.py: scripts/micro/hbm_bw_probe.py failed:\n%s\n%s' % (probe.stdout, probe.stderr[-2000:]))
    copy_tbs = float(m.group(1))
    import stitch_ref as sr
    from rnr_amd import ops, scene
    from rnr_amd.lighting import LightProbeStitcher
    N, S, lp_h, lp_w = args.views, args.size, args.lp_h, args.lp_w
    T, P = lp_h * lp_w, N * S * S
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ids = (np.arange(N) * (720 // N)) % 720
    views = scene.spiral_views(S, ids)
    Pi, Ri = torch.from_numpy(views['proj_inv']).to(DEV), torch.from_numpy(views['R_inv']).to(DEV)
    yy, xx = np.mgrid[0:S, 0:S] + 0.5
    disc = ((yy - S / 2) ** 2 + (xx - S / 2) ** 2 < (1.2 * S / np.sqrt(8.0)) ** 2).astype(np.float32)     # unit sphere from radius 3
    alpha = torch.from_numpy(np.repeat(disc[None], N, 0)).to(DEV)
    env = scene.synthetic_light_probe(400, 800, 2)[0].to(DEV)
    photos = ops.env_background(Pi, Ri, env, (S, S))                                                     # [N,S,S,3]
    radius = LightProbeStitcher.default_radius(S, S)
    st = LightProbeStitcher(lp_h, lp_w, device=DEV)
    st.add(photos, Pi, Ri, alpha=alpha, radius=radius, channels_last=True)
    first = st.result()
    bg = ops.background_mask(alpha, radius)
    B, winners, touched = int(bg.sum()), int(first.count.sum()), int((first.count > 0).sum())
    say('stitch_time: %d views of %d x %d into %d x %d, dilation radius %d, on %s' % (N, S, S, lp_h, lp_w, radius, torch.cuda.get_device_name(0)))
    say('  hbm_bw_probe: %s' % probe.stdout.strip().splitlines()[0])
    say('  %d background pixels (%.1f %% of the views), %d winners (texel, view), %d texels seen (%.1f %% of the probe)'
        % (B, 100.0 * B / P, winners, touched, 100.0 * touched / T))
    Pi64, Ri64 = Pi.double(), Ri.double()
    total, count = torch.zeros(lp_h, lp_w, 3, dtype=torch.float64, device=DEV), torch.zeros(lp_h, lp_w, dtype=torch.int32, device=DEV)
    ws = torch.zeros(N * T, dtype=torch.int32, device=DEV)
    lp, mask = torch.empty(lp_h, lp_w, 3, device=DEV), torch.empty(lp_h, lp_w, dtype=torch.uint8, device=DEV)
    bytes_of = {
        'LightProbeStitcher.add': None, 'LightProbeStitcher.result': None,
        'rnr_background_mask': 5 * P,
        # pass 1: the mask bytes and one 4-byte atomic per background pixel; pass 2: every winner word read, the non-zero ones
        # cleared, 12 bytes fetched per winner, 28 bytes of state read and written per texel seen
        'rnr_stitch_accumulate': P + 4 * B + 4 * N * T + 4 * winners + 12 * winners + 2 * 28 * touched,
        'rnr_stitch_finalize': (24 + 4 + 12 + 1) * T,
        'rnr_probe_prepare (gamma 2.2)': (12 + 1 + 12) * T + (1 + 12) * T,
    }
    fns = {
        'LightProbeStitcher.add': lambda: st.add(photos, Pi64, Ri64, alpha=alpha, radius=radius, channels_last=True),
        'LightProbeStitcher.result': st.result,
        'rnr_background_mask': lambda: ops.background_mask(alpha, radius, out=bg),
        'rnr_stitch_accumulate': lambda: ops.stitch_accumulate(photos, bg, Pi64, Ri64, total, count, ws, channels_last=True),
        'rnr_stitch_finalize': lambda: ops.stitch_finalize(total, count, lp, mask),
        'rnr_probe_prepare (gamma 2.2)': lambda: ops.probe_prepare(first.lp, first.mask, 2.2, out=lp),
    }
    r = {}
    for k, fn in fns.items():
        r[k] = measure(fn, args.rounds, args.window)
        med, lo, hi, host_ms = r[k]
        rate = '' if bytes_of[k] is None else '   %7.1f MB, %.2f TB/s' % (bytes_of[k] / 1e6, bytes_of[k] / (med * 1e-3) / 1e12)
        say('  %-32s %8.3f ms  (%.3f .. %.3f)   host enqueue %.3f ms%s' % (k, med, lo, hi, host_ms, rate))
    say('  copy rate of this run %.2f TB/s; the bytes are counted from the shapes and this input\'s counts, not measured' % copy_tbs)
    # the numpy formulation on this box's CPU, once (it takes seconds), and whether the two agree
    img_h, bg_h = photos.cpu().numpy(), bg.cpu().numpy() != 0
    t0 = time.perf_counter()
    ref = sr.stitch(img_h, bg_h, views['proj_inv'].astype(np.float64), views['R_inv'].astype(np.float64), lp_h, lp_w)
    t_cpu = time.perf_counter() - t0
    same_count = bool(np.array_equal(ref['count'], first.count.cpu().numpy()))
    same_lp = float((ref['lp'].view(np.uint32) == first.lp.cpu().numpy().view(np.uint32)).mean())
    say('  numpy formulation (float64, one thread of this box\'s CPU): %.2f s; minimum tie distance %.2e; count equal: %s; '
        'lp words bit-equal: %.6f' % (t_cpu, ref['tie'], same_count, same_lp))
    add_ms = r['LightProbeStitcher.add'][0]
    say('  numpy / (add + result) = %.0f' % (t_cpu * 1e3 / (add_ms + r['LightProbeStitcher.result'][0])))
    say(json.dumps({'stitch_time': {'views': N, 'size': S, 'probe': [lp_h, lp_w], 'device': torch.cuda.get_device_name(0),
                                    'copy_tb_s': copy_tbs, 'background_pixels': B, 'winners': winners, 'texels_seen': touched,
                                    'times_ms': {k: v[0] for k, v in r.items()}, 'host_ms': {k: v[3] for k, v in r.items()},
                                    'bytes': bytes_of, 'numpy_s': t_cpu, 'count_equal': same_count, 'lp_words_equal': same_lp}}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
