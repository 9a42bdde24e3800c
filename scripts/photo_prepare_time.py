"""Timing of rnr_photo_prepare (csrc/photo.hip) at two photograph sizes, 3000 x 4000 x 3 and 1080 x 1920 x 3 uint8, to 512 x 512
with gamma 2.2 (what dataio.ViewDataset(load_img=True) runs once per photograph):

  (a) kernel            ops.photo_prepare on a photograph already on the device;
  (b) upload + kernel   the uint8 photograph from pageable host memory, then (a): what read_view adds to the decode;
  (c) before            what the project could do before this operator: host astype(float32) / 255 and crop, the float window
                        uploaded, ops.resize_area, torch's pow, a permute to [3,S,S];
  beside them           PIL's decode of the same photograph from a PNG and from a JPEG in memory (host, once each), and the byte
                        floor of (a): the crop's bytes read + the output written at the copy rate scripts/micro/hbm_bw_probe.py
                        measures in the same run.

Device events around windows of back-to-back calls (each --window s or more), a warm-up, medians over --rounds rounds with the
range next to them; (b) and (c) contain host work, so their host wall time per call stands beside the device figure.

    python scripts/photo_prepare_time.py [--size 512] [--gamma 2.2] [--rounds 5] [--window 0.2] [--out profiles/photo_prepare_time.txt]
"""
import argparse
import io
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'relightable-nr_amd'), os.path.join(ROOT, 'scripts')):
    if p not in sys.path:
        sys.path.insert(0, p)

from present_time import sized_reps, window_ms  # noqa: E402

DEV = 'cuda:0'
PHOTOS = [(3000, 4000, 3), (1080, 1920, 3)]


def measure(fn, rounds, window):
    """(median device ms, min, max, median host ms) per call."""
    for _ in range(2):
        fn()
    reps = sized_reps(fn, window)
    t = [window_ms(fn, reps) for _ in range(rounds)]
    dev = [a for a, _ in t]
    return statistics.median(dev), min(dev), max(dev), statistics.median([b for _, b in t])


def decode_ms(u8, fmt):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(u8).save(buf, format=fmt, **({'quality': 90} if fmt == 'JPEG' else {}))
    data = buf.getvalue()
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        np.array(Image.open(io.BytesIO(data)), dtype=np.uint8)
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), len(data)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--gamma', type=float, default=2.2)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--window', type=float, default=0.2)
    ap.add_argument('--out', default=None, help='also write the result lines to this file')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('photo_prepare_time.py needs the GPU: a CPU run measures nothing')
    probe = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'micro', 'hbm_bw_probe.py')], capture_output=True, text=True,
                           timeout=300)
    m = re.search(r'copy \(read \+ write\) ([0-9.]+) TB/s', probe.stdout)
    if probe.returncode != 0 or not m:
        raise SystemExit('photo_prepare_time.py: scripts/micro/hbm_bw_probe.py failed:\n%s\n%s' % (probe.stdout, probe.stderr[-2000:]))
    copy_tbs = float(m.group(1))
    from rnr_amd import capture, ops
    S, lines = args.size, []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('photo_prepare_time: uint8 photographs to %d x %d, gamma %g, on %s' % (S, S, args.gamma, torch.cuda.get_device_name(0)))
    say('  hbm_bw_probe: %s' % probe.stdout.strip().splitlines()[0])
    for h, w, c in PHOTOS:
        # a smooth image with noise on top: a photograph's decode cost depends on its content, pure noise would overstate it
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
        rng = np.random.RandomState(h)
        base = np.stack([128 + 100 * np.sin(xx / 97 + k) * np.cos(yy / 131 - k) for k in range(c)], -1)
        u8 = np.clip(base + rng.normal(0, 6, base.shape), 0, 255).astype(np.uint8)
        _, _, y0, x0, side = capture.crop_geometry(h, w)
        crop = (y0, x0, side, side)
        dev = torch.from_numpy(u8).to(DEV)
        out = torch.empty(3, S, S, device=DEV)

        def kernel():
            ops.photo_prepare(dev, crop, (S, S), args.gamma, out=out)

        def upload_kernel():
            ops.photo_prepare(torch.from_numpy(u8).to(DEV), crop, (S, S), args.gamma, out=out)

        def before():
            win = np.ascontiguousarray((u8.astype(np.float32) / 255.)[y0:y0 + side, x0:x0 + side])
            r = ops.resize_area(torch.from_numpy(win).to(DEV), S, S)
            return torch.pow(r, args.gamma).permute(2, 0, 1).contiguous()

        kernel()
        ref = before()
        same, diff = torch.equal(ref, out), float((ref - out).abs().max())
        floor_us = (side * side * c + 3 * S * S * 4) / (copy_tbs * 1e12) * 1e6
        say('  %d x %d x %d (%.1f MB), crop %d x %d at (%d, %d), %.1f source pixels per output pixel'
            % (h, w, c, u8.nbytes / 1e6, side, side, y0, x0, (side / S) ** 2))
        for name, fn in (('(a) kernel', kernel), ('(b) upload + kernel', upload_kernel), ('(c) before: host / 255 + crop, upload, '
                                                                                         'resize_area, pow', before)):
            med, lo, hi, host = measure(fn, args.rounds, args.window)
            say('    %-58s %10.3f ms  [%.3f .. %.3f]   host %.3f ms per call' % (name, med, lo, hi, host))
        say('    byte floor of (a): %.1f MB of crop read + %.1f MB written at the copy rate %.2f TB/s = %.1f us'
            % (side * side * c / 1e6, 3 * S * S * 4 / 1e6, copy_tbs, floor_us))
        say('    (c) against (a): bit-equal %s, max |difference| %.3e (torch.pow in float32 against the rounded float64 power)'
            % (same, diff))
        for fmt in ('PNG', 'JPEG'):
            ms, nbytes = decode_ms(u8, fmt)
            say('    PIL decode of the %s (%.1f MB), host, median of 3: %.1f ms' % (fmt, nbytes / 1e6, ms))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
