"""Timing of the OpenEXR route (rnr_amd/exr.py, csrc/exr.hip) on a 3000 x 4000 half RGB ZIP photograph to 512 x 512 with gamma 2.2
(what dataio.ViewDataset(load_img=True) runs once per .exr photograph), stage by stage:

  (a) host: read + validate + inflate   rnr_amd.exr.load (zlib on a thread pool of at most 16), host wall time;
  (b) upload                            the chunk bytes and the table from pageable host memory;
  (c) unpack kernel                     ops.exr_unpack on bytes already on the device, beside its byte floor (payload read + raw
                                        written; the kernel reads the lower half of a coded chunk twice) at the copy rate
                                        scripts/micro/hbm_bw_probe.py measures in the same run;
  (d) prepare kernel                    ops.photo_prepare_hdr on the raw scanlines, beside its floor (the crop's bytes + the output);
  (e) the whole route                   ops.read_exr: (a) + (b) + (c) + (d);
  (f) the host route on the same file   (a), then numpy: cumsum + interleave per chunk, astype(float32), crop; the float window
                                        uploaded, ops.resize_area, torch's pow, a permute to [3,S,S].

Device events around windows of back-to-back calls (each --window s or more), a warm-up, medians over --rounds rounds with the range
next to them; stages with host work have their host wall time per call beside the device figure.  The file is written by the
tests' restatement of the format (tests/exr_ref.py): a smooth image with noise, so that deflate shrinks it as it would a photograph.

    python scripts/exr_time.py [--size 512] [--gamma 2.2] [--rounds 5] [--window 0.2] [--out profiles/exr_time.txt]
"""
import argparse
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'relightable-nr_amd'), os.path.join(ROOT, 'scripts'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

from photo_prepare_time import measure  # noqa: E402

DEV = 'cuda:0'
H, W = 3000, 4000


def host_ms(fn, n=5):
    times = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--gamma', type=float, default=2.2)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--window', type=float, default=0.2)
    ap.add_argument('--out', default=None, help='also write the result lines to this file')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('exr_time.py needs the GPU: a CPU run measures nothing')
    probe = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'micro', 'hbm_bw_probe.py')], capture_output=True, text=True,
                           timeout=300)
    m = re.search(r'copy \(read \+ write\) ([0-9.]+) TB/s', probe.stdout)
    if probe.returncode != 0 or not m:
        raise SystemExit('exr_time.py: scripts/micro/hbm_bw_probe.py failed:\n%s\n%s' % (probe.stdout, probe.stderr[-2000:]))
    copy_tbs = float(m.group(1))
    import exr_ref
    from rnr_amd import capture, exr, ops
    S, lines = args.size, []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('exr_time: %d x %d half RGB ZIP photograph to %d x %d, gamma %g, on %s' % (H, W, S, S, args.gamma, torch.cuda.get_device_name(0)))
    say('  hbm_bw_probe: %s' % probe.stdout.strip().splitlines()[0])
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    rng = np.random.RandomState(H)
    chans = {k: (0.6 + 0.5 * np.sin(xx / 97 + i) * np.cos(yy / 131 - i) + rng.normal(0, 0.01, (H, W))).clip(1e-3).astype(np.float16)
             for i, k in enumerate('RGB')}
    with tempfile.TemporaryDirectory() as tmp:
        fp = os.path.join(tmp, 'photo.exr')
        how = exr_ref.write(fp, chans, compression=exr_ref.ZIP)
        file_mb = os.path.getsize(fp) / 1e6
        header, payload, table = exr.load(fp)
        raw_bytes = header.height * header.row_bytes
        say('  file %.1f MB, %d chunks (%d deflated, %d stored raw), raw scanlines %.1f MB, chunk %.0f KB = %d passes of %d bytes'
            % (file_mb, len(how), how.count('deflate'), how.count('raw'), raw_bytes / 1e6, table[0][2] / 1e3,
               -(-table[0][2] // pass_bytes()), pass_bytes()))
        _, _, y0, x0, side = capture.crop_geometry(H, W)
        crop, layout = (y0, x0, side, side), exr.rgb_layout(header)
        table_cpu = torch.tensor(table, dtype=torch.int64)
        dev_payload = torch.frombuffer(payload, dtype=torch.uint8).to(DEV)
        dev_table = table_cpu.to(DEV)
        raw = torch.empty(raw_bytes, dtype=torch.uint8, device=DEV)
        out = torch.empty(3, S, S, device=DEV)

        def upload():
            return torch.frombuffer(payload, dtype=torch.uint8).to(DEV), table_cpu.to(DEV)

        def unpack():
            ops.exr_unpack(dev_payload, dev_table, out=raw)

        def prepare():
            ops.photo_prepare_hdr(raw, (H, W), header.row_bytes, layout, crop, (S, S), args.gamma, out=out)

        def whole():
            return ops.read_exr(fp, DEV, crop, (S, S), args.gamma)

        def host_decode():
            """The numpy restatement of the unpack on the inflated payload -> the float32 crop window [side,side,3]."""
            buf = np.frombuffer(payload, np.uint8)
            rows = np.empty(raw_bytes, np.uint8)
            for src, dst, n, coded in table:
                t = buf[src:src + n]
                if coded:
                    d = t.astype(np.int64) - 128
                    d[0] = t[0]
                    s = np.cumsum(d).astype(np.uint8)
                    half = (n + 1) // 2
                    rows[dst:dst + n:2] = s[:half]
                    rows[dst + 1:dst + n:2] = s[half:]
                else:
                    rows[dst:dst + n] = t
            img = rows.reshape(H, header.row_bytes)
            win = np.stack([img[y0:y0 + side, o:o + 2 * W].view(np.float16)[:, x0:x0 + side].astype(np.float32)
                            for o, _, _ in layout], -1)
            return np.ascontiguousarray(win)

        def host_route():
            exr.load(fp)
            r = ops.resize_area(torch.from_numpy(host_decode()).to(DEV), S, S)
            return torch.pow(r, args.gamma).permute(2, 0, 1).contiguous()

        unpack()
        prepare()
        got = whole()
        ref = host_route()
        assert torch.equal(got, out)
        say('  crop %d x %d at (%d, %d), %.1f source pixels per output pixel; host route against the kernels: max |difference| %.3e '
            '(torch.pow in float32 against the rounded float64 power)' % (side, side, y0, x0, (side / S) ** 2, float((ref - got).abs().max())))
        med, lo, hi = host_ms(lambda: exr.load(fp))
        say('    %-52s %10.3f ms  [%.3f .. %.3f]   host wall time' % ('(a) host: read + validate + inflate (exr.load)', med, lo, hi))
        med1, lo1, hi1 = host_ms(lambda: exr.load(fp, workers=1), 3)
        say('    %-52s %10.3f ms  [%.3f .. %.3f]   host wall time' % ('    the same on one thread', med1, lo1, hi1))
        results = {}
        for name, fn in (('(b) upload of %.1f MB' % (len(payload) / 1e6), upload), ('(c) unpack kernel', unpack),
                         ('(d) prepare kernel', prepare), ('(e) the whole route (ops.read_exr)', whole),
                         ('(f) the host route: numpy decode, upload, resize, pow', host_route)):
            med, lo, hi, host = measure(fn, args.rounds, args.window)
            results[name[:3]] = med
            say('    %-52s %10.3f ms  [%.3f .. %.3f]   host %.3f ms per call' % (name, med, lo, hi, host))
        coded_bytes = sum(r[2] for r in table if r[3])
        unpack_floor = (len(payload) + coded_bytes / 2 + raw_bytes) / (copy_tbs * 1e12) * 1e6
        prepare_floor = (side * side * 6 + 3 * S * S * 4) / (copy_tbs * 1e12) * 1e6
        say('    byte floor of (c): %.1f MB read (the lower half of a coded chunk twice) + %.1f MB written at the copy rate %.2f TB/s '
            '= %.1f us: the kernel takes %.1f x that' % ((len(payload) + coded_bytes / 2) / 1e6, raw_bytes / 1e6, copy_tbs,
                                                      unpack_floor, results['(c)'] * 1e3 / unpack_floor))
        say('    byte floor of (d): %.1f MB of crop read + %.1f MB written = %.1f us: the kernel takes %.1f x that'
            % (side * side * 6 / 1e6, 3 * S * S * 4 / 1e6, prepare_floor, results['(d)'] * 1e3 / prepare_floor))
        say('    (f) / (e) = %.1f' % (results['(f)'] / results['(e)']))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


def pass_bytes():
    from rnr_amd import _lib
    return _lib.EXR_PASS_BYTES


if __name__ == '__main__':
    main()
