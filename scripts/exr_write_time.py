"""Timing of the OpenEXR write route (rnr_amd/exr.py, csrc/exr.hip: rnr_exr_pack), stage by stage, for

  a 3000 x 4000 photograph, HALF, ZIP;  a 1600 x 3200 stitched probe, FLOAT, ZIP;  16 frames of 512 x 512, HALF, ZIP, one batch:

  (a) pack kernel           ops.exr_pack(coded = 1) on pixels already on the device, beside its byte floor (12 B/px read, 6 or
                            12 B/px written) at the copy rate scripts/micro/hbm_bw_probe.py measures in the same run;
  (b) download              the coded bytes into pinned host memory;
  (c) deflate               rnr_amd.exr.deflate_chunks on 16 threads and on one, host wall time;
  (d) the whole route       ops.write_exr / ops.write_exr_batch: (a) + (b) + (c) + the file;
  (e) the host coding       the same coded bytes made on the host, vectorised numpy: download of the float32 pixels, astype(float16),
                            planar B,G,R reorder, split into even and odd bytes, differences, per chunk; checked equal to (a)'s.

Device events around windows of back-to-back calls (each --window s or more), a warm-up, medians over --rounds rounds with the range
next to them; host stages are medians of --rounds wall times.  The images are smooth with noise, so that deflate shrinks them
as it would a photograph.

    python scripts/exr_write_time.py [--rounds 5] [--window 0.2] [--out profiles/exr_write_time.txt]
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'relightable-nr_amd'), os.path.join(ROOT, 'scripts')):
    if p not in sys.path:
        sys.path.insert(0, p)

from exr_time import host_ms  # noqa: E402
from photo_prepare_time import measure  # noqa: E402

DEV = 'cuda:0'
CASES = [('3000 x 4000 photograph, HALF, ZIP', 1, 3000, 4000, 'half'),
         ('1600 x 3200 stitched probe, FLOAT, ZIP', 1, 1600, 3200, 'float'),
         ('16 frames of 512 x 512, HALF, ZIP, one batch', 16, 512, 512, 'half')]


def images(n, h, w):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    rng = np.random.RandomState(h)
    return np.stack([np.stack([(0.6 + 0.5 * np.sin(xx / 97 + i + k) * np.cos(yy / 131 - i) + rng.normal(0, 0.01, (h, w))).clip(1e-3)
                               for i in range(3)]) for k in range(n)]).astype(np.float32)


def host_coding(pixels, dtype, lines):
    """float32 [N,3,H,W] on the host -> the coded bytes of every chunk of every image, one array [N, H * row_bytes]."""
    n, _, h, w = pixels.shape
    rows = np.ascontiguousarray(pixels.astype(dtype)[:, ::-1].transpose(0, 2, 1, 3)).view(np.uint8).reshape(n, h, -1)
    out = np.empty((n, h * rows.shape[2]), np.uint8)
    step = lines * rows.shape[2]
    for k in range(n):
        raw = rows[k].reshape(-1)
        for p in range(0, raw.size, step):
            c = raw[p:p + step]
            split = np.concatenate([c[0::2], c[1::2]])
            o = out[k, p:p + c.size]
            o[0] = split[0]
            np.subtract(split[1:], split[:-1], out=o[1:])
            o[1:] += 128
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--window', type=float, default=0.2)
    ap.add_argument('--out', default=None, help='also write the result lines to this file')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('exr_write_time.py needs the GPU: a CPU run measures nothing')
    probe = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'micro', 'hbm_bw_probe.py')], capture_output=True, text=True,
                           timeout=300)
    m = re.search(r'copy \(read \+ write\) ([0-9.]+) TB/s', probe.stdout)
    if probe.returncode != 0 or not m:
        raise SystemExit('exr_write_time.py: scripts/micro/hbm_bw_probe.py failed:\n%s\n%s' % (probe.stdout, probe.stderr[-2000:]))
    copy_tbs = float(m.group(1))
    from rnr_amd import _lib, exr, ops
    lines_out = []

    def say(s):
        print(s, flush=True)
        lines_out.append(s)

    say('exr_write_time on %s' % torch.cuda.get_device_name(0))
    say('  hbm_bw_probe: %s' % probe.stdout.strip().splitlines()[0])
    with tempfile.TemporaryDirectory() as tmp:
        for title, n, h, w, ptype in CASES:
            code = exr.pixel_type_code(ptype)
            size = exr.TYPE_BYTES[code]
            pixels = images(n, h, w)
            dev = torch.from_numpy(pixels).to(DEV)
            _, lines, sizes = exr.chunk_sizes(w, h, code, 'zip')
            per = sum(sizes)
            packed = torch.empty(n, per, dtype=torch.uint8, device=DEV)
            pinned = torch.empty(n * per, dtype=torch.uint8, pin_memory=True)
            paths = [os.path.join(tmp, 'out_%d.exr' % k) for k in range(n)]

            def pack():
                ops.exr_pack(dev, code, lines, 1, channels_last=False, out=packed)

            def download():
                pinned.copy_(packed.view(-1))

            def whole():
                return ops.write_exr_batch(paths, dev, ptype, 'zip') if n > 1 else [ops.write_exr(paths[0], dev[0], ptype, 'zip')]

            pack()
            download()
            buf = memoryview(pinned.numpy())
            chunks, pos = [], 0
            for _ in range(n):
                for s in sizes:
                    chunks.append(buf[pos:pos + s])
                    pos += s
            how = whole()
            file_mb = sum(os.path.getsize(p) for p in paths) / 1e6
            coded_host = host_coding(pixels, np.float16 if ptype == 'half' else np.float32, lines)
            assert coded_host.tobytes() == bytes(buf), 'the host coding and the kernel disagree'
            say('%s: %d chunks of %.0f KB (%d deflated, %d stored raw), coded bytes %.1f MB, files %.1f MB'
                % (title, len(chunks), sizes[0] / 1e3, sum(x.count('deflate') for x in how), sum(x.count('raw') for x in how),
                   n * per / 1e6, file_mb))
            med, lo, hi, host = pack_ms = measure(pack, args.rounds, args.window)
            floor = n * h * w * (12 + 3 * size) / (copy_tbs * 1e12) * 1e6
            say('    %-52s %10.3f ms  [%.3f .. %.3f]   host %.3f ms per call' % ('(a) pack kernel', med, lo, hi, host))
            say('        byte floor: %.1f MB read + %.1f MB written at the copy rate %.2f TB/s = %.1f us: the kernel takes %.1f x that'
                % (n * h * w * 12 / 1e6, n * per / 1e6, copy_tbs, floor, med * 1e3 / floor))
            med, lo, hi, host = down_ms = measure(download, args.rounds, args.window)
            say('    %-52s %10.3f ms  [%.3f .. %.3f]   host %.3f ms per call' % ('(b) download of %.1f MB into pinned memory' % (n * per / 1e6), med, lo, hi, host))
            d16 = host_ms(lambda: exr.deflate_chunks(chunks, 6), args.rounds)
            say('    %-52s %10.3f ms  [%.3f .. %.3f]   host wall time' % (('(c) deflate, level 6, %d threads' % exr.MAX_INFLATE_WORKERS,) + d16))
            d1 = host_ms(lambda: exr.deflate_chunks(chunks, 6, workers=1), 3)
            say('    %-52s %10.3f ms  [%.3f .. %.3f]   host wall time' % (('    the same on one thread',) + d1))
            wh = host_ms(whole, args.rounds)
            say('    %-52s %10.3f ms  [%.3f .. %.3f]   host wall time' % (('(d) the whole route (ops.write_exr%s)' % ('_batch' if n > 1 else ''),) + wh))
            hc = host_ms(lambda: host_coding(dev.cpu().numpy(), np.float16 if ptype == 'half' else np.float32, lines), args.rounds)
            say('    %-52s %10.3f ms  [%.3f .. %.3f]   host wall time' % (('(e) the host coding: download, numpy astype .. differences',) + hc))
            say('    (e) / ((a) + (b)) = %.0f;  deflate is %.0f %% of (d)' % (hc[0] / (pack_ms[0] + down_ms[0]), 100 * d16[0] / wh[0]))
            del dev, packed, pinned, buf, chunks
    say('  segment of one workgroup: %d units of 16 bits (%d bytes of a chunk)' % (_lib.EXR_PACK_SEGMENT, 2 * _lib.EXR_PACK_SEGMENT))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines_out) + '\n')


if __name__ == '__main__':
    main()
