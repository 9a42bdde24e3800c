"""All 720 spiral_step720 views of the bench scene rendered with precision='f16' (RNR_CONV_F16: fp16 operands, fp32
accumulation) and with the exact-fp32 convolutions, the yardstick: per-view PSNR (peak 1, like oracle.psnr; frames take values
in about [0, 2]) and max |difference| of the f16 frame against the exact one, and the same after quantisation to 8 bits as
cv2.imwrite gets them.  'f16x3' runs alongside for scale, and the exact path against itself gives the run-to-run floor
(BatchNorm statistics are float64 atomics).
Usage (GPU box): python scripts/f16_frames_720.py > f16_frames_720.txt   (profiles/f16_accuracy.txt holds it)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'relightable-nr_amd'))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from rnr_amd import scene  # noqa: E402


def main():
    args = bench.parse([])
    sc = bench.build_scene(args)
    dev = torch.device('cuda', 0)
    V = 8
    pv = {k: torch.from_numpy(v).to(dev) for k, v in scene.spiral_views(512, np.arange(720)).items()}
    others = ('f16', 'f16x3')
    pipes = {p: bench.make_pipeline(sc, args, dev, V, precision=p, skip_background_tiles=False) for p in ('f32',) + others}
    stats = {p: {'max_abs': [], 'psnr': [], 'grey': []} for p in others}
    run2 = []
    u8 = lambda img: (img.clamp(0.0, 1.0) * 255.0).round()
    for lo in range(0, 720, V):
        sl = slice(lo, lo + V)
        a = [pv[k][sl] for k in ('proj', 'pose', 'proj_inv', 'R_inv')]
        ref = pipes['f32'].render(*a).clone()
        run2 += (pipes['f32'].render(*a) - ref).abs().flatten(1).max(1).values.tolist()
        for p in others:
            img = pipes[p].render(*a)
            d = img - ref
            stats[p]['max_abs'] += d.abs().flatten(1).max(1).values.tolist()
            stats[p]['psnr'] += (10.0 * torch.log10(1.0 / d.pow(2).flatten(1).mean(1).clamp_min(1e-30))).tolist()
            stats[p]['grey'] += (u8(img) - u8(ref)).abs().flatten(1).max(1).values.tolist()
    print('f16_frames_720: %s; bench.py build_scene (UV sphere 65 536 faces, nf0 = 64), 720 spiral views at 512 x 512, %d per call,'
          % (torch.cuda.get_device_name(0), V))
    print('every tile computed; yardstick: the exact-fp32 frames (conv_algo %s) of the same run' % pipes['f32'].unet.conv_algo)
    print('exact-fp32 run to run: max |diff| %.3g (median %.3g)' % (float(np.max(run2)), float(np.median(run2))))
    for p in others:
        m, q, g = (np.asarray(stats[p][k]) for k in ('max_abs', 'psnr', 'grey'))
        print('%-6s PSNR vs exact fp32: min %.2f dB (view %d), 1st percentile %.2f, median %.2f;  max |diff| max %.3g, median %.3g;  '
              '8-bit frames: largest difference %d grey level%s, %d of 720 views differ by more than one'
              % (p, q.min(), int(q.argmin()), np.percentile(q, 1), np.median(q), m.max(), np.median(m), int(g.max()),
                 '' if int(g.max()) == 1 else 's', int((g > 1).sum())))


if __name__ == '__main__':
    main()
