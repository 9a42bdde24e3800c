"""Generates tests/golden/metric/metric_cases.npz from the READ-ONLY reference at /root/reference (build container only).

    python tests/golden/metric/make_metric_golden.py            writes the fixture
    python tests/golden/metric/make_metric_golden.py --check    regenerates it in memory and compares it with the file

The reference's metric.py is loaded by file location with an EMPTY stand-in module registered as `pytorch_msssim` (the
library is not installed; nothing of it is called because every call passes compute_ssim=False), and
compute_err_metrics_batch runs on clones of the inputs (it zeroes its arguments in place).  Stored: the inputs, the nine
non-SSIM outputs as the reference returns them, and the parameter names of its three functions (names only).  Nothing of the
reference's text is copied.  4 views of 23 x 19: about 25 KB.
"""
import importlib.util
import inspect
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import metric_ref as mr  # noqa: E402

REFERENCE = '/root/reference/metric.py'
OUT = os.path.join(HERE, 'metric_cases.npz')
NINE = mr.KEYS[:9]
FUNCTIONS = ('psnr', 'compute_err_metrics', 'compute_err_metrics_batch')


def reference_module():
    sys.modules.setdefault('pytorch_msssim', types.ModuleType('pytorch_msssim'))
    spec = importlib.util.spec_from_file_location('reference_metric', REFERENCE)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert os.path.abspath(mod.__file__) == REFERENCE
    return mod


def generate():
    ref = reference_module()
    N, H, W = 4, 23, 19
    est, gt = mr.noise_images(N, H, W, 20)
    est[2:], gt[2:] = mr.bright_images(2, H, W, 21)
    mask = np.stack([np.ones((H, W), np.float32), mr.blob_mask(H, W, 22), mr.rect_mask(H, W, 4, 17, 6, 19), mr.disc_mask(H, W)])
    res = ref.compute_err_metrics_batch(torch.from_numpy(est).clone(), torch.from_numpy(gt).clone(),
                                        torch.from_numpy(mask)[:, None].clone(), compute_ssim=False)
    out = np.concatenate([np.asarray(res[k], np.float64).reshape(N, 1) for k in NINE], axis=1)
    assert all(len(res[k]) == 0 and np.isnan(res[k + '_mean']) for k in mr.KEYS[9:])
    names = {f: list(inspect.signature(getattr(ref, f)).parameters) for f in FUNCTIONS}
    defaults = {f: [repr(p.default) for p in inspect.signature(getattr(ref, f)).parameters.values() if p.default is not p.empty]
                for f in FUNCTIONS}
    return {'est': est, 'gt': gt, 'mask': mask, 'reference_out': out, 'keys': np.array(json.dumps(list(NINE))),
            'parameters': np.array(json.dumps(names)), 'defaults': np.array(json.dumps(defaults))}


def main(argv):
    data = generate()
    if '--check' in argv:
        have = np.load(OUT)
        bad = [k for k in data if k not in have.files or not np.array_equal(have[k], data[k])] + [k for k in have.files if k not in data]
        print('make_metric_golden --check: %s' % ('OK' if not bad else 'FAILED: %s' % bad))
        return 1 if bad else 0
    np.savez_compressed(OUT, **data)
    print('wrote %s (%d bytes)' % (OUT, os.path.getsize(OUT)))
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
