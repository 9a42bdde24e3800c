"""Generates tests/golden/chrom_loss.npz from the READ-ONLY reference (build container only, through ref_harness.py).

    python tests/golden/make_golden_loss.py            writes the fixture
    python tests/golden/make_golden_loss.py --check    regenerates it in memory and compares it with the file

The reference's own network.RaysLTChromLoss runs in float32 on one small case (N = 2, R = 5, 7 x 9; fractional alpha with holes,
a photograph on both sides of the 1/20 clamp), with img and with img=None; recorded are the inputs, its four outputs, the
autograd gradient of its loss in rays_lt, and the parameter names of its forward (names only).  The crop / L1 lines of the
training script are not importable (they sit in the script's loop): torch.nn.L1Loss on `x[:, :, 5:-5, 5:-5] * alpha[:, :, 5:-5,
5:-5]`, as the script forms its arguments, runs on a 13 x 15 image pair of the same alpha recipe (7 x 9 leaves an empty crop),
with the loss and its gradient recorded.  Data only, about 50 KB.
"""
import inspect
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
OUT = os.path.join(HERE, 'chrom_loss.npz')


def generate():
    import ref_harness
    ref = ref_harness.import_reference()['network']
    crit = ref.RaysLTChromLoss()
    rng = np.random.default_rng(391)
    N, R, H, W = 2, 5, 7, 9
    rays = (0.2 + 1.8 * rng.random((N, R, 3, H, W))).astype(np.float32)
    alpha = (rng.random((N, 1, H, W)) * (rng.random((N, 1, H, W)) > 0.25)).astype(np.float32)
    img = (rng.random((N, 3, H, W)) * 0.06).astype(np.float32)
    data = {'rays_lt': rays, 'alpha': alpha, 'img': img,
            'forward_parameters': np.array(json.dumps(list(inspect.signature(ref.RaysLTChromLoss.forward).parameters)))}
    for tag, im in (('img', torch.from_numpy(img)), ('noimg', None)):
        x = torch.from_numpy(rays).clone().requires_grad_()
        loss, chrom, mean, diff = crit(x, torch.from_numpy(alpha), im)
        grad, = torch.autograd.grad(loss, x)
        data.update({'loss_' + tag: loss.detach().numpy(), 'chrom_' + tag: chrom.detach().numpy(),
                     'chrom_mean_' + tag: mean.detach().numpy(), 'chrom_diff_' + tag: diff.detach().numpy(),
                     'grad_' + tag: grad.numpy()})
    H1, W1 = 13, 15
    est = rng.random((N, 3, H1, W1)).astype(np.float32)
    gt = rng.random((N, 3, H1, W1)).astype(np.float32)
    alpha1 = (rng.random((N, 1, H1, W1)) * (rng.random((N, 1, H1, W1)) > 0.25)).astype(np.float32)
    e = torch.from_numpy(est).clone().requires_grad_()
    a_c = torch.from_numpy(alpha1)[:, :, 5:-5, 5:-5]
    l1 = torch.nn.L1Loss(reduction='mean')((e[:, :, 5:-5, 5:-5] * a_c).contiguous().view(-1).float(),
                                           (torch.from_numpy(gt)[:, :, 5:-5, 5:-5] * a_c).reshape(-1).float())
    g1, = torch.autograd.grad(l1, e)
    data.update({'l1_est': est, 'l1_gt': gt, 'l1_alpha': alpha1, 'l1_loss': l1.detach().numpy(), 'l1_grad': g1.numpy()})
    return data


def main(argv):
    data = generate()
    if '--check' in argv:
        have = np.load(OUT)
        bad = [k for k in data if k not in have.files or not np.array_equal(have[k], data[k])] + [k for k in have.files if k not in data]
        print('make_golden_loss --check: %s' % ('OK' if not bad else 'FAILED: %s' % bad))
        return 1 if bad else 0
    np.savez_compressed(OUT, **data)
    print('wrote %s (%d bytes)' % (OUT, os.path.getsize(OUT)))
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
