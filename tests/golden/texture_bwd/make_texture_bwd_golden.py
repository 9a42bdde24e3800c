"""Generates tests/golden/texture_bwd/texture_bwd_cases.npz from the READ-ONLY reference at /root/reference (build container only).

    python tests/golden/texture_bwd/make_texture_bwd_golden.py            writes the fixture
    python tests/golden/texture_bwd/make_texture_bwd_golden.py --check    regenerates it in memory and compares it with the file

The reference's network.TextureMapper(32, 16, 4, apply_sh=True) is imported at run time through tests/golden/ref_harness.py, run
forward on the CPU on the seam scene of tests/texture_bwd_ref.py (2 views of 20 x 24, sh_start_ch 6) and differentiated with
`out.backward(grad_out)`.  Stored: the inputs (uv_map, sh_basis_map, grad_out) and the reference's own float32 gradient of each of
the four levels: data only, about 140 KB.  Nothing of the reference's text is copied.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(os.path.dirname(HERE))
for p in (TESTS, os.path.dirname(HERE), os.path.dirname(TESTS)):
    if p not in sys.path:
        sys.path.insert(0, p)
import texture_bwd_ref as tb  # noqa: E402

OUT = os.path.join(HERE, 'texture_bwd_cases.npz')
S, C, LEVELS, SH_START, SEED = 32, 16, 4, 6, 12


def generate():
    import ref_harness
    ref = ref_harness.import_reference()
    uv, sh, g = tb.seam_scene(SEED, 2, 20, 24, C)
    tm = ref['network'].TextureMapper(S, C, LEVELS, apply_sh=True)
    out = tm(uv.clone(), sh.clone(), sh_start_ch=SH_START)
    out.backward(g)
    data = {'uv': uv.numpy(), 'sh': sh.numpy(), 'grad_out': g.numpy(), 'sh_start_ch': np.array(SH_START),
            'sizes': np.array([int(s) for s in tm.textures_size])}
    for l, p in enumerate(tm.textures):
        assert p.grad is not None and p.grad.dtype == torch.float32
        data['grad%d' % l] = p.grad[0].numpy()
    assert list(data['sizes']) == tb.level_sizes(S, LEVELS)
    return data


def main(argv):
    data = generate()
    if '--check' in argv:
        have = np.load(OUT)
        bad = [k for k in data if k not in have.files or not np.array_equal(have[k], data[k])] + [k for k in have.files if k not in data]
        print('make_texture_bwd_golden --check: %s' % ('OK' if not bad else 'FAILED: %s' % bad))
        return 1 if bad else 0
    np.savez_compressed(OUT, **data)
    print('wrote %s (%d bytes)' % (OUT, os.path.getsize(OUT)))
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
