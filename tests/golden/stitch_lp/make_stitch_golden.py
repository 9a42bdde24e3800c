"""Generates tests/golden/stitch_lp/stitch_cases.npz from the READ-ONLY reference at /root/reference (build container only).

    python tests/golden/stitch_lp/make_stitch_golden.py            writes the fixture
    python tests/golden/stitch_lp/make_stitch_golden.py --check    regenerates it in memory and compares it with the file

The reference's own stitch_lp.py runs end to end under runpy, once per case.  What it cannot import here is stubbed: `cv2`
(imread delivers the case's synthetic photograph of the view, the fillPoly / resize / dilate chain its synthetic coverage, imwrite
captures the arrays), `trimesh` (a mesh without faces), `data_util` (cond_mkdir does nothing) and scipy.io.savemat (captured);
calib.mat is a real file in a temporary directory; np.int is shimmed (numpy >= 1.24) and no bytecode is written.  Stored per
case: the inputs (K, R, images, background masks, the views the sampling pattern uses), the arrays the script hands to imwrite
and savemat (lp, mask, count, num_view) and the case's minimum tie distance (tests/stitch_ref.py), which must be at least
1e-6: a condition on the inputs that keeps every texel index clear of a float64 rounding tie.  Nothing of the reference's text
is copied."""
import json
import os
import runpy
import sys
import tempfile
import types

import numpy as np
import scipy.io

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import stitch_ref as sr  # noqa: E402

REFERENCE = '/root/reference/stitch_lp.py'
OUT = os.path.join(HERE, 'stitch_cases.npz')


def ring(N, H, W, seed):
    return sr.random_cameras(np.random.RandomState(seed), N, H, W)


def fixed(eyes_targets_ups, H, W, focal):
    R = np.stack([sr.look_at(e, t, u) for e, t, u in eyes_targets_ups])
    return np.stack([sr.intrinsic(H, W, focal)] * len(R)), R


# name -> (views, H, W, lp_h, lp_w, sampling pattern, cameras)
CASES = {
    'ring4': (4, 24, 32, 64, 128, 'all', lambda: ring(4, 24, 32, 1)),
    'odd3': (3, 37, 53, 17, 31, 'all', lambda: ring(3, 37, 53, 2)),
    # looking along -x: atan2(z, x) jumps between +pi and -pi inside the image, u = 0 | 1
    'seam': (1, 24, 32, 64, 128, 'all', lambda: fixed([((3.0, 0.1, 0.0), (0.0, 0.13, 0.02), (0.05, 1.0, 0.0))], 24, 32, 0.6)),
    # looking along +y and -y: v = 0 and v = 1 inside the image, where the lp_h - 1 clamp fires
    'poles': (2, 24, 32, 64, 128, 'all', lambda: fixed([((0.02, -3.0, 0.0), (0.0, 0.0, 0.03), (0.0, 0.0, 1.0)),
                                                        ((0.0, 3.0, 0.05), (0.04, 0.0, 0.0), (1.0, 0.0, 0.1))], 24, 32, 0.5)),
    'skip5': (5, 24, 32, 64, 128, 'skip_2', lambda: ring(5, 24, 32, 3)),
}


def case_inputs(name):
    N, H, W, lp_h, lp_w, pattern, cams = CASES[name]
    K, R = cams()
    rng = np.random.RandomState(sum(map(ord, name)))
    images = (rng.randint(0, 1024, (N, H, W, 3)) / 256.0).astype(np.float32)
    yy, xx = np.mgrid[0:H, 0:W]
    masks = np.stack([((yy - rng.uniform(0.3, 0.7) * H) ** 2 + (xx - rng.uniform(0.3, 0.7) * W) ** 2 > (0.3 * H) ** 2)
                      & (rng.rand(H, W) < 0.9) for _ in range(N)])
    if name == 'poles':                     # the poles lie at the image centres: stitch the inside of the discs there
        masks = ~masks
    return N, H, W, lp_h, lp_w, pattern, K, R, images, masks


def run_reference(N, H, W, lp_h, lp_w, pattern, K, R, images, masks):
    """-> dict(lp, mask, count, num_view): what the script hands to imwrite('<idx>.exr'), imwrite('mask/<idx>.png') and savemat."""
    captured, state = {}, {'view': None}
    cv2 = types.ModuleType('cv2')
    cv2.IMREAD_ANYCOLOR, cv2.IMREAD_ANYDEPTH, cv2.IMREAD_UNCHANGED = 4, 2, -1

    def imread(path, flags=None):
        state['view'] = int(os.path.splitext(os.path.basename(path))[0])
        return images[state['view']].copy()

    def resize(img, size, **kw):            # (512, 512): the empty drawing passes through; (w, h): the view's coverage
        return img if tuple(size) == (512, 512) else np.where(masks[state['view']], 0.0, 255.0)

    def imwrite(path, arr):
        captured[os.path.relpath(path, tmp)] = np.array(arr)
        return True
    cv2.imread, cv2.resize, cv2.imwrite = imread, resize, imwrite
    cv2.dilate = lambda img, kernel: img
    cv2.fillPoly = lambda mask, pts, colour: mask
    trimesh = types.ModuleType('trimesh')
    trimesh.load = lambda fp, process=False: types.SimpleNamespace(vertices=np.array([[0.1, 0.0, 0.0], [0.0, 0.1, 0.0], [0.0, 0.0, 0.1]]),
                                                                   faces=np.zeros((0, 3), np.int64))
    data_util = types.ModuleType('data_util')
    data_util.cond_mkdir = lambda d: None
    poses = np.tile(np.eye(4), (N, 1, 1))
    poses[:, :3, :3] = R
    poses[:, 2, 3] = 3.0
    saved = {}
    for k in ('cv2', 'trimesh', 'data_util'):
        saved[k] = sys.modules.get(k)
    real_savemat, argv, had_int = scipy.io.savemat, sys.argv, hasattr(np, 'int')
    with tempfile.TemporaryDirectory() as tmp:
        real_savemat(os.path.join(tmp, 'calib.mat'), {'poses': poses, 'projs': K, 'img_hws': np.tile(np.array([[H, W]]), (N, 1)),
                                                      'global_RT': np.eye(4)})
        sys.modules.update({'cv2': cv2, 'trimesh': trimesh, 'data_util': data_util})
        scipy.io.savemat = lambda path, d: captured.__setitem__(os.path.relpath(path, tmp), d)
        sys.argv = [REFERENCE, '--data_root', tmp, '--sampling_pattern', pattern, '--lp_h', str(lp_h), '--lp_w', str(lp_w)]
        sys.dont_write_bytecode = True
        if not had_int:
            np.int = int  # noqa: NPY001 - the reference uses the removed alias
        try:
            runpy.run_path(REFERENCE, run_name='__main__')
        finally:
            scipy.io.savemat, sys.argv = real_savemat, argv
            if not had_int:
                del np.int
            for k, v in saved.items():
                if v is None:
                    sys.modules.pop(k, None)
                else:
                    sys.modules[k] = v
    d = 'light_probe_stitch_' + pattern
    mat = captured[os.path.join(d, 'count', '0.mat')]
    lp = captured[os.path.join(d, '0.exr')]
    assert lp.dtype == np.float32 and lp.shape == (lp_h, lp_w, 3)
    return {'lp': lp, 'mask': captured[os.path.join(d, 'mask', '0.png')] != 0, 'count': np.asarray(mat['count']).astype(np.int32),
            'num_view': np.int32(mat['num_view'])}


def used_views(N, pattern):
    return [i for i in range(N) if pattern == 'all' or i % int(pattern.split('_')[-1]) == 0]


def generate():
    data = {'names': np.array(json.dumps(list(CASES)))}
    for name in CASES:
        N, H, W, lp_h, lp_w, pattern, K, R, images, masks = case_inputs(name)
        out = run_reference(N, H, W, lp_h, lp_w, pattern, K, R, images, masks)
        used = used_views(N, pattern)
        tie = sr.stitch(images[used], masks[used], np.linalg.inv(K)[used], np.linalg.inv(R)[used], lp_h, lp_w)['tie']
        assert tie >= sr.TIE_MARGIN, '%s: tie distance %.3g below %.0e: choose other inputs' % (name, tie, sr.TIE_MARGIN)
        assert out['mask'].any() and int(out['count'].max()) <= len(used)
        for k, v in (('K', K), ('R', R), ('images', images), ('masks', masks.astype(np.uint8)), ('used', np.array(used, np.int32)),
                     ('lp_hw', np.array([lp_h, lp_w], np.int32)), ('tie', np.float64(tie))) + tuple(out.items()):
            data['%s_%s' % (name, k)] = v
    return data


def main(argv):
    data = generate()
    if '--check' in argv:
        have = np.load(OUT)
        bad = [k for k in data if k not in have.files or not np.array_equal(have[k], data[k])] + [k for k in have.files if k not in data]
        print('make_stitch_golden --check: %s' % ('OK' if not bad else 'FAILED: %s' % bad))
        return 1 if bad else 0
    np.savez_compressed(OUT, **data)
    print('wrote %s (%d bytes)' % (OUT, os.path.getsize(OUT)))
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
