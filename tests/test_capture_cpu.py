"""CPU: the GPU-free half of training from a capture — rnr_amd.capture.crop_geometry against data_util.square_crop_img's slicing,
and dataio.ViewDataset(load_img=True, img_dir=...): its file list, names, sampling, read_camera against the reference's golden
cameras (tests/golden/dataio_views.npz, written by the reference's own ViewDataset), the odd-side crop, and what is refused."""
import os

import numpy as np
import pytest
import torch

PATTERNS = ['all', 'skip_3', 'first_5', 'after_6', 'skipinv_3', 'filter', 'only_2']
CAMERA_KEYS = ['proj_orig', 'proj', 'pose', 'dist_coeffs', 'offset', 'scale', 'view_dir', 'proj_inv', 'R_inv']


def _square_crop_indices(h, w):
    """data_util.square_crop_img (data_util.py:11-18) applied to an array that holds its own (row, column) indices."""
    img = np.stack(np.meshgrid(np.arange(h), np.arange(w), indexing='ij'), -1)
    min_dim = np.amin(img.shape[:2])
    center_coord = np.array(img.shape[:2]) // 2
    center_coord_new = np.array([min_dim // 2, min_dim // 2])
    img = img[center_coord[0] - min_dim // 2:center_coord[0] + min_dim // 2,
              center_coord[1] - min_dim // 2:center_coord[1] + min_dim // 2]
    return img, center_coord, center_coord_new


@pytest.mark.parametrize('hw', [(480, 640), (37, 53), (53, 37), (33, 33), (20, 31)])
def test_crop_geometry_is_square_crop_img(hw):
    from rnr_amd import capture
    h, w = hw
    win, cc, ccn = _square_crop_indices(h, w)
    center, center_new, y0, x0, side = capture.crop_geometry(h, w)
    assert tuple(center) == tuple(cc) and tuple(center_new) == tuple(ccn)
    assert win.shape == (side, side, 2)
    assert np.array_equal(win[..., 0], np.arange(y0, y0 + side)[:, None].repeat(side, 1))
    assert np.array_equal(win[..., 1], np.arange(x0, x0 + side)[None, :].repeat(side, 0))
    assert 0 <= y0 and y0 + side <= h and 0 <= x0 and x0 + side <= w
    if hw == (37, 53):
        assert (y0, x0, side) == (0, 8, 36)
    if hw == (53, 37):
        assert (y0, x0, side) == (8, 0, 36)


def _write_pngs(img_dir, n, h, w):
    from PIL import Image
    os.makedirs(img_dir, exist_ok=True)
    rng = np.random.RandomState(5)
    names = ['view_%03d.png' % (7 * i + 3) for i in range(n)]
    for fn in names:
        Image.fromarray(rng.randint(0, 256, (h, w, 3)).astype(np.uint8)).save(os.path.join(img_dir, fn))
    return names


@pytest.fixture(scope='module')
def capture_dir(tmp_path_factory):
    """calib.mat from the golden calibration and nine 480 x 640 PNGs (plus a dotfile, which glob would not list)."""
    import scipy.io
    root = tmp_path_factory.mktemp('capture')
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'dataio_views.npz'))
    calib_fp = str(root / 'calib.mat')
    scipy.io.savemat(calib_fp, {k[6:]: g[k] for k in g.files if k.startswith('calib:')})
    names = _write_pngs(str(root / 'rgb0'), 9, 480, 640)
    with open(str(root / 'rgb0' / '._x.png'), 'wb') as f:
        f.write(b'not an image')
    return str(root), calib_fp, str(root / 'rgb0'), names, g


def _dataset(root, calib_fp, img_dir, pattern, img_size=(64, 96), **kw):
    import dataio
    return dataio.ViewDataset(root_dir=root, calib_path=calib_fp, calib_format='convert', img_size=list(img_size),
                              sampling_pattern=pattern, load_img=True, img_dir=img_dir, load_precompute=False, **kw)


@pytest.mark.parametrize('pat', PATTERNS)
def test_read_camera_matches_reference(capture_dir, pat):
    """With an even shorter side the photograph's crop and the load_img=False crop agree, so the golden cameras apply."""
    root, calib_fp, img_dir, names, g = capture_dir
    ds = _dataset(root, calib_fp, img_dir, pat)
    assert len(ds) == int(g[pat + ':num'])
    for i in range(len(ds)):
        v, again = ds.read_camera(i), ds.read_camera(i)
        assert 'img_gt' not in v
        for key in CAMERA_KEYS:
            assert v[key].dtype == torch.float32 and not v[key].is_cuda
            assert np.allclose(v[key].numpy(), g[pat + ':' + key][i], rtol=1e-6, atol=1e-6), (pat, i, key)
            assert torch.equal(v[key], again[key]), (pat, i, key)           # pure: nothing compounds
        assert v['idx'] == i and v['img_fn'] == ds.img_idx2fn[i]


def test_file_names_are_real_and_sorted(capture_dir):
    root, calib_fp, img_dir, names, g = capture_dir
    ds = _dataset(root, calib_fp, img_dir, 'all')
    assert names == sorted(names)
    assert ds.img_fp_all == [os.path.join(img_dir, fn) for fn in names]         # the dotfile is not listed
    assert ds.img_idx2fn == names and ds.img_fn2idx == {fn: i for i, fn in enumerate(names)}
    ds = _dataset(root, calib_fp, img_dir, 'skip_3')
    assert ds.img_idx2fn == names[::3] and ds.img_fn2idx == {fn: i for i, fn in enumerate(names[::3])}
    keep = [int(i) for i in g['calib:keep_id'][0]]
    assert _dataset(root, calib_fp, img_dir, 'filter').img_idx2fn == [names[i] for i in keep]
    assert _dataset(root, calib_fp, img_dir, 'only_2').img_idx2fn == [names[2]]


def _one_photo_capture(tmp_path, g, n, h, w):
    import scipy.io
    calib_fp = str(tmp_path / 'calib.mat')
    scipy.io.savemat(calib_fp, {k[6:]: g[k] for k in g.files if k.startswith('calib:')})
    names = _write_pngs(str(tmp_path / 'rgb0'), n, h, w)
    return str(tmp_path), calib_fp, str(tmp_path / 'rgb0'), names


def test_odd_side_uses_the_photographs_own_crop(golden, tmp_path):
    """37 x 53: the window is 36 x 36 starting at column 8, so scale = 64 / 36 (not 64 / 37) and offset = (0, -8); fewer files than
    poses take the first poses."""
    g = golden('dataio_views')
    root, calib_fp, img_dir, names = _one_photo_capture(tmp_path, g, 2, 37, 53)
    ds = _dataset(root, calib_fp, img_dir, 'all', img_size=(64, 64))
    assert len(ds) == 2
    for i in range(2):
        v = ds.read_camera(i)
        assert np.array_equal(v['scale'].numpy(), np.array([64 / 36, 64 / 36], np.float32))
        assert np.array_equal(v['offset'].numpy(), np.array([0, -8], np.float32))
        pose = np.dot(g['calib:poses'][i], np.linalg.inv(g['calib:global_RT']))
        assert np.allclose(v['pose'].numpy(), pose, rtol=1e-6, atol=1e-6)
        p0 = g['calib:projs'][i]
        s = np.float32(64 / 36)
        assert np.allclose(v['proj'].numpy()[0, 0], p0[0, 0] * s, rtol=1e-6)
        assert np.allclose(v['proj'].numpy()[0, -1], (p0[0, -1] - 8) * s, rtol=1e-6, atol=1e-6)
        assert np.allclose(v['proj'].numpy()[1, -1], p0[1, -1] * s, rtol=1e-6, atol=1e-6)


def test_more_files_than_poses_is_refused(golden, tmp_path):
    g = golden('dataio_views')
    root, calib_fp, img_dir, names = _one_photo_capture(tmp_path, g, 10, 8, 8)
    with pytest.raises(ValueError, match=r'10\b.*\b9\b'):
        _dataset(root, calib_fp, img_dir, 'all')


def test_what_is_still_refused(capture_dir):
    import dataio
    root, calib_fp, img_dir, names, g = capture_dir
    with pytest.raises(NotImplementedError, match='view_maps'):
        dataio.ViewDataset(root, calib_fp, 'convert', [64, 64], 'all', load_img=False, load_precompute=True)
    with pytest.raises(NotImplementedError, match='view_maps'):
        dataio.ViewDataset(root, calib_fp, 'convert', [64, 64], 'all', load_img=True, img_dir=img_dir, load_precompute=True)
    with pytest.raises(NotImplementedError, match='image directory'):
        dataio.ViewDataset(root, calib_fp, 'convert', [64, 64], 'all', load_img=True)
    with pytest.raises(ValueError):
        dataio.ViewDataset(root, calib_fp, 'convert', [64, 64], 'all', load_img=True, img_dir=os.path.join(root, 'missing'))


def test_photograph_modes_and_formats(golden, tmp_path):
    """Grey photographs are a ValueError, 16-bit ones and .exr / .hdr / .mat (listed, in order) a NotImplementedError — raised
    before anything touches a GPU.  The camera of a refused mode still reads: it needs the header only."""
    from PIL import Image
    g = golden('dataio_views')
    root, calib_fp, img_dir, names = _one_photo_capture(tmp_path, g, 1, 8, 10)
    Image.fromarray(np.zeros((8, 10), np.uint8)).save(os.path.join(img_dir, 'w_grey.png'))
    Image.fromarray(np.zeros((8, 10), np.uint16)).save(os.path.join(img_dir, 'x_deep.png'))
    for fn in ('y_probe.hdr', 'z_img.mat'):
        with open(os.path.join(img_dir, fn), 'wb') as f:
            f.write(b'\0')
    ds = _dataset(root, calib_fp, img_dir, 'all', img_size=(4, 4))
    assert ds.img_idx2fn == names + ['w_grey.png', 'x_deep.png', 'y_probe.hdr', 'z_img.mat']
    assert tuple(ds.read_camera(1)['scale'].tolist()) == (0.5, 0.5)
    with pytest.raises(ValueError, match='w_grey.png'):
        ds.read_view(1)
    with pytest.raises(NotImplementedError, match='x_deep.png'):
        ds.read_view(2)
    for i in (3, 4):
        with pytest.raises(NotImplementedError, match=ds.img_idx2fn[i]):
            ds.read_view(i)
        with pytest.raises(NotImplementedError, match=ds.img_idx2fn[i]):
            ds.read_camera(i)


def test_read_view_without_a_gpu_fails_loudly(capture_dir):
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    root, calib_fp, img_dir, names, g = capture_dir
    ds = _dataset(root, calib_fp, img_dir, 'only_2')
    with pytest.raises(RuntimeError, match='GPU'):
        ds.read_view(0)
    with pytest.raises(RuntimeError, match='GPU'):
        ds[0]
