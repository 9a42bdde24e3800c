"""CPU: the yardstick of the image-metric tests (tests/metric_ref.py) against the reference's own float32 results
(tests/golden/metric/metric_cases.npz, written by make_metric_golden.py from metric.compute_err_metrics_batch with
compute_ssim=False), the identities the kernel relies on, and the drop-in's signatures.

Tolerances of the yardstick-vs-fixture test: 4 x the largest deviation of the float64 yardstick from the reference's float32
results over the fixture's four views, measured when the fixture was written (the deviation is the reference's own float32
rounding — its differences, squares and `a / 255 - b / 255` are float32 — seen on one draw, hence the factor 4):
    key          measured (relative)   bound
    mae*         1.61e-9               6.5e-9
    mse*         5.11e-9               2.1e-8
    key          measured (dB)         bound
    psnr*        6.63e-6               2.7e-5
"""
import inspect
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metric_ref as mr  # noqa: E402

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'metric', 'metric_cases.npz')
MAE_RTOL, MSE_RTOL, PSNR_ATOL = 6.5e-9, 2.1e-8, 2.7e-5


def test_yardstick_matches_the_reference_run():
    d = np.load(FIXTURE)
    assert tuple(json.loads(str(d['keys']))) == mr.KEYS[:9]
    est, gt, mask = d['est'], d['gt'], d['mask']
    assert est.shape == (4, 3, 23, 19) and mask.shape == (4, 23, 19) and os.path.getsize(FIXTURE) < 64 * 1024
    out, _ = mr.batch(est, gt, mask, compute_ssim=False)
    ref = d['reference_out']
    for i, k in enumerate(mr.KEYS[:9]):
        err = np.abs(out[:, i] - ref[:, i])
        if i < 6:
            err, tol = err / np.abs(ref[:, i]), (MAE_RTOL if i < 3 else MSE_RTOL)
        else:
            tol = PSNR_ATOL
        print('%-10s max deviation %.3g (bound %.3g)' % (k, err.max(), tol))
        assert (err <= tol).all(), (k, err.max(), tol)
    assert np.isnan(out[:, 9:]).all()


def test_box_ssim_is_a_mean_over_a_part_of_the_images_map():
    """A valid convolution over a crop consists of exactly those windows of the full image that lie wholly inside the crop: the
    crop's map and the sub-map of the image's map are the same numbers (75 x 53, ragged mask)."""
    est, gt = mr.noise_images(1, 75, 53, 30)
    mask = mr.blob_mask(75, 53, 31) == 1
    x, y = mr.scaled(est[0], 1).transpose(1, 2, 0), mr.scaled(gt[0], 1).transpose(1, 2, 0)
    x[~mask], y[~mask] = 0, 0
    ys, xs = mask.nonzero()
    y0, y1, x0, x1 = ys.min(), ys.max() + 1, xs.min(), xs.max() + 1
    assert y1 - y0 >= 11 and x1 - x0 >= 11 and (y1 - y0, x1 - x0) != (75, 53)
    full = mr.ssim_map(x, y)
    crop = mr.ssim_map(x[y0:y1, x0:x1], y[y0:y1, x0:x1])
    sub = full[y0:y1 - 10, x0:x1 - 10]
    assert crop.shape == sub.shape
    print('crop map vs sub-map: max difference %.3g' % np.abs(crop - sub).max())
    assert np.array_equal(crop, sub)


def test_filter_order_changes_the_map_by_rounding_only():
    """The map with the passes in either order, on the cancellation-prone bright images: the order sensitivity that the GPU
    tests' SSIM bound (1e-9) leaves room for."""
    est, gt = mr.bright_images(1, 64, 64, 32)
    x, y = mr.scaled(est[0], 1).transpose(1, 2, 0), mr.scaled(gt[0], 1).transpose(1, 2, 0)
    d = np.abs(mr.ssim_map(x, y, True) - mr.ssim_map(x, y, False)).max()
    print('filter order: max map difference %.3g' % d)
    assert d < 1e-11


@pytest.mark.parametrize('name', ['four_masks', 'four_masks_bright', 'boxes', 'tiles', 'disc128'])
def test_ssim_valid_equals_ssim_bb(name):
    """metric.py:79-82 copies ground truth over estimate pixels outside the mask; both images are 0 there already, so the third
    SSIM evaluation (done literally by the yardstick) sees the second one's arrays."""
    ref = mr.case(name)['ref']
    assert np.array_equal(ref[:, 10], ref[:, 11], equal_nan=True)
    assert not np.isnan(ref[:, 10]).all()


def test_yardstick_edge_cases():
    ref, box = mr.case('four_masks')['ref'], mr.case('four_masks')['box']
    assert np.isfinite(ref[0]).all() and np.isfinite(ref[1]).all()
    assert np.isfinite(ref[2, :10]).all() and np.isnan(ref[2, 10:]).all() and box[2, 4] == 1         # single pixel
    assert np.isnan(ref[3, [1, 2, 4, 5, 7, 8, 10, 11]]).all() and (box[3] == 0).all()                  # empty mask
    assert ref[3, 0] == 0 and ref[3, 3] == 0 and ref[3, 6] == 100 and abs(ref[3, 9] - 1) < 1e-12
    assert box[1, 0] == 0 and box[1, 2] == 0 and box[1, 1] < 29 and box[1, 3] < 37                     # blob: two borders
    b = mr.case('boxes')['box']
    assert [(r[1] - r[0], r[3] - r[2]) for r in b] == [(11, 11), (12, 11), (40, 10)]
    assert np.isnan(mr.case('boxes')['ref'][2, 10]) and np.isfinite(mr.case('boxes')['ref'][:2, 10]).all()
    for n in ('10x13', '13x10'):
        r = mr.case(n)['ref']
        assert np.isnan(r[:, 9:]).all() and np.isfinite(r[:, :9]).all()


@pytest.mark.parametrize('name', sorted(mr.SECOND_PASS))
def test_second_pass_cases_sit_on_their_thresholds(name):
    """rnr_image_metrics_workspace_bytes(N, H, W) / N is 40 x bands + 16 x tiles: each second-pass case has the record counts
    it is named for, and the data that decides its result lies where only the later pass reads it."""
    from rnr_amd import _lib
    L = _lib.load()
    H, W, bands, tiles = mr.SECOND_PASS[name]
    c = mr.case(name)
    N = c['est'].shape[0]
    assert c['est'].shape == (N, 3, H, W) and c['mask'].shape == (N, H, W) and N == 2
    per_view = L.rnr_image_metrics_workspace_bytes(N, H, W) // N
    assert L.rnr_image_metrics_workspace_bytes(N, H, W) % N == 0 and per_view == mr.BAND_BYTES * bands + mr.TILE_BYTES * tiles
    band_rows = max(8, -(-H // 256))
    assert -(-H // band_rows) == bands
    assert tiles == -(-(H - 10) // 32) * -(-(W - 10) // 32)
    ref, box = c['ref'], c['box']
    if name == 'wide300':
        assert W > 256 and box[0].tolist() == [260, 300, 0, 13, 13 * 40]             # view 0: the second x pass alone
        assert box[1, 0] < 256 < box[1, 1] and np.isfinite(ref).all()
    elif name == 'bands256':
        assert bands == 256 and band_rows == 8 and box[1, 2:4].tolist() == [2040, 2048]  # view 1: the 256th band alone
        assert np.isnan(ref[1, 10:]).all() and np.isfinite(ref[1, :10]).all() and np.isfinite(ref[0]).all()
    elif name == 'bands9':
        assert band_rows == 9 and H - (bands - 1) * band_rows == 6                   # the last band is short
        assert box[0].tolist() == [0, 12, 2040, 2049, 9 * 12]                        # a box 9 high: no window
        assert np.isnan(ref[0, 10:]).all() and np.isfinite(ref[0, :10]).all() and np.isfinite(ref[1]).all()
        assert box[1].tolist() == [0, 12, 0, 2049, 2049 * 12]
    else:
        assert tiles == 257 and band_rows == 33 and (H - 10) - 256 * 32 == 1         # the 257th tile: one row of windows
        assert box[1, 2:4].tolist() == [8100, 8203] and box[1, 2] // 32 == 253        # in-box windows: tiles 253..256 alone
        assert np.isfinite(ref).all()


def test_dropin_signatures_equal_the_references():
    """Parameter names, order and defaults of psnr, compute_err_metrics, compute_err_metrics_batch as recorded from the reference."""
    import metric
    d = np.load(FIXTURE)
    names, defaults = json.loads(str(d['parameters'])), json.loads(str(d['defaults']))
    assert set(names) == {'psnr', 'compute_err_metrics', 'compute_err_metrics_batch'}
    for f, want in names.items():
        sig = inspect.signature(getattr(metric, f))
        assert list(sig.parameters) == want, f
        assert [repr(p.default) for p in sig.parameters.values() if p.default is not p.empty] == defaults[f], f


def test_dropin_raises_without_a_gpu():
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    import metric
    c = mr.case('one_window')
    with pytest.raises(RuntimeError):
        metric.compute_err_metrics_batch(torch.from_numpy(c['est']), torch.from_numpy(c['gt']), torch.from_numpy(c['mask'])[:, None])
    with pytest.raises(RuntimeError):
        metric.compute_err_metrics(c['est'][0].transpose(1, 2, 0), c['gt'][0].transpose(1, 2, 0), c['mask'][0])
    with pytest.raises(RuntimeError):
        metric.psnr(c['est'][0].transpose(1, 2, 0), c['gt'][0].transpose(1, 2, 0))


def test_keys_are_the_abi_order():
    """rnr_amd.metrics.KEYS and the yardstick's KEYS follow the RNR_METRIC_* enum of include/rnr_hip.h."""
    import re
    from rnr_amd import metrics
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'rnr_hip.h')).read()
    enum = re.search(r'enum \{ (RNR_METRIC_MAE = 0,.*?)\};', hdr, flags=re.S).group(1)
    order = tuple(s.strip().split(' ')[0][len('RNR_METRIC_'):].lower() for s in enum.split(','))
    assert order == metrics.KEYS == mr.KEYS
