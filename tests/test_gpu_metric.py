"""-m gpu: rnr_image_metrics (MAE / MSE / PSNR over image, box and mask, SSIM over image and box, per view) against the float64
yardstick of tests/metric_ref.py, which restates metric.compute_err_metrics step by step, and the layers above it
(ops.image_metrics, rnr_amd.metrics, the drop-in metric module, LightTransport.score).

Bounds (metric_ref.SUM_RTOL, PSNR_ATOL, SSIM_ATOL), derived, both sides float64:
    sum-derived outputs  1e-10 relative: n 2^-53 for n = 3 x 512^2 terms in any summation order
    PSNR                 1e-9 dB: 10 / ln 10 = 4.34 x the sum bound
    SSIM                 1e-9 absolute: per window 2^-53 x ~100 operations x 65025 / C2 = 1100 -> 1e-11, filter-order sensitivity
                         ~1e-12 (test_metric_ref_cpu.py), and the mean over at most 2.5e5 windows adds n 2^-53
    box                  exact
A wrong tap, weight, window range or divisor shows at 1e-5 or more.

Sizes are the smallest at which each piece can go wrong (metric_ref.case): one window; no window; 37 x 29 with a full, a ragged,
a one-pixel and an empty mask; boxes of 11 x 11, 11 x 12, 10 x 40; 75 x 53 and 53 x 85 (two full 32-window tiles and a
remainder on either axis); 128 x 128 with a disc; and the smallest sizes at which a second-level loop of the kernels runs a
second pass, masked so that the later pass decides the result: 13 x 300 (sums_kernel's x loop, W > 256), 2048 x 12 and
2049 x 12 (256 bands of 8 rows; band_rows 9 with a short last band), 8203 x 13 (257 tiles per view, band_rows 33: the tile
loop of finalise_kernel).  The largest of them has 3 x 8203 x 13 = 3.2e5 terms and 2.5e4 windows per view, below the
3 x 512^2 terms and 2.5e5 windows the bounds above are derived for.  Every comparison prints its figures before it asserts."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metric_ref as mr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def T(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x))


def _run(est, gt, mask, channels_last=False, **kw):
    """ops.image_metrics on host arrays [N,3,H,W] -> (out [N,12], box [N,5]) numpy."""
    from rnr_amd import ops
    e, g = T(est).to(DEV), T(gt).to(DEV)
    if channels_last:
        e, g = e.permute(0, 2, 3, 1).contiguous(), g.permute(0, 2, 3, 1).contiguous()
    m = None if mask is None else T(mask).to(DEV)
    out, box = ops.image_metrics(e, g, m, channels_last=channels_last, return_box=True, **kw)
    assert out.dtype == torch.float64 and out.is_cuda and box.dtype == torch.int32
    return out.cpu().numpy(), box.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


# ------------------------------------------------------------------------------------------------
# 1. every case, both layouts, against the yardstick
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('channels_last', [False, True], ids=['planar', 'channels_last'])
@pytest.mark.parametrize('name', mr.CASES)
def test_against_the_float64_yardstick(name, channels_last):
    c = mr.case(name)
    out, box = _run(c['est'], c['gt'], c['mask'], channels_last)
    mr.compare(out, box, c['ref'], c['box'], '%s %s' % (name, 'channels-last' if channels_last else 'planar'))


def test_identical_images():
    """est == gt: every error 0, every PSNR 100, every SSIM within the bound of 1 (NaN where the yardstick has NaN)."""
    c = mr.case('four_masks_bright')
    ref, ref_box = mr.batch(c['est'], c['est'], c['mask'])
    out, box = _run(c['est'], c['est'].copy(), c['mask'])
    mr.compare(out, box, ref, ref_box, 'identical')
    fin = ~np.isnan(ref)
    assert (out[:, :6][fin[:, :6]] == 0).all() and (out[:, 6:9][fin[:, 6:9]] == 100).all()
    assert (np.abs(out[:, 9:][fin[:, 9:]] - 1) <= mr.SSIM_ATOL).all() and fin[0].all()


# ------------------------------------------------------------------------------------------------
# 2. mask semantics
# ------------------------------------------------------------------------------------------------
def test_only_mask_equal_one_is_valid():
    """0.5, NaN, 2, -1 and 0.999 in the mask count as not valid: the same bits as with 0 there."""
    c = mr.case('four_masks')
    base, base_box = _run(c['est'], c['gt'], c['mask'])
    m = c['mask'].copy()
    other = np.resize(np.array([0.5, np.nan, 2.0, -1.0, np.float32(1) - np.float32(2 ** -24), np.inf], np.float32), m.shape)
    m[m != 1] = other[m != 1]
    out, box = _run(c['est'], c['gt'], m)
    assert np.array_equal(_bits(out), _bits(base)) and np.array_equal(box, base_box)


def test_values_outside_the_mask_never_enter():
    """NaN and infinities outside the mask give the same bits as zeros there (the mask is a select, not a product)."""
    c = mr.case('tiles')
    base, base_box = _run(c['est'], c['gt'], c['mask'])
    est, gt = c['est'].copy(), c['gt'].copy()
    outside = np.broadcast_to((c['mask'] != 1)[:, None], est.shape)
    junk = np.resize(np.array([np.nan, np.inf, -np.inf, 3e38], np.float32), est.shape)
    est[outside] = junk[outside]
    gt[outside] = np.roll(junk, 1)[outside]
    assert np.isnan(est).any() and outside.any()
    for cl in (False, True):
        out, box = _run(est, gt, c['mask'], cl)
        ref, _ = _run(c['est'], c['gt'], c['mask'], cl)
        assert np.isfinite(out).all()
        assert np.array_equal(_bits(out), _bits(ref)) and np.array_equal(box, base_box)
    assert np.isfinite(base).all()


def test_nan_inside_a_mask_stays_in_its_view():
    c = mr.case('boxes')                      # three views
    base, base_box = _run(c['est'], c['gt'], c['mask'])
    est = c['est'].copy()
    y, x = np.argwhere(c['mask'][1] == 1)[7]
    est[1, 2, y, x] = np.nan
    out, box = _run(est, c['gt'], c['mask'])
    assert np.isnan(out[1]).all()
    assert np.array_equal(_bits(out[[0, 2]]), _bits(base[[0, 2]])) and np.array_equal(box, base_box)
    assert np.isfinite(out[0]).all() and np.isfinite(out[2, :10]).all()


# ------------------------------------------------------------------------------------------------
# 3. scale, compute_ssim, determinism, inputs untouched
# ------------------------------------------------------------------------------------------------
def test_scale_is_one_float32_product():
    """scale=255 on [0,1] inputs == scale=1 on the float32-premultiplied inputs, bit for bit; and against the yardstick."""
    rng = np.random.default_rng(40)
    est, gt = rng.random((2, 3, 37, 29), dtype=np.float32), rng.random((2, 3, 37, 29), dtype=np.float32)
    mask = mr.four_masks(37, 29)[:2]
    a, abox = _run(est, gt, mask, scale=255.0)
    b, bbox = _run(est * np.float32(255), gt * np.float32(255), mask, scale=1.0)
    assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(abox, bbox)
    ref, ref_box = mr.batch(est, gt, mask, scale=255.0)
    mr.compare(a, abox, ref, ref_box, 'scale 255')


def test_compute_ssim_false():
    c = mr.case('tiles')
    full, _ = _run(c['est'], c['gt'], c['mask'])
    out, box = _run(c['est'], c['gt'], c['mask'], compute_ssim=False)
    assert np.isnan(out[:, 9:]).all() and np.array_equal(_bits(out[:, :9]), _bits(full[:, :9]))
    assert np.array_equal(box, c['box']) and np.isfinite(full).all()


@pytest.mark.parametrize('name', ['disc128', 'tiles257'])
def test_two_calls_same_bits_and_inputs_untouched(name):
    from rnr_amd import ops
    c = mr.case(name)
    e, g, m = T(c['est']).to(DEV), T(c['gt']).to(DEV), T(c['mask']).to(DEV)
    a = ops.image_metrics(e, g, m).clone()
    b = ops.image_metrics(e, g, m)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    for dev_t, host in ((e, c['est']), (g, c['gt']), (m, c['mask'])):
        assert np.array_equal(_bits(dev_t.cpu().numpy()), _bits(host))
    given = torch.full((2, 12), -7.0, dtype=torch.float64, device=DEV)
    assert ops.image_metrics(e, g, m, out=given) is given and torch.equal(given.view(torch.int64), a.view(torch.int64))


# ------------------------------------------------------------------------------------------------
# 4. guard bands
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,channels_last', [('tiles', False), ('tiles', True), ('tiles257', False), ('tiles257', True)],
                         ids=['planar', 'channels_last', 'tiles257-planar', 'tiles257-channels_last'])
def test_guard_bands(name, channels_last):
    """est, gt and mask carved out of NaN-filled buffers, out, box and the workspace out of sentinel-filled ones, through the C
    ABI: the results are the plain call's (no NaN picked up), nothing outside out, box and the workspace is written.  At
    8203 x 13 the Tile records start 2 x 249 x 40 bytes into the workspace and there are 257 of them per view."""
    from rnr_amd import _lib
    L = _lib.load()
    c = mr.case(name)
    N, _, H, W = c['est'].shape
    G = 64                                                   # guard elements on either side
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def carve_in(a):
        buf = torch.full((a.size + 2 * G,), float('nan'), dtype=torch.float32, device=DEV)
        buf[G:G + a.size] = T(a).reshape(-1).to(DEV)
        return buf, buf[G:G + a.size]
    lay = (lambda a: a.transpose(0, 2, 3, 1)) if channels_last else (lambda a: a)
    (be, e), (bg, g), (bm, m) = carve_in(lay(c['est'])), carve_in(lay(c['gt'])), carve_in(c['mask'])
    wsb = L.rnr_image_metrics_workspace_bytes(N, H, W)
    assert wsb % 8 == 0 and wsb > 0
    out_buf = torch.full((N * 12 + 2 * G,), -12345.0, dtype=torch.float64, device=DEV)
    box_buf = torch.full((N * 5 + 2 * G,), -777, dtype=torch.int32, device=DEV)
    ws_buf = torch.full((wsb + 2 * G * 8,), 0x5A, dtype=torch.uint8, device=DEV)
    out, box, ws = out_buf[G:G + N * 12], box_buf[G:G + N * 5], ws_buf[G * 8:G * 8 + wsb]
    _lib.check(L.rnr_image_metrics(p(e), p(g), p(m), 1 if channels_last else 0, 1.0, 1, p(out), p(box), p(ws), N, H, W,
                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    mr.compare(out.cpu().numpy().reshape(N, 12), box.cpu().numpy().reshape(N, 5), c['ref'], c['box'], 'guarded %s' % name)
    plain, _ = _run(c['est'], c['gt'], c['mask'], channels_last)
    assert np.array_equal(_bits(out.cpu().numpy().reshape(N, 12)), _bits(plain))
    assert (out_buf[:G] == -12345.0).all() and (out_buf[G + N * 12:] == -12345.0).all()
    assert (box_buf[:G] == -777).all() and (box_buf[G + N * 5:] == -777).all()
    assert (ws_buf[:G * 8] == 0x5A).all() and (ws_buf[G * 8 + wsb:] == 0x5A).all()
    for buf, n in ((be, e.numel()), (bg, g.numel()), (bm, m.numel())):
        assert torch.isnan(buf[:G]).all() and torch.isnan(buf[G + n:]).all()


# ------------------------------------------------------------------------------------------------
# 5. errors
# ------------------------------------------------------------------------------------------------
def test_errors():
    from rnr_amd import _lib, ops
    L = _lib.load()
    e = torch.zeros(1, 3, 12, 12, device=DEV)
    with pytest.raises(RuntimeError):
        ops.image_metrics(e.cpu(), e.cpu())
    with pytest.raises(ValueError):
        ops.image_metrics(e, torch.zeros(1, 3, 12, 13, device=DEV))
    with pytest.raises(ValueError):
        ops.image_metrics(e, e, torch.zeros(1, 1, 12, 12, device=DEV))
    with pytest.raises(ValueError):
        ops.image_metrics(e, e, channels_last=True)
    with pytest.raises(ValueError):
        ops.image_metrics(e, e, out=torch.zeros(2, 12, dtype=torch.float64, device=DEV))
    p = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)
    out = torch.zeros(12, dtype=torch.float64, device=DEV)
    ws = torch.zeros(L.rnr_image_metrics_workspace_bytes(1, 12, 12), dtype=torch.uint8, device=DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    bad = [(None, e, out, ws, 0, 1, 12, 12), (e, None, out, ws, 0, 1, 12, 12), (e, e, None, ws, 0, 1, 12, 12), (e, e, out, None, 0, 1, 12, 12),
           (e, e, out, ws, 2, 1, 12, 12), (e, e, out, ws, 0, 0, 12, 12), (e, e, out, ws, 0, 1, 0, 12), (e, e, out, ws, 0, 1, 12, -1),
           (e, e, out, ws, 0, 2, 18919, 18919)]                                 # 2 x 3 x 18919^2 = 2^31 + 1.9e5
    for a, b, o, w, layout, n, h, wd in bad:
        assert L.rnr_image_metrics(p(a), p(b), None, layout, 1.0, 1, p(o), None, p(w), n, h, wd, st) != 0
        assert L.rnr_last_error()
    torch.cuda.synchronize()
    assert (out == 0).all()
    assert L.rnr_image_metrics_workspace_bytes(0, 12, 12) == 0


# ------------------------------------------------------------------------------------------------
# 6. the layers above
# ------------------------------------------------------------------------------------------------
def test_dropin_returns_the_ops_numbers():
    """metric.compute_err_metrics_batch / compute_err_metrics / psnr: the reference's dict shape, the op's numbers, arguments
    left as they were (numpy, CPU tensors and device tensors alike), ValueError naming the view with an empty mask."""
    import metric
    c = mr.case('four_masks')
    est, gt, mask = c['est'][:3], c['gt'][:3], c['mask'][:3]
    want, _ = _run(est, gt, mask)
    te, tg, tm = T(est.copy()), T(gt.copy()), T(mask.copy())[:, None]
    for dev in ('cpu', DEV):
        a, b, m = te.to(dev), tg.to(dev), tm.to(dev)
        res = metric.compute_err_metrics_batch(a, b, m)
        assert list(res) == list(mr.KEYS) + [k + '_mean' for k in mr.KEYS]
        for i, k in enumerate(mr.KEYS):
            assert res[k].shape == (3, 1) and res[k].dtype == np.float64
            assert np.array_equal(_bits(res[k][:, 0]), _bits(want[:, i]))
            assert np.array_equal(res[k + '_mean'], want[:, i].mean(), equal_nan=True)
        assert torch.equal(a.cpu(), T(est)) and torch.equal(b.cpu(), T(gt)) and torch.equal(m.cpu(), T(mask)[:, None])
    res = metric.compute_err_metrics_batch(te, tg, tm, compute_ssim=False)
    for i, k in enumerate(mr.KEYS):
        if i < 9:
            assert np.array_equal(_bits(res[k][:, 0]), _bits(want[:, i]))
        else:
            assert res[k] == [] and np.isnan(res[k + '_mean'])
    with pytest.raises(ValueError, match='view 3'):
        metric.compute_err_metrics_batch(T(c['est']), T(c['gt']), T(c['mask'])[:, None])
    # one view, channel-last numpy arrays, as compute_err_metrics takes them
    e1, g1 = np.ascontiguousarray(est[1].transpose(1, 2, 0)), np.ascontiguousarray(gt[1].transpose(1, 2, 0))
    keep = e1.copy()
    one = metric.compute_err_metrics(e1, g1, mask[1])
    assert list(one) == list(mr.KEYS) and np.array_equal(e1, keep)
    mr.compare(np.array([[one[k] for k in mr.KEYS]]), None, c['ref'][1:2], None, 'compute_err_metrics')
    assert list(metric.compute_err_metrics(e1, g1, mask[1], compute_ssim=False)) == list(mr.KEYS[:9])
    assert abs(metric.psnr(e1, g1) - mr.psnr(e1.astype(np.float64), g1.astype(np.float64))) <= mr.PSNR_ATOL
    m3 = mask[1][:, :, None].repeat(3, axis=2)
    assert abs(metric.psnr(e1, g1, m3) - c['ref'][1, 8]) <= mr.PSNR_ATOL
    assert metric.psnr(e1, e1.copy()) == 100


@pytest.mark.parametrize('size', [(9, 11), (13, 15)], ids=['9x11', '13x15'])
def test_light_transport_score(size):
    """LightTransport.score on the lighting tests' smallest scene (2 views, 13 + 13 rays, a 16 x 32 probe; 9 x 11 has no SSIM
    window, 13 x 15 has): the numbers of ops.image_metrics on the rendered frames with mask = alpha and scale 255, and of the
    yardstick on those frames; score_frames' dict."""
    from rnr_amd import metrics, ops
    from rnr_amd.pipeline import LightTransport
    rng = np.random.default_rng(7)
    N, (H, W), ns, nd = 2, size, 13, 13
    R = ns + nd
    uv = rng.random((N, H, W, 2, R)).astype(np.float32)
    lt = (rng.random((N, R, 3, H, W)) * 2).astype(np.float32)
    alpha = (rng.random((N, H, W)) > 0.25).astype(np.float32)
    uv[alpha == 0] = -1.0
    lt = lt * alpha[:, None, None]
    a_s, a_d = [rng.random((N, 3, H, W)).astype(np.float32) * 0.5 for _ in range(2)]
    lp = T(rng.random((16, 32, 3)).astype(np.float32)).to(DEV)
    tr = LightTransport(*[T(t).to(DEV) for t in (uv, lt, a_s, a_d, alpha)], nd)
    targets = T(rng.random((N, 3, H, W)).astype(np.float32)).to(DEV)
    got = tr.score(lp, targets)
    assert list(got) == list(metrics.KEYS) and all(v.shape == (N,) and v.is_cuda and v.dtype == torch.float64 for v in got.values())
    frames = tr.render(lp)
    want = ops.image_metrics(frames, targets, tr.alpha, scale=255.0)
    stacked = torch.stack([got[k] for k in metrics.KEYS], 1)
    assert torch.equal(stacked.view(torch.int64), want.view(torch.int64))
    ref, _ = mr.batch(frames.cpu().numpy(), targets.cpu().numpy(), alpha, scale=255.0)
    mr.compare(stacked.cpu().numpy(), None, ref, None, 'score %dx%d' % size)
    assert np.isnan(ref[:, 9:]).all() == (H < 11)
    no_ssim = tr.score(lp, targets, mask=torch.ones(N, 1, H, W, device=DEV), compute_ssim=False)
    assert torch.isnan(no_ssim['ssim']).all() and float(no_ssim['mae'][0]) == float(no_ssim['mae_bb'][0]) == float(no_ssim['mae_valid'][0])
