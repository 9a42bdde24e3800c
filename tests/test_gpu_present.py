"""-m gpu: the presenter (rnr_present_u8: the frame as 8-bit B,G,R over the light-probe background) and the stand-alone
background operator (rnr_env_background), against the reference composed in tests/present_ref.py from oracle/ (float32
directions and tap coordinates, float64 colour, the numpy quantiser), and RNRPipeline(present=...).

Shapes are the smallest at which the paths differ: H W a multiple of 4 or not (four pixels per thread / one), W not a multiple
of 4 (groups straddle rows), out misaligned by a byte, several views, probes of 1 x 1 (every tap clamps), 5 x 9 and 100 x 200.
Tolerances are derived (present_ref.colour_tol), never measured; every test prints its figures before it asserts."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import present_ref as pr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
T = pr.T
PRE, POST = 64, 67          # guard bytes around a carved output


def _carve(nbytes, offset, shape, dtype=torch.uint8):
    """`nbytes` of output inside a larger pattern-filled byte buffer, PRE + offset bytes from its (>= 256-byte aligned) start."""
    total = PRE + offset + nbytes + POST
    pattern = ((np.arange(total) * 37 + 11) % 251).astype(np.uint8)
    buf = T(pattern).to(DEV)
    out = buf[PRE + offset:PRE + offset + nbytes].view(dtype).view(shape)
    assert out.data_ptr() % 4 == offset % 4
    return buf, out, pattern


def _guards_intact(buf, pattern, nbytes, offset):
    got = buf.cpu().numpy()
    lo = PRE + offset
    return bool((got[:lo] == pattern[:lo]).all() and (got[lo + nbytes:] == pattern[lo + nbytes:]).all())


# ------------------------------------------------------------------------------------------------
# 1. quantiser
# ------------------------------------------------------------------------------------------------
# [N,H,W], byte offset of out: four pixels per thread | H W odd: one per thread | H W % 4 == 0 but W % 4 != 0: groups straddle
# rows | the vector shape one byte off alignment: one pixel per thread
QUANT_CASES = [((1, 8, 16), 0), ((2, 7, 13), 0), ((3, 6, 10), 0), ((2, 8, 16), 1)]


@pytest.mark.parametrize('rgb', [False, True], ids=['bgr', 'rgb'])
@pytest.mark.parametrize('size,offset', QUANT_CASES, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else 'off%d' % v)
def test_quantiser_exact(size, offset, rgb):
    """RNR_PRESENT_FRAME byte for byte against q(v) = clip(rint(float32(v) * float32(255)), 0, 255) with NaN -> 0, +inf -> 255,
    -inf -> 0, on every tie (k + 0.5) / 255 (all 255 products are exact in float32), both float32 neighbours of each, 0, -0, 1,
    values just outside [0, 1], -3, 7, +-inf and NaN.  The 777 values do not fit one image of these sizes, so each size is
    presented as often as it takes to pass every value through its path.  out is carved from a pattern-filled buffer: the bytes
    before and after it stay as they were."""
    from rnr_amd import ops
    N, H, W = size
    vals = pr.quantiser_values()
    n = N * 3 * H * W
    wrong = 0
    for c in range(math.ceil(len(vals) / n)):
        img = np.resize(np.roll(vals, -c * n), (N, 3, H, W))
        buf, out, pattern = _carve(N * H * W * 3, offset, (N, H, W, 3))
        ops.present_u8(T(img).to(DEV), None, None, None, None, mode='frame', rgb=rgb, out=out)
        want = pr.to_bytes(img, rgb=rgb)
        wrong += int((out.cpu().numpy() != want).sum())
        assert _guards_intact(buf, pattern, N * H * W * 3, offset)
    print('quantiser %s off %d rgb %d: %d wrong bytes' % (size, offset, rgb, wrong))
    assert wrong == 0


# ------------------------------------------------------------------------------------------------
# 2. rnr_env_background vs float64
# ------------------------------------------------------------------------------------------------
BG_CASES = [(cam, size, lp_hw, per_view) for cam in pr.CAMERAS for size in pr.SIZES for lp_hw in pr.PROBES
            for per_view in ((False, True) if size[0] > 1 else (False,))]
_bg_id = lambda v: v if isinstance(v, str) else ('x'.join(map(str, v)) if isinstance(v, tuple) else 'lpN%d' % v)


@pytest.mark.parametrize('cam,size,lp_hw,per_view', BG_CASES, ids=_bg_id)
def test_env_background_vs_float64(cam, size, lp_hw, per_view):
    """rnr_env_background (view_dir<NormExact>, ocml atan2f / acosf, Taps::blend) vs present_ref.background, lp_n = 1 and N.

    Per-pixel tolerance, derived in present_ref.colour_tol(fused=False):
        (Wl du + Hl dv + 2 EPS (Wl + Hl)) x (probe gradient per texel) + 10 EPS max|lp|,
        du = (68 EPS / rho + 4.8e-7) / 2 pi + 1.5e-7,   dv = (68 EPS / rho + 4.8e-7) / pi + 1.2e-7,   rho = sqrt(d.x^2 + d.z^2):
    68 EPS is the direction error of the kernel's plus the reference's float32 normalisations (34 each), 4.8e-7 rad ocml's and
    torch's atan2f / acosf (2 ulp of pi each), the rest the roundings of u, v, the tap products and the blend.  No pixel is
    excluded: the preconditions hold for every pixel (test_present_cpu.py) and the excluded share is asserted to be 0."""
    from rnr_amd import ops
    N, H, W = size
    c = pr.case(cam, size, lp_hw, per_view)
    assert pr.preconditions(c['d'])[0] == 0.0
    lp = T(c['lp']).to(DEV)
    out = torch.full((N, H, W, 3), float('nan'), device=DEV)
    ops.env_background(T(c['proj_inv']).to(DEV), T(c['R_inv']).to(DEV), lp if per_view else lp[0], (H, W), out=out)
    tol = pr.colour_tol(c['lp'], c['d'], fused=False)
    err = (out.cpu().double() - c['ref']).abs().amax(-1)
    print('env_background %s %s lp %s lp_n %d: max err %.3g, max err / tol %.3g' % (cam, size, lp_hw, N if per_view else 1,
                                                                                  float(err.max()), float((err / tol).max())))
    assert not torch.isnan(out).any()
    assert (err <= tol).all(), float((err / tol).max())


# ------------------------------------------------------------------------------------------------
# 3. exact seam and pole pixels
# ------------------------------------------------------------------------------------------------
# signed-permutation R_inv -> -view_dir of the centre pixel, what it must select: (column by u, row by v)
AXIS_CASES = {
    'seam+0': ([[0, 0, -1], [0, 1, 0], [1, 0, 0]], (-1.0, 0.0, +0.0)),      # z = +0: atan2 = +pi, u = 1: column Wl - 1
    'seam-0': ([[0, 0, -1], [0, 1, 0], [-1, 0, 0]], (-1.0, 0.0, -0.0)),     # z = -0: atan2 = -pi, u = 0: column 0
    'pole+y': ([[1, 0, 0], [0, 0, 1], [0, 1, 0]], (0.0, 1.0, 0.0)),         # v = 0: row 0
    'pole-y': ([[1, 0, 0], [0, 0, -1], [0, 1, 0]], (0.0, -1.0, 0.0)),       # v = 1: row Hl - 1
}


@pytest.mark.parametrize('name', list(AXIS_CASES))
def test_exact_seam_and_pole_pixels(name):
    """proj_inv = [[1,0,-cx],[0,1,-cy],[0,0,f]] with (cx, cy) a pixel centre and f = 1: that pixel's camera direction is
    exactly (0, 0, -1); a signed-permutation R_inv turns -view_dir into exactly (-1, 0, +0), (-1, 0, -0), (0, +1, 0), (0, -1, 0)
    (checked, sign bits included, on rnr_view_dir_map's output, whose bits rnr_env_background claims).  Expected, exact:
    u = 1 -> column Wl - 1, u = 0 -> column 0, v = 0 -> row 0, v = 1 -> row Hl - 1 — the float32 values torch's sign-bit atan2
    gives on those directions — so the pixel IS one texel of the probe: equal as floats in rnr_env_background, equal as bytes
    in rnr_present_u8(BACKGROUND) (texels (j + 0.25) / 255: a byte names its texel, and stays put under the 6e-9 the
    polynomial u is off 0 at the seam).  5 x 8 pixels: the four-per-thread path of the presenter; 3 x 5: one per thread."""
    from oracle import rnr_oracle as orc
    from rnr_amd import ops
    r_inv, want_d = AXIS_CASES[name]
    lh, lw = 4, 8
    lp = ((np.arange(lh * lw * 3, dtype=np.float64) + 0.25) / 255).astype(np.float32).reshape(lh, lw, 3)
    for H, W, row, col in ((5, 8, 2, 3), (3, 5, 1, 4)):
        pi = T(np.array([[[1, 0, -(col + 0.5)], [0, 1, -(row + 0.5)], [0, 0, 1]]], np.float32)).to(DEV)
        ri = T(np.array([r_inv], np.float32)).to(DEV)
        world, _ = ops.view_dir_map((H, W), pi, ri)
        d = -world.cpu()[0, row, col]
        assert d.tolist() == list(want_d) and np.signbit(d.numpy()[2]) == np.signbit(np.float32(want_d[2])), d
        uv = orc.spherical_mapping(d, dim=0)
        u, v = float(uv[0]), float(uv[1])
        if name.startswith('seam'):
            assert (u, v) == ((1.0, 0.5) if name == 'seam+0' else (0.0, 0.5))
        else:
            assert v == (0.0 if name == 'pole+y' else 1.0) and u in (0.0, 0.5, 1.0)
        x, y = pr.tap_coords(d[None], lh, lw)
        tcol, trow = int(x[0]), int(y[0])
        assert float(x[0]) == tcol and float(y[0]) == trow             # the pixel is one texel
        assert tcol == {1.0: lw - 1, 0.0: 0, 0.5: lw // 2}[u] and trow == {0.0: 0, 0.5: lh // 2, 1.0: lh - 1}[v]
        want = lp[trow, tcol]
        bg = ops.env_background(pi, ri, T(lp).to(DEV), (H, W)).cpu().numpy()[0, row, col]
        print('%s %dx%d: d %s u %g v %g -> texel (%d, %d); env_background %s' % (name, H, W, d.tolist(), u, v, trow, tcol, bg))
        assert (bg == want).all(), (bg, want)
        b = ops.present_u8(None, None, pi, ri, T(lp).to(DEV), mode='background', rgb=True, img_hw=(H, W)).cpu().numpy()[0, row, col]
        assert (b == pr.quantise(want)).all(), (b, pr.quantise(want))


# ------------------------------------------------------------------------------------------------
# 4. rnr_present_u8: BACKGROUND and COMPOSITE
# ------------------------------------------------------------------------------------------------
def _alpha(N, H, W):
    """Foreground blocks, single pixels, a value in (0, 1) and a negative one in view 0; view 1 (if any) fully covered."""
    a = np.zeros((N, H, W), np.float32)
    a[0, 1:4, 2:7] = 1.0
    a[0, 0, 0] = a[0, H - 1, W - 1] = a[0, H - 2, W // 2] = 1.0
    a[0, 0, W - 1] = 0.5            # alpha > 0: foreground
    a[0, H - 1, 0] = -1.0           # not > 0: background
    if N > 1:
        a[1:] = 1.0
    return a


@pytest.mark.parametrize('cam,size,lp_hw', [c[:3] for c in BG_CASES if not c[3]], ids=_bg_id)
def test_present_background_and_composite(cam, size, lp_hw):
    """Every byte g of RNR_PRESENT_BACKGROUND: |g - clip(255 r, 0, 255)| <= 0.5 + 255 tol, r the float64 colour of
    present_ref.background, tol = present_ref.colour_tol(fused=True) + 1 EPS max|lp|: the stand-alone bound with the fused
    kernel's terms — 74 EPS direction error (v_rsq normalisations: 40, the reference's 34) and fast_atan2f / fast_acosf against
    torch's (7e-7 / 7.4e-7 rad, _colour_tol of test_gpu_shade_sweep.py); the FMA blend rounds no more than the plain one; 1 EPS
    for the product with 255.  RNR_PRESENT_COMPOSITE: foreground bytes (alpha > 0) equal the quantiser's rule exactly, background
    bytes equal the BACKGROUND call's (hence meet the bound), and the frame — non-zero everywhere — does not leak where alpha is
    not > 0.  Both channel orders.  No pixel excluded (share asserted 0)."""
    from rnr_amd import ops
    N, H, W = size
    c = pr.case(cam, size, lp_hw, False)
    assert pr.preconditions(c['d'])[0] == 0.0
    pi, ri, lp = T(c['proj_inv']).to(DEV), T(c['R_inv']).to(DEV), T(c['lp'][0]).to(DEV)
    tol = pr.colour_tol(c['lp'], c['d'], fused=True) + pr.EPS * float(np.abs(c['lp']).max())
    bound = (0.5 + 255 * tol)[..., None]
    target = (255 * c['ref']).clamp(0, 255)
    bg = ops.present_u8(None, None, pi, ri, lp, mode='background', rgb=True, img_hw=(H, W)).cpu()
    err = (bg.double() - target).abs()
    print('present background %s %s lp %s: max |g - 255 r| %.4f, max bound %.4f, worst err - bound %.3g'
          % (cam, size, lp_hw, float(err.max()), float(bound.max()), float((err - bound).max())))
    assert (err <= bound).all()
    rng = np.random.default_rng(H * W + lp_hw[1])
    img = (rng.random((N, 3, H, W)) * 1.4 - 0.2).astype(np.float32)
    alpha = _alpha(N, H, W)
    comp = ops.present_u8(T(img).to(DEV), T(alpha).to(DEV), pi, ri, lp, mode='composite', rgb=True).cpu()
    fg = T(alpha > 0)
    assert fg.any() and (~fg).any()
    assert torch.equal(comp[fg], T(pr.to_bytes(img, rgb=True))[fg])
    assert torch.equal(comp[~fg], bg[~fg])
    bgr = ops.present_u8(T(img).to(DEV), T(alpha).to(DEV), pi, ri, lp, mode='composite').cpu()
    assert torch.equal(bgr, comp.flip(-1))


@pytest.mark.parametrize('which', ['image', 'alpha'])
def test_misaligned_planes_take_the_one_pixel_path(which):
    """The four-pixel path loads its planes as float4: rnr_present_u8 takes it only when image (and, for COMPOSITE, alpha) are
    16-byte aligned.  [2,8,16] with out aligned and the image, or alpha, one float (4 bytes) off a 16-byte boundary: the bytes
    equal those of the aligned call and the quantiser's rule, and out's surroundings stay as they were."""
    from rnr_amd import ops
    N, H, W = 2, 8, 16
    c = pr.case('seeded', (2, 7, 13), (5, 9), False)
    pi, ri, lp = T(c['proj_inv']).to(DEV), T(c['R_inv']).to(DEV), T(c['lp'][0]).to(DEV)
    rng = np.random.default_rng(8)
    img = T((rng.random((N, 3, H, W)) * 1.4 - 0.2).astype(np.float32)).to(DEV)
    alpha = T(_alpha(N, H, W)).to(DEV)
    alpha[1, 2:5, 3:9] = 0.0
    aligned = ops.present_u8(img, alpha, pi, ri, lp, mode='composite').cpu()

    def shifted(t):
        store = torch.empty(t.numel() + 1, dtype=torch.float32, device=DEV)
        out = store[1:].view(t.shape)
        out.copy_(t)
        assert out.data_ptr() % 16 == 4 and out.is_contiguous()
        return out
    a = dict(image=shifted(img) if which == 'image' else img, alpha=shifted(alpha) if which == 'alpha' else alpha)
    buf, out, pattern = _carve(N * H * W * 3, 0, (N, H, W, 3))
    ops.present_u8(a['image'], a['alpha'], pi, ri, lp, mode='composite', out=out)
    assert torch.equal(out.cpu(), aligned) and _guards_intact(buf, pattern, N * H * W * 3, 0)
    fg = alpha.cpu() > 0
    assert torch.equal(aligned[fg], T(pr.to_bytes(img.cpu().numpy()))[fg])
    if which == 'image':        # FRAME reads the image alone
        buf, out, pattern = _carve(N * H * W * 3, 0, (N, H, W, 3))
        ops.present_u8(a['image'], None, None, None, None, mode='frame', out=out)
        assert (out.cpu().numpy() == pr.to_bytes(img.cpu().numpy())).all() and _guards_intact(buf, pattern, N * H * W * 3, 0)


# ------------------------------------------------------------------------------------------------
# 5. argument errors
# ------------------------------------------------------------------------------------------------
def test_argument_errors_leave_out_untouched():
    """Unknown mode, a NULL pointer the mode reads, lp_h or lp_w < 1, a probe of 2^24 floats or more (2048 x 2731 x 3 is the first
    such width at 2048 rows; the header's limit), sizes <= 0 (and, for rnr_env_background, a probe batch that is neither 1 nor
    N): non-zero return, a message in rnr_last_error(), no launch — out keeps its pattern."""
    from rnr_amd import _lib, ops
    L = _lib.load()
    N, H, W, lh, lw = 2, 4, 6, 3, 5
    img = torch.rand(N, 3, H, W, device=DEV)
    alpha = torch.ones(N, H, W, device=DEV)
    pi = torch.eye(3, device=DEV).repeat(N, 1, 1).contiguous()
    lp = torch.rand(N, lh, lw, 3, device=DEV)
    buf, out, pattern = _carve(N * H * W * 3, 0, (N, H, W, 3))
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)
    FRAME, COMP, BG, RGB = 0, 1, 2, 8
    ok = dict(image=img, alpha=alpha, proj_inv=pi, R_inv=pi, lp=lp, lp_h=lh, lp_w=lw, mode=COMP, out=out, n=N, h=H, w=W)
    bad = [dict(mode=3), dict(mode=4 | RGB), dict(mode=-1), dict(mode=16), dict(out=None), dict(image=None), dict(image=None, mode=FRAME),
           dict(alpha=None), dict(proj_inv=None), dict(R_inv=None, mode=BG), dict(lp=None, mode=BG | RGB), dict(lp_h=0), dict(lp_w=0, mode=BG),
           dict(lp_h=-2), dict(n=0), dict(h=0), dict(w=-1), dict(n=-3, mode=FRAME),
           dict(lp_h=2048, lp_w=2731), dict(lp_h=1 << 12, lp_w=1 << 12, mode=BG)]      # 3 Hl Wl >= 2^24: 24-bit texel offsets
    with ops.on_device(DEV):
        for kw in bad:
            a = dict(ok, **kw)
            rc = L.rnr_present_u8(P(a['image']), P(a['alpha']), P(a['proj_inv']), P(a['R_inv']), P(a['lp']), a['lp_h'], a['lp_w'],
                                  a['mode'], P(a['out']), a['n'], a['h'], a['w'], ops._stream())
            msg = L.rnr_last_error().decode()
            assert rc != 0 and msg.startswith('rnr_present_u8'), (kw, rc, msg)
        torch.cuda.synchronize()
        assert (buf.cpu().numpy() == pattern).all()
        # the same arguments without the fault do launch (so the list above tests the checks, not a dead entry point)
        assert L.rnr_present_u8(P(img), P(alpha), P(pi), P(pi), P(lp), lh, lw, COMP, P(out), N, H, W, ops._stream()) == 0
        torch.cuda.synchronize()
        assert not (out.cpu().numpy().ravel() == pattern[PRE:PRE + N * H * W * 3]).all()
        buf, out, pattern = _carve(N * H * W * 3 * 4, 0, (N, H, W, 3), torch.float32)
        ok = dict(proj_inv=pi, R_inv=pi, lp=lp, lp_n=N, lp_h=lh, lp_w=lw, out=out, n=N, h=H, w=W)
        bad = [dict(proj_inv=None), dict(R_inv=None), dict(lp=None), dict(out=None), dict(lp_n=0), dict(lp_n=3), dict(lp_h=0), dict(lp_w=-1),
               dict(n=0), dict(h=-1), dict(w=0), dict(lp_h=2048, lp_w=2731)]
        for kw in bad:
            a = dict(ok, **kw)
            rc = L.rnr_env_background(P(a['proj_inv']), P(a['R_inv']), P(a['lp']), a['lp_n'], a['lp_h'], a['lp_w'], P(a['out']), a['n'],
                                      a['h'], a['w'], ops._stream())
            msg = L.rnr_last_error().decode()
            assert rc != 0 and msg.startswith('rnr_env_background'), (kw, rc, msg)
        torch.cuda.synchronize()
        assert (buf.cpu().numpy() == pattern).all()
    with pytest.raises(ValueError):
        ops.present_u8(img, alpha, pi, pi, lp[0], mode='overlay')
    with pytest.raises(ValueError):
        ops.present_u8(img, alpha, pi[:1], pi, lp[0], mode='composite')         # one 3x3 per view


# ------------------------------------------------------------------------------------------------
# 6. pipeline
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def small():
    """The 64^2, nf0 = 4 scene of the existing frame tests, four poses, the frames / alpha of a pipeline built WITHOUT the
    new arguments (one view per call and all four at once), computed once."""
    from rnr_amd import scene, testing
    from rnr_amd.pipeline import RNRPipeline
    sc = testing.tiny_scene(img_size=64, nf0=4, tex_size=32, tex_ch=16, nlat=16, nlon=32, seed=0)

    def mk(**kw):
        kw.setdefault('max_views', 4)
        return RNRPipeline(sc['mesh'], 64, sc['textures'], sc['unet_sd'], sc['pivots_spec'], sc['pivots_diff'], sc['lp'], nf0=4,
                           device=DEV, **kw)
    v = {k: T(x).to(DEV) for k, x in scene.spiral_views(64, [5, 200, 400, 650]).items()}
    args = lambda lo, hi: (v['proj'][lo:hi], v['pose'][lo:hi], v['proj_inv'][lo:hi], v['R_inv'][lo:hi])
    base = mk()
    frames = base.render(*args(0, 4), keep_intermediates=True).clone()
    alpha = base.last['gb']['alpha'].clone()
    assert 0.1 < float((alpha > 0).float().mean()) < 0.9
    lp = torch.as_tensor(sc['lp'], dtype=torch.float32).reshape(sc['lp'].shape[-3], sc['lp'].shape[-2], 3).contiguous().to(DEV)
    return {'sc': sc, 'mk': mk, 'args': args, 'v': v, 'base': base, 'frames': frames, 'alpha': alpha, 'lp': lp}


def _by_hand(small, frame, lo, hi, lp=None, mode='composite', rgb=False):
    from rnr_amd import ops
    v = small['v']
    return ops.present_u8(frame.contiguous(), small['alpha'][lo:hi].contiguous(), v['proj_inv'][lo:hi], v['R_inv'][lo:hi],
                          small['lp'] if lp is None else lp, mode=mode, rgb=rgb)


def test_pipeline_present_off_is_todays_pipeline(small):
    """present=None: render() / submit() frames bit-identical to a pipeline built without the argument; presented / .u8 None,
    and no 8-bit buffer exists."""
    off = small['mk'](present=None)
    assert torch.equal(off.render(*small['args'](0, 4)), small['frames'])
    assert off.presented is None and off._own.u8 == [None, None]
    h = off.submit(*small['args'](1, 3))
    assert torch.equal(h.synchronize(), small['base'].render(*small['args'](1, 3))) and h.u8 is None and off.presented is None
    fly = small['mk'](present=None, inflight=2)
    h = fly.submit(*small['args'](0, 2))
    assert torch.equal(h.synchronize(), small['base'].render(*small['args'](0, 2))) and h.u8 is None
    assert all(s.u8 == [None, None] for s in fly._slots)


@pytest.mark.parametrize('kw', [dict(), dict(fuse_ray=True), dict(streams=2, max_views=3), dict(present_rgb=True), dict(present='frame')],
                         ids=['plain', 'fuse_ray', 'streams2_3views', 'rgb', 'frame'])
def test_pipeline_presented_equals_present_u8_by_hand(small, kw):
    """present='composite' (and 'frame'): the float frame is bit-identical to the present=None frame of the same pipeline
    options, and `presented` equals ops.present_u8(frame, alpha, ...) called by hand — on the plain path, with the ray renderer
    in the out layer's epilogue, with two stream lanes on three views, in R,G,B."""
    n = kw.get('max_views', 4)
    opts = {k: x for k, x in kw.items() if k not in ('present', 'present_rgb')}
    mode = kw.get('present', 'composite')
    want = small['frames'][:n] if not opts else small['mk'](**opts).render(*small['args'](0, n)).clone()
    pipe = small['mk'](**dict(kw, present=mode))
    frame = pipe.render(*small['args'](0, n))
    assert torch.equal(frame, want)
    u8 = pipe.presented
    assert u8 is not None and u8.dtype == torch.uint8 and tuple(u8.shape) == (n, 64, 64, 3)
    hand = _by_hand(small, frame, 0, n, mode=mode, rgb=kw.get('present_rgb', False))
    assert torch.equal(u8, hand)
    bgpix = ~(small['alpha'][:n] > 0)
    if mode == 'composite':
        assert float(u8[bgpix].float().mean()) > 20.0         # the probe, not black, behind the object
    else:
        assert int(u8[bgpix].max()) == 0                       # the frame alone is exactly 0 there
    # a second call flips to the other buffer pair: the first call's bytes are still what they were
    first = u8.clone()
    again = pipe.render(*small['args'](0, 1))
    assert pipe.presented.data_ptr() != u8.data_ptr() and torch.equal(u8, first)
    assert torch.equal(pipe.presented, _by_hand(small, again, 0, 1, mode=mode, rgb=kw.get('present_rgb', False)))


def test_pipeline_present_calls_in_flight(small):
    """inflight=2 over four submits (1, 2, 1, 2 views): every handle's float frame is bit-identical to the frame the same
    submits give on an inflight=2 pipeline built without `present`, and its .u8 the by-hand bytes — all four read only after
    the fourth submit, inside the documented lifetime (2 x inflight further submits)."""
    pipe = small['mk'](present='composite', inflight=2)
    plain = small['mk'](inflight=2)
    spans = [(0, 1), (1, 3), (3, 4), (0, 2)]
    handles = [pipe.submit(*small['args'](lo, hi)) for lo, hi in spans]
    want = [plain.submit(*small['args'](lo, hi)) for lo, hi in spans]
    assert pipe.presented is handles[-1].u8 and all(w.u8 is None for w in want)
    for (lo, hi), h, w in zip(spans, handles, want):
        frame = h.wait()
        ref = w.wait()
        torch.cuda.synchronize()
        assert torch.equal(frame, ref), (lo, hi, float((frame - ref).abs().max()))
        assert h.u8 is not None and torch.equal(h.u8, _by_hand(small, frame, lo, hi))
    one = small['mk'](present='composite')
    h = one.submit(*small['args'](2, 3))                       # inflight == 1: render + an event
    assert torch.equal(h.u8, _by_hand(small, h.synchronize(), 2, 3))


def test_pipeline_background_probe_is_honoured(small):
    """background_probe [7,11,3] (another size than the 100 x 200 lighting probe): background bytes follow it, foreground bytes
    do not change, the float frame does not change."""
    rng = np.random.default_rng(5)
    probe = T((0.2 + 0.6 * rng.random((7, 11, 3))).astype(np.float32)).to(DEV)
    pipe = small['mk'](present='composite', background_probe=probe)
    frame = pipe.render(*small['args'](0, 4))
    assert torch.equal(frame, small['frames'])
    u8 = pipe.presented
    assert torch.equal(u8, _by_hand(small, frame, 0, 4, lp=probe))
    lit = _by_hand(small, frame, 0, 4)
    fg = small['alpha'] > 0
    assert torch.equal(u8[fg], lit[fg])
    assert float((u8[~fg].int() - lit[~fg].int()).abs().float().mean()) > 5.0
    with pytest.raises(ValueError):
        small['mk'](present='overlay')


@pytest.mark.parametrize('kw', [dict(), dict(streams=2, max_views=3), dict(inflight=2)], ids=['fused', 'streams2_3views', 'inflight2'])
def test_pipeline_composite_under_sh_lighting_uses_the_calls_probe(small, kw):
    """SH lighting (sh_coeff given, lp=None): 'composite' shows the probe reconstructed for THIS call's lighting_idx — the one
    frame_prepare writes in a fused group or a slot in flight, SHLighting.light_probe on the stream-lane path (img_bg_sh).
    By hand: ops.present_u8 on LightingSH's reconstruction of the same coefficients; lighting_idx 1 then 0, so a probe left over
    from another call would show.  The float frames are bit-identical to the same pipeline without `present`."""
    from rnr_amd import ops, scene
    from rnr_amd.pipeline import RNRPipeline
    sc, v = small['sc'], small['v']
    coeff = torch.from_numpy(scene.synthetic_sh_coeff(2, 10, 3))
    n = kw.get('max_views', 4)

    def mk(**more):
        o = dict(kw, **more)
        o.setdefault('max_views', 4)
        return RNRPipeline(sc['mesh'], 64, sc['textures'], sc['unet_sd'], sc['pivots_spec'], sc['pivots_diff'], None, nf0=4,
                           device=DEV, sh_coeff=coeff, sh_lmax=10, **o)
    pipe, plain = mk(present='composite'), mk()
    run = (lambda p, idx: p.submit(*small['args'](0, n), lighting_idx=idx)) if 'inflight' in kw else \
          (lambda p, idx: p.render(*small['args'](0, n), lighting_idx=idx))
    probes = []
    for idx in (1, 0):
        got, ref = run(pipe, idx), run(plain, idx)
        u8 = got.u8 if 'inflight' in kw else pipe.presented
        frame, want = (got.synchronize(), ref.synchronize()) if 'inflight' in kw else (got, ref)
        torch.cuda.synchronize()
        assert torch.equal(frame, want)
        probe = pipe.sh_lighting.light_probe(pipe.sh_coeff[idx])
        probes.append(probe)
        hand = ops.present_u8(frame.contiguous(), small['alpha'][:n].contiguous(), v['proj_inv'][:n], v['R_inv'][:n], probe, mode='composite')
        assert torch.equal(u8, hand), idx
    bgpix = ~(small['alpha'][:n] > 0)
    other = ops.present_u8(frame.contiguous(), small['alpha'][:n].contiguous(), v['proj_inv'][:n], v['R_inv'][:n], probes[0], mode='composite')
    assert not torch.equal(other[bgpix], hand[bgpix])          # the two lightings do differ where the background shows
