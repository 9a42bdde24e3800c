"""-m gpu: WHERE the shading kernels (shade.hip) touch memory.  The float64 sweeps (test_gpu_shade_sweep.py, test_gpu_ray_backward.py,
test_gpu_texture_backward.py) check values on fresh torch allocations, where a load or store a few rows past the end neither
faults nor changes a checked value.  Here every operand of every entry point is carved out of a sentinel-filled allocation at
the weakest alignment include/rnr_hip.h grants it (rnr_amd.testing.EntryCalls), over the table oracle/shade_guard_cases.py:

  (a) guard sweep: all guards intact; no output element left as the sentinel, none non-finite; every deterministic output
      bitwise the unguarded run's (which the float64 sweeps verify); the atomic outputs (grad_lp, the texture gradients) within
      the bounds their own tests derive, (n + 16) EPS A_t and (n + 6) EPS A_t, untouched texels exactly 0;
  (b) NaN tracers, pure index properties compared bitwise with the clean run: regions the header says the ray kernels do not
      use hold the sentinel; one NaN planted at one pixel, one texel or one probe texel surfaces exactly where the formula says;
  (c) every alignment and size refusal of the entry points returns an error naming the entry point and launches nothing.
No tolerance here is measured."""
import numpy as np
import pytest
import torch

import texture_bwd_ref as tb
from oracle import shade_guard_cases as gc
from rnr_amd.testing import (ALIGN_BYTE, ALIGN_WORD, QUAD_OPERANDS, SENTINEL, EntryCalls, In, Levels, Out, Struct, Workspace,
                             _sentinel_bytes)
from test_gpu_conv_guard import assert_intact, bits
from test_gpu_ray_backward import _oracle_grads, _tap_counts

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24
T = gc.T
SENTINEL_I32 = SENTINEL - (1 << 32) if SENTINEL >= 1 << 31 else SENTINEL


def run_calls(calls, guard):
    ec = EntryCalls(guard)
    for fn, args in calls:
        ec.call(fn, **args)
    return ec


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def holds_sentinel(t):
    """Every byte of the device tensor t is still the sentinel's."""
    b = t.cpu().contiguous().view(-1).view(torch.uint8)
    return torch.equal(b, _sentinel_bytes(b.numel()))


def atomic_bounds(case, info):
    """{operand name: (tolerance tensor, A_t == 0 mask)} of the case's atomic outputs, from the host as their own tests do."""
    fn = case.fns[0]
    if fn == 'rnr_ray_renderer_backward' and 'grad_lp' not in info['skip']:
        s = info['scene']
        g = [None if k in info['skip'] else T(x) for k, x in zip(gc.RENDERER_G, s['g'])]
        mag = _oracle_grads(T(s['uv']), T(s['lt']), T(s['lp']), T(s['a_s']), T(s['a_d']), s['nd'], False, True, 1.0,
                            [None if x is None else x.abs() for x in g])
        n_t = _tap_counts(T(s['uv']), s['lp'].shape)[..., None].double()
        return {'grad_lp': ((n_t + 16) * EPS * mag[1], mag[1] == 0)}
    if fn == 'rnr_texture_mapper_backward':
        s = info['scene']
        sh = T(s['sh']) if s['sh'] is not None else None
        n_t, A_t = tb.tap_stats(T(s['uv']), sh, T(s['g']), s['sizes'], s['C'], gc.TEXTURE_SH_START)
        return {'grad_textures_host[%d]' % l: ((n.double() + 6) * EPS * A, A == 0) for l, (n, A) in enumerate(zip(n_t, A_t))}
    return {}


def check_sweep(case, finite=True):
    calls, info = case.make()
    g = run_calls(calls, True)
    assert_intact(case.id, g.report(), set(g.dev))
    u = run_calls(case.make()[0], False)
    got, ref = g.results(), u.results()
    assert set(got) == set(ref) and got
    atomic = atomic_bounds(case, info)
    for name, t in got.items():
        assert not bool((bits(t) == SENTINEL_I32).any()), '%s: %s holds the sentinel (unwritten, or a guard was read)' % (case.id, name)
        if finite and t.dtype.is_floating_point:
            assert bool(torch.isfinite(t).all()), '%s: %s not finite at %d elements' % (case.id, name, int((~torch.isfinite(t)).sum()))
        if name in atomic:
            tol, untouched = atomic[name]
            assert bool(((t.double() - ref[name].double()).abs() <= tol).all()), (case.id, name)
            assert float(t[untouched].abs().max() if untouched.any() else 0.0) == 0.0, (case.id, name)
        else:
            assert same_bits(t, ref[name]), '%s: %s differs from the unguarded run at %d elements' % (
                case.id, name, int((bits(t) != bits(ref[name])).sum()))
    assert not (set(atomic) - set(got))


@pytest.mark.parametrize('id', gc.SHADE_IDS)
def test_guard_sweep(id):
    check_sweep(gc.BY_ID[id])


# ------------------------------------------------------------------------------------------------
# (b) NaN tracers
# ------------------------------------------------------------------------------------------------
NAN = float('nan')


def _sentinel_like(t):
    return torch.full(t.shape, SENTINEL_I32, dtype=torch.int32).view(torch.float32)


def _run1(fn, args):
    return run_calls([(fn, args)], False).results()


@pytest.mark.parametrize('fn,key', [(fn, key) for key in ('sweep2', 'sweep3', 'npix33', 'bg_workgroup_3x4x8')
                                    for fn in ('rnr_ray_render', 'rnr_ray_weights', 'rnr_ray_transport')
                                    if fn != 'rnr_ray_weights' or gc.RAY[key][1] <= 15])
def test_unread_regions_hold_the_sentinel(fn, key):
    """Everything the header says the ray kernels do not use holds the sentinel NaN: unet_raw columns >= 3 R; the net_in
    channels other than the ray directions, normal / view and the two albedo triples; on background pixels the whole unet_raw
    row, the ray directions, normal / view — and for rnr_ray_weights, which selects, the albedo triples too (rnr_ray_render
    multiplies them with its zero sums as the reference does and rnr_ray_transport copies them: the header requires them finite
    there).  The outputs are bitwise the clean run's."""
    s = gc.ray_scene(key)
    clean = _run1(fn, gc.ray_args(fn, s))
    R = s['ns'] + s['nd']
    raw, ni = T(s['raw']).clone(), T(s['net_in']).clone()
    used = torch.zeros(ni.shape[-1], dtype=torch.bool)
    used[:3 * R + 6] = True
    for ch in s['alb']:
        used[3 * R + 6 + ch:3 * R + 9 + ch] = True
    raw[..., 3 * R:] = _sentinel_like(raw[..., 3 * R:])
    ni[..., ~used] = _sentinel_like(ni[..., ~used])
    bg = T(s['alpha']) == 0
    assert bool(bg.any())
    raw[bg] = _sentinel_like(raw[bg])
    keep = used.clone()
    keep[:3 * R + 6] = False                    # on background pixels only the albedo triples stay
    if fn == 'rnr_ray_weights':
        keep[:] = False
    row = ni[bg]
    row[:, ~keep] = _sentinel_like(row[:, ~keep])
    ni[bg] = row
    poisoned = _run1(fn, gc.ray_args(fn, dict(s, raw=raw.numpy(), net_in=ni.numpy())))
    for name, t in clean.items():
        assert bool(torch.isfinite(t).all()), name
        assert same_bits(poisoned[name], t), '%s %s: %s consumed an unused value at %d elements' % (
            fn, key, name, int((bits(poisoned[name]) != bits(t)).sum()))


def _pixel(p, H, W):
    return p // (H * W), (p % (H * W)) // W, p % W


def _only_pixel_differs(clean, dirty, pix_index, what):
    """clean / dirty: pixel-major views [npix, k] of one output; every row but pix_index bitwise equal."""
    other = torch.ones(clean.shape[0], dtype=torch.bool)
    other[pix_index] = False
    assert same_bits(dirty[other], clean[other]), '%s: a NaN at pixel %d reached %d other pixels' % (
        what, pix_index, int((bits(dirty[other]) != bits(clean[other])).any(-1).sum()))


# pixel-major views of rnr_shade_inputs' outputs
_SHADE_VIEWS = {'net_in': lambda t: t.reshape(-1, t.shape[-1]), 'rays_uv': lambda t: t.reshape(-1, t.shape[-2] * t.shape[-1]),
                'neural_img': lambda t: t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]), 'sh_basis_map': lambda t: t.reshape(-1, 9)}


@pytest.mark.parametrize('which', ['normal_map', 'uv_map', 'alpha'])
@pytest.mark.parametrize('id', ['C24_cpad_eq_cin_2x5x7_all', 'C28_one_level_2x5x7_rays_uv'])
def test_shade_inputs_pixel_locality(id, which):
    """One NaN in one per-pixel input of rnr_shade_inputs, at the first pixel of a workgroup (32), the last pixel of the view
    that workgroup straddles (34) and the last of the batch (69): that pixel's dependent channels are non-finite (normal: the
    copied normal; uv: every texture channel; alpha: the specular ray directions), every other pixel of every output is bitwise
    the clean run's."""
    spec = gc.SHADE[id]
    C, ns, nd, _, _, N, H, W = spec[:8]
    R = ns + nd
    args, s = gc.shade_inputs_args(spec)
    clean = _run1('rnr_shade_inputs', args)
    key = {'normal_map': 'normal', 'uv_map': 'uv', 'alpha': 'alpha'}[which]
    for p in (32, 34, 69):
        args, s = gc.shade_inputs_args(spec)
        x = T(s[key]).clone()
        x.reshape(N * H * W, -1)[p, 0] = NAN
        args[which] = In(x)
        dirty = _run1('rnr_shade_inputs', args)
        for name, view in _SHADE_VIEWS.items():
            if name in clean:
                _only_pixel_differs(view(clean[name]), view(dirty[name]), p, '%s -> %s' % (which, name))
        row = _SHADE_VIEWS['net_in'](dirty['net_in'])[p]
        dep = {'normal_map': row[3 * R:3 * R + 1], 'uv_map': row[3 * R + 6:3 * R + 6 + C], 'alpha': row[:3 * ns]}[which]
        assert dep.numel() and not bool(torch.isfinite(dep).any()), (which, p, dep)


def _level_taps_of(uv, side):
    """Per pixel of uv [npix, 2]: the four (row, column) taps and weights on a level of side `side` (the kernel's expressions)."""
    from oracle import rnr_oracle as orc
    x = uv[:, 0] * (side - 1)
    y = (side - 1) - uv[:, 1] * (side - 1)
    (x0, y0, x1, y1), (w00, w10, w01, w11) = orc.bilinear_taps(side, side, x, y)
    return ((y0, x0, w00), (y1, x0, w10), (y0, x1, w01), (y1, x1, w11))


def _texel_pixels(uv, side, y, x):
    """(must, may): pixels with texel (y, x) among their taps with non-zero weight / among their taps at all."""
    must = torch.zeros(uv.shape[0], dtype=torch.bool)
    may = torch.zeros(uv.shape[0], dtype=torch.bool)
    for yy, xx, w in _level_taps_of(uv, side):
        hit = (yy == y) & (xx == x)
        may |= hit
        must |= hit & (w != 0)
    return must, may


def _texels(uv, sizes):
    """(level, y, x) of three texels: the corner (0, 0) of level 0, the first texel of the last row of level 1 (of level 0 when
    there is one level only), and the interior texel of level 0 that the pixel in the middle of the batch taps hardest."""
    out = [(0, 0, 0)]
    l = 1 if len(sizes) > 1 else 0
    out.append((l, sizes[l] - 1, 0))
    mid = uv.shape[0] // 2
    yy, xx, w = max(_level_taps_of(uv[mid:mid + 1], sizes[0]), key=lambda t: float(t[2]))
    out.append((0, int(yy), int(xx)))
    return out


def _check_texel_tracer(clean, dirty, must, may, c, what):
    """clean / dirty [npix, C]: non-finite where must (channel c), nowhere outside may x (channel c: the blend is per channel and
    the SH factor does not mix channels, so a lane that mixed the channels of a float4 shows), bitwise clean wherever finite."""
    bad = ~torch.isfinite(dirty)
    assert bool(torch.isfinite(clean).all())
    assert bool(bad[must, c].all()), '%s: the texel did not surface at %d pixels that tap it' % (what, int((~bad[must, c]).sum()))
    allowed = torch.zeros_like(bad)
    allowed[:, c] = may
    assert not bool((bad & ~allowed).any()), '%s: the texel surfaced at %d elements that do not tap it' % (what, int((bad & ~allowed).sum()))
    assert same_bits(dirty[~bad], clean[~bad]), what
    assert bool(must.any()) and not bool(may.all())


@pytest.mark.parametrize('id', ['C24_cpad_eq_cin_2x5x7_all', 'C28_2x5x7_sh_basis_map'])
def test_shade_inputs_texel_locality(id):
    """One NaN in one texel (level, y, x, c) of rnr_shade_inputs' textures — a corner, the last row, an interior one — on the
    early-texture path (C = 24) and the fallback loop (C = 28): it surfaces in channel c of every pixel that taps the texel with
    a non-zero weight, possibly in pixels that tap it with weight 0 (the blend multiplies all four), nowhere else; the ray
    directions, normal, view direction and the other outputs are bitwise clean."""
    spec = gc.SHADE[id]
    C, ns, nd, _, levels, N, H, W = spec[:8]
    R = ns + nd
    args, s = gc.shade_inputs_args(spec)
    clean = _run1('rnr_shade_inputs', args)
    uv = T(s['uv']).reshape(-1, 2)
    for k, (l, y, x) in enumerate(_texels(uv, levels)):
        c = (5, C - 1, 0)[k]
        args, s = gc.shade_inputs_args(spec)
        tex = [T(t).clone() for t in s['tex']]
        tex[l][y, x, c] = NAN
        args['textures_host'] = Levels(In(t) for t in tex)
        dirty = _run1('rnr_shade_inputs', args)
        must, may = _texel_pixels(uv, levels[l], y, x)
        cn, dn = [_SHADE_VIEWS['net_in'](r['net_in']) for r in (clean, dirty)]
        _check_texel_tracer(cn[:, 3 * R + 6:3 * R + 6 + C], dn[:, 3 * R + 6:3 * R + 6 + C], must, may, c, '%s texel %s' % (id, (l, y, x, c)))
        assert same_bits(dn[:, :3 * R + 6], cn[:, :3 * R + 6]) and same_bits(dn[:, 3 * R + 6 + C:], cn[:, 3 * R + 6 + C:])
        for name in ('rays_uv', 'sh_basis_map'):
            if name in clean:
                assert same_bits(dirty[name], clean[name]), name
        if 'neural_img' in clean:
            assert same_bits(_SHADE_VIEWS['neural_img'](dirty['neural_img']), dn[:, 3 * R + 6:3 * R + 6 + C])


@pytest.mark.parametrize('with_sh', [False, True])
@pytest.mark.parametrize('hw', [(9, 13), (17, 19)])
def test_texture_mapper_texel_locality(hw, with_sh):
    """The same for rnr_texture_mapper (one lane per (pixel, channel): the NaN stays in channel c)."""
    s = gc.texture_scene(hw, with_sh, 'fwd')
    clean = _run1('rnr_texture_mapper', gc.texture_args(s, False))['out']
    uv = T(s['uv']).reshape(-1, 2)
    view = lambda t: t.permute(0, 2, 3, 1).reshape(-1, s['C'])
    for k, (l, y, x) in enumerate(_texels(uv, s['sizes'])):
        c = (5, s['C'] - 1, 0)[k]
        tex = [t.copy() for t in s['tex']]
        tex[l][y, x, c] = NAN
        dirty = _run1('rnr_texture_mapper', gc.texture_args(dict(s, tex=tex), False))['out']
        must, may = _texel_pixels(uv, s['sizes'][l], y, x)
        _check_texel_tracer(view(clean), view(dirty), must, may, c, 'texture_mapper %s texel %s' % (hw, (l, y, x, c)))
        bad = ~torch.isfinite(view(dirty))
        assert not bool(bad[:, [i for i in range(s['C']) if i != c]].any())


@pytest.mark.parametrize('hw', [(9, 13), (17, 19)], ids=['lanes_9x13', 'tiles_17x19'])
def test_texture_mapper_backward_pixel_locality(hw):
    """One NaN in one grad_out element (view, channel c, pixel) of rnr_texture_mapper_backward, both forms, at the first pixel
    of a workgroup (per-lane form: pixel 64 of the 64-pixel groups; tile form: row 16, column 0, the origin of a 16 x 16 tile) /
    the last pixel of view 0 / the last of the batch: the non-finite texels of every level are exactly that
    pixel's taps with non-zero weight, in channel c alone."""
    s = gc.texture_scene(hw, True, 'bwd')
    N, H, W, C = s['N'], s['H'], s['W'], s['C']
    uv = T(s['uv']).reshape(-1, 2)
    first = gc.TT * W if min(hw) >= gc.TT else gc.TB_PIX
    for p, c in ((first, 0), (H * W - 1, 5), (N * H * W - 1, C - 1)):
        n, y, x = _pixel(p, H, W)
        g = s['g'].copy()
        g[n, c, y, x] = NAN
        got = _run1('rnr_texture_mapper_backward', gc.texture_args(dict(s, g=g), True))
        for l, side in enumerate(s['sizes']):
            want = torch.zeros(side, side, dtype=torch.bool)
            for yy, xx, w in _level_taps_of(uv[p:p + 1], side):
                if float(w) != 0:
                    want[int(yy), int(xx)] = True
            bad = ~torch.isfinite(got['grad_textures_host[%d]' % l])
            assert bool(want.any()) and torch.equal(bad[..., c], want), (hw, p, l)
            bad[..., c] = False
            assert not bool(bad.any()), (hw, p, l)


# rnr_ray_renderer / rnr_ray_renderer_backward: pixel-major views [npix, k] of the [N,C,H,W] and [N,R,C,H,W] outputs
def _img_view(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]) if t.dim() == 4 else t.permute(0, 3, 4, 1, 2).reshape(-1, t.shape[1] * t.shape[2])


RENDERER_PIXELS = (64, 116, 233)        # first of a 64-pixel workgroup, last of view 0 (which workgroup 1 straddles), last of the batch


@pytest.mark.parametrize('form', ['tiled_C3_R13', 'lane_C5_R13'])
def test_ray_renderer_pixel_locality(form):
    """One NaN in one rays_lt element, then in one rays_uv element, of rnr_ray_renderer: `out` (and rays_color for the uv) is
    non-finite at that pixel, every other pixel of every output is bitwise clean."""
    s = gc.renderer_scene(form, False)
    N, H, W = gc.RENDERER_NHW
    clean = _run1('rnr_ray_renderer', gc.renderer_args(s, False))
    for p in RENDERER_PIXELS:
        n, y, x = _pixel(p, H, W)
        lt = s['lt'].copy()
        lt[n, 2, 1, y, x] = NAN
        uv = s['uv'].copy()
        uv[n, y, x, 0, 3] = NAN
        for tag, dirty_scene in (('rays_lt', dict(s, lt=lt)), ('rays_uv', dict(s, uv=uv))):
            dirty = _run1('rnr_ray_renderer', gc.renderer_args(dirty_scene, False))
            for name in clean:
                _only_pixel_differs(_img_view(clean[name]), _img_view(dirty[name]), p, '%s -> %s' % (tag, name))
            assert not bool(torch.isfinite(dirty['out'][n, 1, y, x])), (tag, p)
            if tag == 'rays_uv':
                assert not bool(torch.isfinite(dirty['rays_color'][n, 3, :, y, x]).any()), p


@pytest.mark.parametrize('form', ['tiled_C3_R13', 'lane_C5_R13'])
def test_ray_renderer_backward_pixel_locality(form):
    """One NaN in one g_out element of rnr_ray_renderer_backward: grad_rays_lt and the albedo gradients are non-finite at that
    pixel only, grad_lp exactly on the texels that pixel's rays tap with non-zero weight (computed as _tap_counts does), in
    that channel only."""
    s = gc.renderer_scene(form, False)
    N, H, W = gc.RENDERER_NHW
    clean = _run1('rnr_ray_renderer_backward', gc.renderer_args(s, True))
    c = 1
    for p in RENDERER_PIXELS:
        n, y, x = _pixel(p, H, W)
        g = [a.copy() for a in s['g']]
        g[0][n, c, y, x] = NAN
        dirty = _run1('rnr_ray_renderer_backward', gc.renderer_args(dict(s, g=g), True))
        for name in ('grad_rays_lt', 'grad_albedo_specular', 'grad_albedo_diffuse'):
            _only_pixel_differs(_img_view(clean[name]), _img_view(dirty[name]), p, 'g_out -> ' + name)
            assert not bool(torch.isfinite(_img_view(dirty[name])[p]).all()), (name, p)
        taps = _tap_counts(T(s['uv'][n:n + 1, y:y + 1, x:x + 1]), s['lp'].shape)[0] > 0
        assert bool(taps.any()) and not bool(taps.all())
        bad = ~torch.isfinite(dirty['grad_lp'][0])
        assert torch.equal(bad[..., c], taps), (p, int(bad[..., c].sum()), int(taps.sum()))
        bad[..., c] = False
        assert not bool(bad.any())


def _probe_texels(x, y, lh, lw):
    """A corner, a texel of the last row and an interior one among those float32 tap coordinates (x, y) [n] reach."""
    from oracle import rnr_oracle as orc
    (x0, y0, x1, y1), w = orc.bilinear_taps(lh, lw, x, y)
    hit = torch.zeros(lh, lw, dtype=torch.bool)
    for yy, xx, ww in ((y0, x0, w[0]), (y1, x0, w[1]), (y0, x1, w[2]), (y1, x1, w[3])):
        hit[yy[ww != 0], xx[ww != 0]] = True
    inner = hit.clone()
    inner[0], inner[-1], inner[:, 0], inner[:, -1] = False, False, False, False
    picks = []
    for region in (hit[0], hit[-1]):
        cols = region.nonzero().reshape(-1)
        picks.append(int(cols[0]) if len(cols) else None)
    out = [(0, picks[0])] if picks[0] is not None else []
    if picks[1] is not None:
        out.append((lh - 1, picks[1]))
    yy, xx = inner.nonzero()[len(inner.nonzero()) // 2].tolist()
    return out + [(yy, xx)]


def _probe_sets(x, y, lh, lw, ty, tx):
    """(must, may) [n]: samples with probe texel (ty, tx) among their non-zero-weight taps / among their taps."""
    from oracle import rnr_oracle as orc
    (x0, y0, x1, y1), w = orc.bilinear_taps(lh, lw, x, y)
    must, may = torch.zeros_like(x, dtype=torch.bool), torch.zeros_like(x, dtype=torch.bool)
    for yy, xx, ww in ((y0, x0, w[0]), (y1, x0, w[1]), (y0, x1, w[2]), (y1, x1, w[3])):
        h = (yy == ty) & (xx == tx)
        may |= h
        must |= h & (ww != 0)
    return must, may


def test_ray_renderer_probe_locality():
    """One NaN in one probe texel (all channels of it) under rnr_ray_renderer: rays_color is non-finite for every (pixel, ray)
    that taps the texel with non-zero weight, possibly where the weight is 0, nowhere else; `out` only at pixels with such a
    ray."""
    s = gc.renderer_scene('tiled_C3_R13', False)
    N, H, W = gc.RENDERER_NHW
    R, (lh, lw) = s['R'], s['lp'].shape[1:3]
    clean = _run1('rnr_ray_renderer', gc.renderer_args(s, False))
    uv = T(s['uv'])
    x = (uv[..., 0, :] * float(lw)).clamp(max=lw - 1).reshape(-1)
    y = (uv[..., 1, :] * float(lh)).clamp(max=lh - 1).reshape(-1)
    for ty, tx in _probe_texels(x, y, lh, lw):
        lp = s['lp'].copy()
        lp[0, ty, tx, :] = NAN
        dirty = _run1('rnr_ray_renderer', gc.renderer_args(dict(s, lp=lp), False))
        must, may = [m.reshape(N * H * W, R) for m in _probe_sets(x, y, lh, lw, ty, tx)]
        bad = ~torch.isfinite(dirty['rays_color'].permute(0, 3, 4, 1, 2).reshape(N * H * W, R, -1))
        assert bool(must.any()) and bool(bad[must].all()) and not bool(bad[~may].any()), (ty, tx)
        bad_out = ~torch.isfinite(_img_view(dirty['out']))
        assert bool(bad_out[must.any(1)].all()) and not bool(bad_out[~may.any(1)].any()), (ty, tx)
        for name in clean:
            a, b = _img_view(clean[name]), _img_view(dirty[name])
            assert same_bits(b[~may.any(1)], a[~may.any(1)]), name


@pytest.mark.parametrize('key', ['sweep2', 'sweep4'])
def test_ray_render_probe_locality(key):
    """The same under the fused rnr_ray_render.  Its taps are those of the uv rnr_ray_transport unpacks (same arithmetic, the
    header says; test_gpu_ray_backward.py checks it), so the host derives the sets from that output."""
    s = gc.ray_scene(key)
    N, H, W, R = s['N'], s['H'], s['W'], s['ns'] + s['nd']
    lh, lw = s['lp'].shape[:2]
    clean = _run1('rnr_ray_render', gc.ray_args('rnr_ray_render', s))['image']
    uv = _run1('rnr_ray_transport', gc.ray_args('rnr_ray_transport', s))['rays_uv']
    x = (uv[..., 0, :] * float(lw)).clamp(max=lw - 1).reshape(-1)
    y = (uv[..., 1, :] * float(lh)).clamp(max=lh - 1).reshape(-1)
    for ty, tx in _probe_texels(x, y, lh, lw):
        lp = s['lp'].copy()
        lp[ty, tx, :] = NAN
        dirty = _run1('rnr_ray_render', gc.ray_args('rnr_ray_render', dict(s, lp=lp)))['image']
        must, may = [m.reshape(N * H * W, R).any(1) for m in _probe_sets(x, y, lh, lw, ty, tx)]
        bad = ~torch.isfinite(_img_view(dirty)).any(1)
        assert bool(must.any()) and bool(bad[must].all()) and not bool(bad[~may].any()), (ty, tx)
        assert same_bits(_img_view(dirty)[~may], _img_view(clean)[~may])


def test_env_background_probe_locality():
    """One NaN in one probe texel under rnr_env_background.  The host has the kernel's directions only up to the rounding of
    atan2f / acosf (2 ulp of pi: 4.8e-7 rad, 4e-7 in u, v as test_gpu_shade_sweep.py derives, times the 9 texels of the probe's
    width: 4e-6) and of the view direction (34 EPS, test_view_dir_map_three_views_vs_float64): with a margin of 1e-4 texel, a
    pixel whose sample lies within 1 - 1e-4 texel of the planted one on both axes must show it, one farther than 1 + 1e-4 on
    either axis must be bitwise clean."""
    import present_ref as pr
    N, H, W = 3, 5, 17
    rng = np.random.default_rng(17)
    pi, ri = gc.sc._proj_inv(rng, N, H, W), gc.sc._rotations(rng, N)
    lp = (rng.random((1, 5, 9, 3))).astype(np.float32)
    args = lambda probe: dict(proj_inv=In(T(pi)), R_inv=In(T(ri)), lp=In(T(probe)), lp_n=1, lp_h=5, lp_w=9, out=Out((N, H, W, 3)),
                              num_views=N, height=H, width=W)
    clean = _run1('rnr_env_background', args(lp))['out'].reshape(-1, 3)
    x, y = pr.tap_coords(pr.directions(pi, ri, H, W), 5, 9)
    x, y = x.reshape(-1).double(), y.reshape(-1).double()
    for ty, tx in _probe_texels(x.float(), y.float(), 5, 9):
        probe = lp.copy()
        probe[0, ty, tx, :] = NAN
        dirty = _run1('rnr_env_background', args(probe))['out'].reshape(-1, 3)
        dx, dy = (x - tx).abs(), (y - ty).abs()
        must = (dx < 1 - 1e-4) & (dy < 1 - 1e-4)
        may = (dx < 1 + 1e-4) & (dy < 1 + 1e-4)
        bad = ~torch.isfinite(dirty).all(1)
        assert bool(must.any()) and bool(bad[must].all()) and not bool(bad[~may].any()), (ty, tx)
        assert same_bits(dirty[~may], clean[~may])


# ------------------------------------------------------------------------------------------------
# (c) refusals launch nothing
# ------------------------------------------------------------------------------------------------
# entry point -> (the case to start from, its size arguments: each <= 0 must be refused)
VIEW_SIZES = ('num_views', 'height', 'width')
REFUSALS = {
    'rnr_project_vertices': ('project_vertices-255_optional', ('num_views', 'num_vertices')),
    'rnr_face_tangents': ('face_tangents-255', ('mesh.num_faces',)),
    'rnr_shade_inputs': ('shade_inputs-C24_cpad_eq_cin_2x5x7_all', VIEW_SIZES + ('num_faces', 'num_levels', 'tex_channels')),
    'rnr_ray_render': ('ray_render-sweep2', VIEW_SIZES),
    'rnr_ray_weights': ('ray_weights-sweep2', VIEW_SIZES),
    'rnr_ray_transport': ('ray_transport-sweep2', VIEW_SIZES),
    'rnr_sh_basis': ('sh_basis-n127', ('n',)),
    'rnr_sh_reconstruct': ('sh_reconstruct-ns63_nb9', ('num_samples', 'num_basis', 'num_channels')),
    'rnr_sh_fit': ('sh_fit-ns63_nb9', ('num_samples', 'num_basis', 'num_channels')),
    'rnr_sh_reconstruct_backward': ('sh_reconstruct_backward-ns63_nb9', ('num_samples', 'num_basis', 'num_channels')),
    'rnr_interpolate_bilinear': ('interpolate_bilinear-n255_taps', ('h', 'w', 'c', 'n')),
    'rnr_resize_area': ('resize_area-shrink255', ('src_h', 'src_w', 'dst_h', 'dst_w', 'channels')),
    'rnr_nchw_to_nhwc': ('nchw_to_nhwc-255', ('n', 'c', 'h', 'w')),
    'rnr_nhwc_to_nchw': ('nhwc_to_nchw-255_bias_tanh', ('n', 'c', 'h', 'w')),
    'rnr_view_dir_map': ('view_dir_map-255_cam', VIEW_SIZES),
    'rnr_env_background': ('env_background-255_lpN', VIEW_SIZES + ('lp_h', 'lp_w')),
    'rnr_tbn_map': ('tbn_map-255', VIEW_SIZES + ('num_faces',)),
    'rnr_tbn_matvec': ('tbn_matvec-255_plain', ('num_pixels',)),
    'rnr_ray_sampler': ('ray_sampler-255_reflect', ('num_pixels', 'num_rays')),
    'rnr_texture_mapper': ('texture_mapper-9x13_sh', VIEW_SIZES + ('num_levels', 'tex_channels')),
    'rnr_texture_mapper_backward': ('texture_mapper_backward-9x13_sh', VIEW_SIZES + ('num_levels', 'tex_channels')),
    'rnr_ray_renderer': ('ray_renderer-tiled_C3_R13_lp1', VIEW_SIZES + ('channels', 'lp_h', 'lp_w')),
    'rnr_ray_renderer_backward': ('ray_renderer_backward-tiled_C3_R13_lp1', VIEW_SIZES + ('channels', 'lp_h', 'lp_w')),
}


def _operands(args, prefix=''):
    """(path, operand) of every device operand (In / Out / Workspace) of a call's arguments."""
    for k, v in args.items():
        if isinstance(v, (In, Out, Workspace)):
            yield prefix + k, v
        elif isinstance(v, Levels):
            for l in sorted({0, len(v) - 1}):
                yield '%s%s[%d]' % (prefix, k, l), v[l]
        elif isinstance(v, Struct):
            yield from _operands(v, prefix + k + '.')


def _set(args, path, value):
    if '.' in path:
        head, field = path.split('.')
        args[head][field] = value
    else:
        args[path] = value


def refusal_variants(fn, base_id, sizes, call_index=-1):
    """-> list of (tag, make) where make() gives the case's calls with one argument of call `call_index` made unacceptable: a
    size 0, or one device operand one alignment class below its contract."""
    variants = []
    for sz in sizes:
        def make(sz=sz):
            calls = gc.BY_ID[base_id].make()[0]
            _set(calls[call_index][1], sz, 0)
            return calls
        variants.append((sz + '=0', make))
    paths = [p for p, _ in _operands(gc.BY_ID[base_id].make()[0][call_index][1])]
    for path in paths:
        def make(path=path):
            calls = gc.BY_ID[base_id].make()[0]
            op = dict(_operands(calls[call_index][1]))[path]
            param = path.split('.')[0].split('[')[0]
            op.align = ALIGN_WORD if (fn, param) in QUAD_OPERANDS else ALIGN_BYTE
            return calls
        variants.append((path + ' misaligned', make))
    return variants


def check_refusals(fn, base_id, sizes, call_index=-1, named=None):
    from rnr_amd import _lib
    L = _lib.load()
    variants = refusal_variants(fn, base_id, sizes, call_index)
    assert len(variants) > len(sizes)
    for tag, make in variants:
        calls = make()
        ec = EntryCalls(True)
        for f, a in calls[:call_index] if call_index != -1 else calls[:-1]:
            ec.call(f, **a)
        before = {n: ec.dev[n].clone() for n in ec.outputs + ec.workspaces}
        f, a = calls[call_index]
        assert f == fn
        first_out, first_ws = len(ec.outputs), len(ec.workspaces)
        rc = ec.call(fn, check=False, **a)
        err = L.rnr_last_error().decode()
        assert rc != 0, '%s accepted %s' % (fn, tag)
        assert (named or fn) in err, (fn, tag, err)
        assert 'aligned' in err or not tag.endswith('misaligned'), (fn, tag, err)        # refused for that reason
        assert_intact('%s %s' % (fn, tag), ec.report(), set(ec.dev))
        for n in ec.outputs[first_out:] + ec.workspaces[first_ws:]:
            assert holds_sentinel(ec.dev[n]), '%s %s: %s was written' % (fn, tag, n)
        for n, t in before.items():
            assert torch.equal(ec.dev[n].view(-1).view(torch.uint8), t.view(-1).view(torch.uint8)), \
                '%s %s: %s of an earlier call was written' % (fn, tag, n)
    ok = run_calls(gc.BY_ID[base_id].make()[0], True)           # the same calls with valid arguments succeed
    assert all(not bool((bits(t) == SENTINEL_I32).any()) for n, t in ok.results().items() if t.element_size() == 4)


@pytest.mark.parametrize('fn', sorted(REFUSALS))
def test_refusals_launch_nothing(fn):
    """Every size argument 0 in turn, and every device operand in turn one alignment class below its contract (4-byte aligned
    where the header asks for 16, an odd address where it asks for 4): the return code is non-zero, rnr_last_error names the
    entry point, every output still holds the sentinel and every guard is intact.  The same call with valid arguments succeeds
    and writes every element."""
    base_id, sizes = REFUSALS[fn]
    check_refusals(fn, base_id, sizes)


def test_ray_weights_refuses_rows_too_wide_for_lds():
    """rnr_ray_weights checks its LDS need as rnr_ray_render does: 32 * (staged floats + c_w) floats must fit 64 KiB."""
    from rnr_amd import _lib
    s = gc.ray_scene('npix1')
    args = gc.ray_args('rnr_ray_weights', s)
    args['c_w'] = 512
    args['ray_w'] = Out((1, 1, 1, 512))
    ec = EntryCalls(True)
    assert ec.call('rnr_ray_weights', check=False, **args) != 0
    assert 'rnr_ray_weights: rows too wide' in _lib.load().rnr_last_error().decode()
    assert holds_sentinel(ec.dev['ray_w'])
    args['c_w'] = 480
    args['ray_w'] = Out((1, 1, 1, 480))
    assert EntryCalls(True).call('rnr_ray_weights', check=False, **args) == 0
