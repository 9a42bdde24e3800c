"""-m gpu: the extension kernels of include/rnr_hip.h section 1 and rnr_project_vertices with per-view optional arguments,
at ragged sizes and on inputs no rasterized scene produces, against oracle/raster_ext64.py (pinned to the C oracle by
tests/test_raster_ext_cpu.py).

1. rnr_backward_textures / rnr_backward_depth_map (float atomics; the depth kernel pre-reduces per wave, keyed by view and
   face).  The index maps are the lane patterns of raster_ext64.face_patterns at (B, S) = (1,5) (3,5) (2,37) (3,50) (1,64):
   partial last waves and workgroups, three views inside one wave, and the aligned control.
   EXACT inputs: every term and every sum of any subset of the terms of an entry is a float32 value (proven by the builders),
   so no addition rounds in any order and the result must equal the float64 sum bit for bit — one dropped, doubled or
   misdirected lane changes it.
   GAUSSIAN inputs: the terms t_1 .. t_k of an entry are float32 values (restated one operation at a time in numpy, pinned bit
   for bit to the C oracle); the reference is their float64 sum S.  The kernel adds them in float32 in an order we do not
   know: atomics in any order, and in the depth kernel a butterfly over the wave first, where the lanes that are not members
   of the group contribute exact zeros (x + 0 = x, no rounding).  Whatever the order — any binary tree over the k terms — the
   computed sum satisfies
       |got - S| <= (k - 1) u sum|t_i|,   u = 2^-24
   (each term passes through at most k - 1 roundings of relative size <= u; that the bound holds as written, without
   higher-order terms, is Jeannerod & Rump, SIAM J. Matrix Anal. Appl. 34 (2013)).  k = 1 (and k = 0) ask for bitwise
   equality.  The atomics may flush subnormals: every non-zero term is >= 2^-60 in magnitude (asserted by the builders), so a
   non-zero partial sum is a multiple of 2^-83 and never subnormal.  No measured constant enters.

2. The kernels without atomics are bit-exact against the C oracle on constructed input: the silhouette sweep
   (rnr_backward_pixel_map) on raster_ext64.edge_faces — axis-parallel edges, vertices on pixel centres, an edge inside pixel
   coordinate (-1, 0), faces off every border, zero area, the whole image, back faces over a non-zero pre-fill, 200 sub-pixel
   faces, B * nf odd; rnr_forward_texture_sampling with per-view textures, the upper clamp, weights of exactly 0 and 1, eps = 0
   and sentinel-filled outputs; rnr_load_textures on integer uvs (each coordinate wrapped exactly once), non-square images and a
   mixed is_update; rnr_create_texture_image for face counts on both sides of a tile-grid step over a sentinel-filled atlas.

3. rnr_project_vertices (shade.hip) with K, R, t, distortion, offset and scale that differ per view, against the header's
   formula in float64.  Bound: raster_ext64.project_ref carries a running error analysis through the formula — an operation
   c = a (op) b on operands known to within ea, eb is known to within the propagated error (|b| ea + |a| eb + ea eb for a
   product, ea + eb for a sum, (ea + |c| eb) / (|b| - eb) for a quotient, ea / (sqrt(a) + sqrt(a - ea)) for the root) plus its
   own rounding u (|c| + propagated).  Unrolled, that is the familiar count-the-roundings rule: for a sum of products each
   term is charged u times its magnitude once per float32 rounding on its path to the output (z: 3 products and 3 additions
   -> 6 u sum|v_i R_2i|, |t_2|), and the later stages (division by z, distortion polynomial, K, offset / scale, NDC) pass those
   on through their derivatives.  It holds for any order of the additions inside a sum and needs correctly rounded +, -, *,
   / and sqrt, which the build's -ffp-contract=off and HIP's default correctly rounded division and square root provide.
"""
import numpy as np
import pytest
import torch

from oracle import raster_ext64 as rx

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def bits(a):
    """tests/test_gpu_raster.py: float32 bit patterns with NaNs canonicalised."""
    a = np.ascontiguousarray(a)
    if a.dtype != np.float32:
        return a
    b = a.view(np.uint32).copy()
    b[np.isnan(a)] = 0x7fc00000
    return b


def _t(a, dt=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dt).contiguous()


def _np(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def run_backward_textures(fim, c, nf, ts):
    from rnr_amd import ops
    B = fim.shape[0]
    gt = torch.zeros(B, nf, ts, ts, ts, 3, device=DEV)
    ops.backward_textures(_t(fim, torch.int32), _t(c['sampling_weight_map']), _t(c['sampling_index_map'], torch.int32),
                          _t(c['grad_rgb_map']), gt, nf)
    return _np(gt)


def run_backward_depth(fim, c, init):
    from rnr_amd import ops
    gf = _t(init)
    ops.backward_depth_map(_t(c['faces']), _t(c['depth_map']), _t(fim, torch.int32), _t(c['face_inv_map']),
                           _t(c['weight_map']), _t(c['grad_depth_map']), gf, fim.shape[1])
    return _np(gf)


def assert_within_sum_bound(got, r, what):
    got = got.reshape(-1).astype(np.float64)
    err, bound = np.abs(got - r['S']), rx.sum_bound(r)
    worst = int(np.argmax(err - bound))
    print('%s: max err %.3g, bound there %.3g, k max %d' % (what, err[worst], bound[worst], r['k'].max(initial=0)))
    assert (err <= bound).all(), (what, worst, got[worst], r['S'][worst], bound[worst], int(r['k'][worst]))
    single = r['k'] <= 1
    assert np.array_equal(bits(got[single].astype(np.float32)), bits(r['S'][single].astype(np.float32))), what


# ---------------------------------------------------------------------------------------------------------------------
# 1. accumulating kernels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,S', rx.SIZES)
def test_backward_textures_exact_inputs_bitwise(B, S):
    seen = 0
    for name, nf, fim in rx.face_patterns(B, S):
        for ts in (1, 2, 3):
            c = rx.exact_textures_case(fim, nf, ts, seed=10 * ts + B)
            got = run_backward_textures(fim, c, nf, ts)
            assert np.array_equal(bits(got), bits(c['want'])), (name, ts, int((got != c['want']).sum()))
            k = c['ref64']['k']
            assert (k.sum() > 0) == (name != 'all_background'), name
            if name == 'one_face_everywhere' and ts == 1:
                assert k.max() >= 64
            seen += 1
    assert seen == 3 * len(rx.PATTERN_NAMES)


@pytest.mark.parametrize('B,S', rx.SIZES)
def test_backward_depth_map_exact_inputs_bitwise(B, S):
    """Once into zeros and once on top of small integers (the kernel ADDS).  A view holds S^2 pixels, so the largest group
    of `one_face_everywhere` has k = S^2 contributions: >= 64 (whole waves in one group) from S = 37 on."""
    seen = 0
    for name, nf, fim in rx.face_patterns(B, S):
        for prefill in (False, True):
            c = rx.exact_depth_case(fim, nf, seed=20 + B + S, prefill=prefill)
            got = run_backward_depth(fim, c, c['init'])
            assert np.array_equal(bits(got), bits(c['want'])), (name, prefill, int((got != c['want']).sum()))
            k = c['ref64']['k']
            assert (k.sum() > 0) == (name != 'all_background'), name
            if name == 'one_face_everywhere':
                assert k.max() == S * S and (k.max() >= 64) == (S >= 37)
            if name != 'all_background':
                assert (c['want'] != c['init']).any(), name
            seen += 1
    assert seen == 2 * len(rx.PATTERN_NAMES)


@pytest.mark.parametrize('B,S', rx.SIZES)
def test_backward_textures_gaussian_inputs_within_summation_bound(B, S):
    for name, nf, fim in rx.face_patterns(B, S):
        for ts in (1, 3):
            c = rx.gauss_textures_case(fim, nf, ts, seed=30 * ts + S)
            got = run_backward_textures(fim, c, nf, ts)
            assert (c['ref64']['k'].sum() > 0) == (name != 'all_background'), name
            assert_within_sum_bound(got, c['ref64'], 'textures %s ts=%d' % (name, ts))


@pytest.mark.parametrize('B,S', rx.SIZES)
def test_backward_depth_map_gaussian_inputs_within_summation_bound(B, S):
    for name, nf, fim in rx.face_patterns(B, S):
        c = rx.gauss_depth_case(fim, nf, seed=40 + S)
        got = run_backward_depth(fim, c, np.zeros((B, nf, 3, 3), np.float32))
        assert (c['ref64']['k'].sum() > 0) == (name != 'all_background'), name
        if name == 'distinct_face_per_pixel':
            assert c['ref64']['k'].max() == 1                # every entry bitwise
        assert_within_sum_bound(got, c['ref64'], 'depth %s' % name)


# ---------------------------------------------------------------------------------------------------------------------
# 2. kernels without atomics: bit-exact against the C oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S,B', [(64, 1), (64, 3), (50, 3)])
def test_backward_pixel_map_constructed_geometry_bit_exact(S, B):
    """raster_ext64.edge_faces views (non-vacuity of each case: tests/test_raster_ext_cpu.py, against the oracle alone).
    grad_faces starts from a non-zero pre-fill: rows of back faces keep it, both flags 0 keeps all of it."""
    from rnr_amd import ops
    c = rx.pixel_map_case(S, B, seed=S + B)
    assert (B * c['faces'].shape[1]) % 2 == 1               # the 2 B nf thread grid ends in mid-workgroup
    dev = {k: _t(c[k]) for k in ['faces', 'rgb_map', 'alpha_map', 'grad_rgb_map', 'grad_alpha_map']}
    fim = _t(c['face_index_map'], torch.int32)
    for rr, ra in [(1, 1), (0, 1), (1, 0), (0, 0)]:
        want = rx.pixel_map_want(c, rr, ra)
        gf = _t(c['init'])
        ops.backward_pixel_map(dev['faces'], fim, dev['rgb_map'], dev['alpha_map'], dev['grad_rgb_map'], dev['grad_alpha_map'],
                               gf, S, c['eps'], rr, ra)
        got = _np(gf)
        assert np.array_equal(bits(got), bits(want)), (rr, ra, int((bits(got) != bits(want)).sum()))
        if rr or ra:
            assert (want != c['init']).sum() > 1000
        else:
            assert np.array_equal(got, c['init'])


@pytest.mark.parametrize('S', [37, 64])
@pytest.mark.parametrize('ts', [2, 3, 5])
@pytest.mark.parametrize('eps', [1e-3, 0.0])
def test_forward_texture_sampling_synthetic_maps_bit_exact(S, ts, eps):
    """B = 3 with textures that differ per view; see raster_ext64.texture_sampling_case for why every fetch stays inside
    `textures` also with eps = 0.  Background pixels keep the sentinel the outputs were filled with."""
    from rnr_amd import ops
    c = rx.texture_sampling_case(S, ts, eps, seed=ts)
    want, facts = rx.texture_sampling_want(c)
    assert min(facts['covered'], facts['background']) > 100 and facts['upper_clamped'] > 20
    assert facts['weight_zero'] > 20 and facts['weight_one'] > 10
    B = c['faces'].shape[0]
    rgb = torch.full((B, S, S, 3), float(rx.SENTINEL_F), device=DEV)
    sim = torch.full((B, S, S, 8), int(rx.SENTINEL_I), dtype=torch.int32, device=DEV)
    swm = torch.full((B, S, S, 8), float(rx.SENTINEL_F), device=DEV)
    ops.forward_texture_sampling(_t(c['faces']), _t(c['textures']), _t(c['face_index_map'], torch.int32), _t(c['weight_map']),
                                 _t(c['depth_map']), rgb, sim, swm, S, eps)
    assert np.array_equal(_np(sim), want['sampling_index_map'])
    assert np.array_equal(bits(_np(swm)), bits(want['sampling_weight_map']))
    assert np.array_equal(bits(_np(rgb)), bits(want['rgb_map']))


@pytest.mark.parametrize('ih,iw', [(7, 13), (16, 5)])
@pytest.mark.parametrize('ts', [2, 3, 8])
def test_load_textures_integer_uvs_and_ragged_images_bit_exact(ih, iw, ts):
    """All 4 wrappings x both filters.  Expected values from the C oracle, which wraps each coordinate exactly once (the
    header's rule; tests/test_raster_ext_cpu.py pins its values on the integers).  Faces with is_update = 0 keep uv and cube."""
    from oracle import raster as oras
    from rnr_amd import ops
    c = rx.load_textures_case(ih, iw, ts, seed=ih + ts)
    upd = c['is_update'].astype(bool)
    for wrapping in range(4):
        for bilinear in (False, True):
            want_tex, want_uv = oras.load_textures(c['image'], c['faces'], c['textures'], c['is_update'], wrapping, bilinear)
            uv, tex = _t(c['faces']), _t(c['textures'])
            ops.load_textures(_t(c['image']), uv, tex, _t(c['is_update'], torch.int32), wrapping, bilinear)
            got_uv, got_tex = _np(uv), _np(tex)
            assert np.array_equal(bits(got_uv), bits(want_uv)), (wrapping, bilinear)
            assert np.array_equal(bits(got_tex), bits(want_tex)), (wrapping, bilinear)
            assert np.array_equal(bits(got_uv[~upd]), bits(c['faces'][~upd]))
            assert np.array_equal(bits(got_tex[~upd]), bits(c['textures'][~upd]))
            assert not np.array_equal(got_tex[upd], c['textures'][upd])
            for before, after in zip(c['faces'][0].reshape(-1)[:4], got_uv[0].reshape(-1)[:4]):
                assert after == rx.WRAPPED_ONCE[wrapping][float(before)]


@pytest.mark.parametrize('nf', [1, 2, 4, 5, 16, 17, 40])
def test_create_texture_image_tile_grid_steps_bit_exact(nf):
    from rnr_amd import ops
    for tsi in (2, 4):
        for tile in (4, 8):
            c = rx.create_texture_image_case(nf, tsi, tile, seed=nf + tsi)
            want, beyond = rx.create_texture_image_want(c)
            img = _t(c['image'])
            ops.create_texture_image(_t(c['vertices_all']), _t(c['textures']), img, 1e-5)
            got = _np(img)
            assert np.array_equal(bits(got), bits(want)), (tsi, tile)
            assert (got[beyond] == rx.SENTINEL_F).all() and not (got[~beyond] == rx.SENTINEL_F).any()
            assert beyond.any() == (nf in (5, 17, 40))


def test_create_texture_image_refuses_a_width_off_the_tile_grid():
    from rnr_amd import _lib, ops
    c = rx.create_texture_image_case(5, 2, 4, seed=1)              # 3 tiles a row
    img = torch.zeros(8, 16, 3, device=DEV)
    with pytest.raises(_lib.RnrError, match='image width 16 is not a multiple of the tile count 3'):
        ops.create_texture_image(_t(c['vertices_all']), _t(c['textures']), img, 1e-5)
    assert (_np(img) == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# 3. projection with per-view optional arguments
# ---------------------------------------------------------------------------------------------------------------------
def _opt(c, form):
    d = c['dist_coeffs'] if form != 'plain' else None
    o, s = (c['offset'], c['scale']) if form == 'all' else (None, None)
    return d, o, s


def _dev_or_none(x):
    return None if x is None else _t(x)


def assert_within_projection_bound(got, ref, bound, what):
    err = np.abs(got.astype(np.float64) - ref)
    worst = np.unravel_index(int(np.argmax(err - bound)), err.shape)
    print('%s: max err / bound %.3f, bound max %.3g' % (what, (err / bound).max(), bound.max()))
    assert (err <= bound).all(), (what, worst, err[worst], bound[worst])


@pytest.mark.parametrize('form', ['plain', 'dist', 'all'])
def test_project_vertices_per_view_arguments_within_running_error_bound(form):
    from rnr_amd import ops
    c = rx.projection_case(seed=4)
    d, o, s = _opt(c, form)
    ref, bound = rx.project_ref(c['vertices'], c['K'], c['R'], c['t'], c['orig_size'], d, o, s)
    got = _np(ops.project_vertices(_t(c['vertices']), _t(c['K']), _t(c['R']), _t(c['t']), c['orig_size'], _dev_or_none(d),
                                   _dev_or_none(o), _dev_or_none(s)))
    assert got.shape == (3, 300, 3) and bound.max() < 2e-5
    assert_within_projection_bound(got, ref, bound, form)


def test_projection_broadcast_forms_within_running_error_bound():
    """neural_renderer.projection: one distortion row for three views, a shared mesh [1,nv,3] and per-view meshes [N,nv,3]."""
    import neural_renderer as nr
    c = rx.projection_case(seed=5)
    K, R, t = _t(c['K']), _t(c['R']), _t(c['t'][:, None, :])
    o, s = _t(c['offset']), _t(c['scale'])
    d1 = c['dist_coeffs'][1:2]
    for verts, tag in [(c['vertices'][None], 'shared mesh'), (c['vertices_per_view'], 'per-view meshes')]:
        ref, bound = rx.project_ref(verts if verts.shape[0] > 1 else verts[0], c['K'], c['R'], c['t'], c['orig_size'],
                                    np.repeat(d1, 3, 0), c['offset'], c['scale'])
        got = _np(nr.projection(_t(verts), K, R, t, _t(d1), c['orig_size'], o, s))
        assert got.shape == (3, 300, 3)
        assert_within_projection_bound(got, ref, bound, tag + ', [1,5] distortion')
        ref, bound = rx.project_ref(verts if verts.shape[0] > 1 else verts[0], c['K'], c['R'], c['t'], c['orig_size'],
                                    c['dist_coeffs'])
        got = _np(nr.projection(_t(verts), K, R, t, _t(c['dist_coeffs']), c['orig_size']))
        assert_within_projection_bound(got, ref, bound, tag + ', [N,5] distortion')


def test_project_vertices_refuses_arguments_that_are_not_per_view():
    """A [1,5] dist_coeffs (or any per-view argument with another leading dimension) with N = 3 would be read out of bounds."""
    from rnr_amd import ops
    c = rx.projection_case(seed=4)
    a = {k: _t(c[k]) for k in ['vertices', 'K', 'R', 't', 'dist_coeffs', 'offset', 'scale']}
    call = lambda **kw: ops.project_vertices(a['vertices'], a['K'], kw.get('R', a['R']), kw.get('t', a['t']), 256,
                                             kw.get('dist_coeffs', a['dist_coeffs']), kw.get('offset', a['offset']),
                                             kw.get('scale', a['scale']))
    for name in ['R', 't', 'dist_coeffs', 'offset', 'scale']:
        with pytest.raises(ValueError, match='project_vertices: %s must hold' % name):
            call(**{name: a[name][:1].contiguous()})
        with pytest.raises(ValueError, match='project_vertices: %s must hold' % name):
            call(**{name: torch.cat([a[name], a[name][:1]]).contiguous()})
    assert call().shape == (3, 300, 3)
