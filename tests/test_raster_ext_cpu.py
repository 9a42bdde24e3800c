"""Pins oracle/raster_ext64.py (the references and input builders of tests/test_gpu_raster_ext_sweep.py) to the C oracle
oracle/raster_oracle.c, which tests/test_oracle_golden.py pins to the reference's own fixtures.  CPU only.

  * the numpy float32 restatements of the per-pixel terms of backward_textures / backward_depth_map, added one by one in
    pixel order, reproduce the C oracle's accumulation BIT FOR BIT (a recorded soup and two lane patterns);
  * the exact-input builders prove their own exactness (asserts inside the builders) and their float64 sums, cast to
    float32, equal the C oracle's serial float32 sums bit for bit;
  * every lane pattern, constructed geometry and synthetic map states its non-vacuity condition, computed from the
    reference alone;
  * the float64 projection reference carries a bound that holds for the project's float32 CPU oracle and is tight enough to
    see a swapped offset component.
"""
import numpy as np
import pytest
import torch

from oracle import raster as oras
from oracle import raster_ext64 as rx
from oracle import rnr_oracle as orc


def bits(a):
    a = np.ascontiguousarray(a)
    if a.dtype != np.float32:
        return a
    b = a.view(np.uint32).copy()
    b[np.isnan(a)] = 0x7fc00000
    return b


# ---------------------------------------------------------------------------------------------------------------------
# lane patterns
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,S', rx.SIZES)
def test_face_patterns_are_what_their_names_say(B, S):
    pats = {name: (nf, m) for name, nf, m in rx.face_patterns(B, S)}
    assert list(pats) == rx.PATTERN_NAMES
    P = S * S
    for name, (nf, m) in pats.items():
        cov = int((m >= 0).sum())
        assert (cov == 0) == (name == 'all_background'), name
    nf, m = pats['one_face_everywhere']
    assert (m == m.flat[0]).all() and P >= 25
    nf, m = pats['distinct_face_per_pixel']
    assert nf == P and all(len(np.unique(m[b])) == P for b in range(B))
    assert len(np.unique(pats['alternating_two'][1])) == 2
    flat = pats['runs_of_three'][1].reshape(-1)
    assert (flat[0::3][:len(flat) // 3] == flat[2::3][:len(flat) // 3]).all() and (flat[:-3] != flat[3:]).all()
    assert len(np.unique(pats['random_of_seven'][1])) == 7 or B * P < 40
    m = pats['only_last_pixel'][1]
    assert int((m >= 0).sum()) == 1 and m.reshape(-1)[-1] >= 0
    m = pats['same_face_id_in_every_view'][1]
    assert all(np.array_equal(m[b], m[0]) for b in range(B)) and m[0].flat[0] == m[0].flat[-1] == 1 and (m == -1).any()
    # ragged sizes: the last wave / workgroup is partial, and at (3, 5) one wave holds pixels of three views
    assert ((B * P) % 64 != 0) == ((B, S) != (1, 64))


# ---------------------------------------------------------------------------------------------------------------------
# term restatements == C oracle accumulations, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
def _check_terms_against_c(fim, nf, ts, tex_in, dep_in):
    B = fim.shape[0]
    e, t = rx.textures_terms(fim, tex_in['sampling_weight_map'], tex_in['sampling_index_map'], tex_in['grad_rgb_map'], nf, ts)
    seq = rx.sequential32(e, t, B * nf * ts ** 3 * 3)
    want = oras.backward_textures(fim, tex_in['sampling_weight_map'], tex_in['sampling_index_map'], tex_in['grad_rgb_map'], nf, ts)
    assert np.array_equal(bits(seq), bits(want.reshape(-1)))
    S = fim.shape[1]
    e, t = rx.depth_terms(dep_in['faces'], dep_in['depth_map'], fim, dep_in['face_inv_map'], dep_in['weight_map'],
                          dep_in['grad_depth_map'])
    seq = rx.sequential32(e, t, B * nf * 9)
    want = oras.backward_depth_map(dep_in['faces'], dep_in['depth_map'], fim, dep_in['face_inv_map'], dep_in['weight_map'],
                                   dep_in['grad_depth_map'], S)
    assert np.array_equal(bits(seq), bits(want.reshape(-1)))
    assert (want != 0).any()


def test_terms_reproduce_c_oracle_on_recorded_soup(golden):
    g = golden('raster_bwd_soup48')
    fim = g['face_index_map']
    _check_terms_against_c(fim, g['faces'].shape[1], int(g['texture_size']), g, g)
    assert (fim >= 0).sum() > 100


@pytest.mark.parametrize('B,S,name', [(3, 5, 'same_face_id_in_every_view'), (2, 37, 'random_of_seven'), (1, 64, 'one_face_everywhere')])
def test_terms_reproduce_c_oracle_on_patterns(B, S, name):
    nf, fim = rx.pattern(B, S, name)
    _check_terms_against_c(fim, nf, 3, rx.gauss_textures_case(fim, nf, 3, 5), rx.gauss_depth_case(fim, nf, 6))


# ---------------------------------------------------------------------------------------------------------------------
# exact builders: exactness proven inside, result == the C oracle's serial float32 sum
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,S', rx.SIZES)
def test_exact_builders_prove_exactness_and_match_c_oracle(B, S):
    for name, nf, fim in rx.face_patterns(B, S):
        for ts in (1, 2, 3):
            c = rx.exact_textures_case(fim, nf, ts, seed=ts)
            want = oras.backward_textures(fim, c['sampling_weight_map'], c['sampling_index_map'], c['grad_rgb_map'], nf, ts)
            assert np.array_equal(bits(c['want']), bits(want)), (name, ts)
            k = c['ref64']['k']
            assert (k.sum() > 0) == (name != 'all_background')
            if name == 'one_face_everywhere' and ts == 1:
                assert k.max() >= 64                       # 8 S^2 additions into the one texel of the face
        for prefill in (False, True):
            c = rx.exact_depth_case(fim, nf, seed=7, prefill=prefill)
            want = oras.backward_depth_map(c['faces'], c['depth_map'], fim, c['face_inv_map'], c['weight_map'],
                                           c['grad_depth_map'], S, grad_faces=c['init'])
            assert np.array_equal(bits(c['want']), bits(want)), (name, prefill)
            k = c['ref64']['k']
            if name == 'one_face_everywhere':
                assert k.max() == S * S and (S * S >= 64) == (k.max() >= 64)   # a view's S^2 pixels: >= 64 from S = 37 on
            if name == 'all_background':
                assert np.array_equal(c['want'], c['init'])
            else:
                assert (c['want'] != c['init']).any(), name


def test_gauss_bound_is_zero_for_single_contributions():
    nf, fim = rx.pattern(2, 37, 'distinct_face_per_pixel')
    c = rx.gauss_depth_case(fim, nf, 3)
    r = c['ref64']
    assert r['k'].max() == 1 and (rx.sum_bound(r) == 0).all()
    nf, fim = rx.pattern(1, 64, 'one_face_everywhere')
    r = rx.gauss_depth_case(fim, nf, 3)['ref64']
    assert r['k'].max() == 4096 and 0 < rx.sum_bound(r).max() < 4096 * rx.U32 * r['A'].max() * 1.0001


# ---------------------------------------------------------------------------------------------------------------------
# constructed geometry
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S', [64, 50])
def test_edge_faces_hold_every_feature(S):
    faces, tags = rx.edge_faces(S)
    assert len(faces) % 2 == 1 and np.isfinite(faces).all()
    for tag, n in [('axis_on_centres', 2), ('axis_between', 2), ('lattice', 24), ('edge_in_-1_0', 2), ('partly_off', 4),
                   ('wholly_off', 5), ('zero_area', 3), ('covers_image', 1), ('back', 2), ('subpixel', 200), ('soup', 30)]:
        assert (tags == tag).sum() >= n, tag
    back = rx.is_backface(faces)
    assert back[tags == 'back'].all() and not back[np.isin(tags, ['lattice', 'covers_image', 'zero_area', 'subpixel'])].any()
    pix = 0.5 * (faces[:, :, :2].astype(np.float64) * S + S - 1)
    e = pix[tags == 'edge_in_-1_0']
    assert ((e > -1) & (e < 0)).all(-1).sum() == 0 and sum(((f[:, a] > -1) & (f[:, a] < 0)).sum() == 2 for f in e for a in (0, 1)) == 2
    w = pix[tags == 'wholly_off']
    assert all(((f[:, 0] < -1).all() or (f[:, 0] > S).all() or (f[:, 1] < -1).all() or (f[:, 1] > S).all()) for f in w)
    if S == 64:                                            # pixel centres are exact in float32: vertices sit ON them
        lat = pix[np.isin(tags, ['lattice', 'axis_on_centres'])]
        assert np.array_equal(lat, np.round(lat))
    sub = pix[tags == 'subpixel']
    assert (sub.max(1) - sub.min(1)).max() < 1.0
    # the image-covering face really covers every pixel centre
    r = oras.face_index_map(faces[None][:, tags == 'covers_image'], S, 0.0, 100.0)
    assert (r['face_index_map'] == 0).all()


@pytest.mark.parametrize('S,B', [(64, 1), (64, 3), (50, 3)])
def test_pixel_map_case_is_not_vacuous(S, B):
    """Checked against the oracle alone: each flag pair yields more than 300 non-zero gradient entries (alpha alone: 100), the constructed faces
    (not only the soup) take part, back faces keep the pre-fill, both flags 0 leaves everything."""
    c = rx.pixel_map_case(S, B, seed=S + B)
    assert c['faces'].shape[1] % 2 == 1 and (B * c['faces'].shape[1]) % 2 == 1
    if B > 1:
        assert not np.array_equal(c['faces'][0], c['faces'][1]) and not np.array_equal(c['face_index_map'][0], c['face_index_map'][1])
    cov = (c['face_index_map'] >= 0).mean((1, 2))
    assert all((cov[b] == 1.0) == (B > 1 and b % 2 == 0) for b in range(B)) and cov.min() > 0.3   # views 0, 2 of a batch: covered
    shown = {t for b in range(B) for t in c['tags'][b][np.unique(c['face_index_map'][b][c['face_index_map'][b] >= 0])]}
    assert {'lattice', 'axis_on_centres', 'axis_between', 'partly_off', 'edge_in_-1_0', 'subpixel', 'soup'} <= shown
    assert ('covers_image' in shown) == (B > 1)
    back = rx.is_backface(c['faces']).reshape(B, -1)
    for rr, ra in [(1, 1), (0, 1), (1, 0)]:
        want = rx.pixel_map_want(c, rr, ra)
        raw = oras.backward_pixel_map(c['faces'], c['face_index_map'], c['rgb_map'], c['alpha_map'], c['grad_rgb_map'],
                                      c['grad_alpha_map'], S, c['eps'], rr, ra)
        assert np.array_equal(bits(want[back]), bits(c['init'][back])) and back.sum() >= 2 * B
        assert (raw[back] == 0).all()
        assert ((raw != 0) & ~np.isnan(raw)).sum() > (300 if rr else 100), (rr, ra)
        for tag in ['lattice', 'partly_off', 'edge_in_-1_0', 'axis_between', 'subpixel']:
            assert (raw[c['tags'] == tag] != 0).any(), tag
        assert (want[..., 2][~back] == 0).all()             # z entries of front faces are overwritten with 0
    assert np.array_equal(rx.pixel_map_want(c, 0, 0), c['init'])


# ---------------------------------------------------------------------------------------------------------------------
# synthetic texture-sampling maps
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S', [37, 64])
@pytest.mark.parametrize('ts', [2, 3, 5])
@pytest.mark.parametrize('eps', [1e-3, 0.0])
def test_texture_sampling_case_takes_every_branch(S, ts, eps):
    c = rx.texture_sampling_case(S, ts, eps, seed=ts)
    want, facts = rx.texture_sampling_want(c)
    cov = c['face_index_map'] >= 0
    assert facts['covered'] > 100 and facts['background'] > 100
    assert facts['upper_clamped'] > 20 and facts['weight_zero'] > 20 and facts['weight_one'] > 10
    assert (want['rgb_map'][~cov] == rx.SENTINEL_F).all() and (want['sampling_index_map'][~cov] == rx.SENTINEL_I).all()
    assert (want['sampling_weight_map'][~cov] == rx.SENTINEL_F).all()
    assert not (want['rgb_map'][cov] == rx.SENTINEL_F).any()
    # the wrapper of oracle/raster.py computes the same on the covered pixels
    ref = oras.texture_sampling(c['faces'], c['textures'], c['face_index_map'], c['weight_map'], c['depth_map'], S, eps)
    for k in want:
        assert np.array_equal(bits(want[k][cov]), bits(ref[k][cov])), k
    # per-view textures matter: view 1 sampled from view 0's cubes gives another image
    other = dict(c, textures=np.roll(c['textures'], 1, 0))
    assert not np.array_equal(rx.texture_sampling_want(other)[0]['rgb_map'], want['rgb_map'])
    if eps == 0.0:        # a coordinate clamped to exactly ts - 1 selects corner ts with weight 0 (see the builder)
        assert want['sampling_index_map'][cov].max() >= ts ** 3


# ---------------------------------------------------------------------------------------------------------------------
# load_textures / create_texture_image
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('wrapping', [0, 1, 2, 3])
def test_integer_uvs_are_wrapped_exactly_once(wrapping):
    """The header's rule.  REPEAT is the mode in which a second wrap would show (1 -> 0 -> 1): there the values below are
    NOT a fixed point of the wrap.  MIRRORED_REPEAT and CLAMP_TO_EDGE map [0, 1] onto itself pointwise, so wrapping their
    result again changes nothing — on these integers, on the builder's coordinates, and on every float32 value."""
    c = rx.load_textures_case(7, 13, 3, seed=1)
    assert all(v in c['faces'][0].reshape(-1) for v in rx.INTEGER_UVS) and c['is_update'][0] == 1
    assert all(v in c['faces'][1].reshape(-1) for v in rx.INTEGER_UVS) and c['is_update'][1] == 0
    tex, uv = oras.load_textures(c['image'], c['faces'], c['textures'], c['is_update'], wrapping, True)
    upd = c['is_update'].astype(bool)
    for before, after in zip(c['faces'][upd].reshape(-1), uv[upd].reshape(-1)):
        if float(before) in rx.WRAPPED_ONCE[wrapping]:
            assert after == rx.WRAPPED_ONCE[wrapping][float(before)], (before, after)
    assert np.array_equal(bits(uv[~upd]), bits(c['faces'][~upd])) and np.array_equal(bits(tex[~upd]), bits(c['textures'][~upd]))
    assert (~upd).sum() > 3 and upd.sum() > 10
    if wrapping != 3:
        assert uv[upd].min() >= 0 and uv[upd].max() <= 1          # every fetch lands inside the image
        assert not np.array_equal(tex[upd], c['textures'][upd])
    else:
        assert (tex[upd] == 0).all() and np.array_equal(bits(uv), bits(c['faces']))
    _, uv2 = oras.load_textures(c['image'], uv, c['textures'], c['is_update'], wrapping, True)
    assert np.array_equal(bits(uv2), bits(uv)) == (wrapping != 0)


@pytest.mark.parametrize('nf', [1, 2, 4, 5, 16, 17, 40])
def test_texture_atlas_case_leaves_tiles_beyond_the_last_face(nf):
    for tsi, tile in [(2, 4), (4, 8)]:
        c = rx.create_texture_image_case(nf, tsi, tile, seed=nf)
        want, beyond = rx.create_texture_image_want(c)
        assert want.shape[1] == c['per_row'] * tile and want.shape[0] == c['rows'] * tile
        assert (c['per_row'] - 1) ** 2 < nf <= c['per_row'] ** 2
        assert (want[beyond] == rx.SENTINEL_F).all() and not (want[~beyond] == rx.SENTINEL_F).any()
        assert beyond.any() == (nf in (5, 17, 40))       # 6, 20, 42 tiles; 1, 2, 4, 16 fill their grids
        ref = oras.create_texture_image(c['vertices_all'], c['textures'], want.shape[:2], 1e-5)
        assert np.array_equal(bits(ref[~beyond]), bits(want[~beyond]))


# ---------------------------------------------------------------------------------------------------------------------
# projection reference
# ---------------------------------------------------------------------------------------------------------------------
def _opt(c, form):
    d = c['dist_coeffs'] if form != 'plain' else None
    o, s = (c['offset'], c['scale']) if form == 'all' else (None, None)
    return d, o, s


@pytest.mark.parametrize('form', ['plain', 'dist', 'all'])
def test_project_ref_bound_holds_for_float32_cpu_oracle_and_sees_a_swapped_offset(form):
    c = rx.projection_case(seed=4)
    d, o, s = _opt(c, form)
    ref, bound = rx.project_ref(c['vertices'], c['K'], c['R'], c['t'], c['orig_size'], d, o, s)
    T = lambda x: None if x is None else torch.from_numpy(x)
    got = orc.projection(T(c['vertices'])[None], T(c['K']), T(c['R']), T(c['t'])[:, None, :],
                         T(d) if d is not None else torch.zeros(3, 5), c['orig_size'], T(o), T(s)).numpy()
    assert (np.abs(got - ref) <= bound).all()
    assert bound.max() < 2e-5 and bound[..., 2].max() < 3e-6       # a handful of ulps of outputs of size ~1 resp. ~4
    assert np.abs(ref[..., :2]).max() < 8 and ref[..., 2].min() >= 0.5
    if form == 'all':
        swapped, _ = rx.project_ref(c['vertices'], c['K'], c['R'], c['t'], c['orig_size'], d, o[:, ::-1], s)
        assert (np.abs(swapped[..., 0] - ref[..., 0]) > 10 * bound[..., 0]).all()
        other_view, _ = rx.project_ref(c['vertices'], c['K'], c['R'], c['t'], c['orig_size'], np.roll(d, 1, 0), o, s)
        assert (np.abs(other_view - ref)[..., :2] > bound[..., :2]).mean() > 0.9
