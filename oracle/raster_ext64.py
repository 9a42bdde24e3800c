"""ORACLE (test infrastructure): references and input builders for the extension kernels of include/rnr_hip.h section 1
(forward_texture_sampling, backward_pixel_map, backward_textures, backward_depth_map, load_textures, create_texture_image)
and for rnr_project_vertices with its per-view optional arguments.  Written from the header's contract; numpy only.
tests/test_raster_ext_cpu.py pins every helper here to oracle/raster_oracle.c, tests/test_gpu_raster_ext_sweep.py uses them.

Three kinds of reference:
  * the C oracle itself (oracle/raster.py) for the kernels without atomics, which are bit-exact on any input;
  * for the two accumulating kernels, the per-pixel TERMS restated in numpy float32, one operation at a time
    (textures_terms, depth_terms), scattered into the output entries in float64 (scatter64): the sum S of the float32 terms
    per entry, the number k of contributions and the sum of their magnitudes.  On the exact inputs (exact_textures_case,
    exact_depth_case) every term and every sum of any subset of terms is a small dyadic number, so S cast to float32 is
    the one possible result of any summation order; on Gaussian inputs any float32 summation order stays within
    (k - 1) 2^-24 sum|t| of S;
  * for the projection, the header's formula in float64 with a running error bound carried through every operation
    (project_ref).
"""
import ctypes

import numpy as np

from . import raster as oras

U32 = 2.0 ** -24          # unit roundoff of binary32
MIN_TERM = 2.0 ** -60     # Gaussian builders keep every non-zero term above this: far from float32's subnormal range


# =====================================================================================================================
# lane patterns
# =====================================================================================================================
PATTERN_NAMES = ['all_background', 'one_face_everywhere', 'distinct_face_per_pixel', 'alternating_two', 'runs_of_three',
                 'random_of_seven', 'only_last_pixel', 'same_face_id_in_every_view']
SIZES = [(1, 5), (3, 5), (2, 37), (3, 50), (1, 64)]


def face_patterns(B, S, nf=11):
    """Yields (name, nf, face_index_map [B,S,S] int32): synthetic index maps that put chosen lane patterns into the 64-lane
    waves of the per-pixel kernels (pixel i of the flattened [B,S,S] map is lane i % 64 of wave i / 64).  nf >= 7; the
    pattern `distinct_face_per_pixel` has nf = S * S."""
    assert nf >= 7
    P = S * S
    p = np.arange(B * P).reshape(B, S, S)          # global pixel number
    q = p % P                                      # pixel number inside its view
    rng = np.random.default_rng(1000 * B + S)

    def out(name, n, m):
        m = np.ascontiguousarray(m, np.int32)
        assert m.shape == (B, S, S) and m.min() >= -1 and m.max() < n
        return name, n, m
    yield out('all_background', nf, np.full((B, S, S), -1))
    yield out('one_face_everywhere', nf, np.full((B, S, S), 2))                # one group per view a wave touches
    yield out('distinct_face_per_pixel', P, q)                                 # 64 groups a wave
    yield out('alternating_two', nf, np.where(p % 2 == 0, 0, nf - 1))
    yield out('runs_of_three', nf, (p // 3) % nf)
    seven = rng.permutation(nf)[:7]
    yield out('random_of_seven', nf, seven[rng.integers(0, 7, size=(B, S, S))])
    last = np.full((B, S, S), -1)
    last[B - 1, S - 1, S - 1] = nf - 1
    yield out('only_last_pixel', nf, last)
    # face 1 on the first and on the last third of every view, background between: where two views meet (inside one wave
    # when S * S is no multiple of 64) the same face NUMBER continues and must not be summed across the view boundary
    yield out('same_face_id_in_every_view', nf, np.where((q < P // 3 + 1) | (q >= P - P // 3 - 1), 1, -1))


def pattern(B, S, name, nf=11):
    for n, f, m in face_patterns(B, S, nf):
        if n == name:
            return f, m
    raise KeyError(name)


# =====================================================================================================================
# backward_textures: terms, exact and Gaussian inputs
# =====================================================================================================================
def textures_terms(fim, swm, sim, grad_rgb, nf, ts):
    """Contributions of rnr_backward_textures in the C oracle's order (pixel, corner, channel):
    entry = flat index into grad_textures [B,nf,ts,ts,ts,3], term = float32(sampling_weight * grad_rgb), one multiplication."""
    fim = np.asarray(fim, np.int32)
    B, S = fim.shape[:2]
    swm = np.asarray(swm, np.float32).reshape(-1, 8)
    sim = np.asarray(sim, np.int32).reshape(-1, 8)
    g = np.asarray(grad_rgb, np.float32).reshape(-1, 3)
    px = np.flatnonzero(fim.reshape(-1) >= 0)
    cube = ts * ts * ts * 3
    base = ((px // (S * S)) * nf + fim.reshape(-1)[px]).astype(np.int64) * cube
    assert sim[px].min(initial=0) >= 0 and sim[px].max(initial=0) < ts ** 3
    entry = base[:, None, None] + sim[px].astype(np.int64)[:, :, None] * 3 + np.arange(3)[None, None, :]
    term = swm[px][:, :, None] * g[px][:, None, :]
    assert term.dtype == np.float32
    return entry.reshape(-1), term.reshape(-1)


def depth_terms(faces, depth_map, fim, face_inv_map, weight_map, grad_depth_map):
    """Contributions of rnr_backward_depth_map in the C oracle's order (pixel, then the three z entries, then the six x / y
    entries): entry = flat index into grad_faces [B,nf,3,3]; every term is evaluated in float32 one operation at a time in
    the association of the header's reference kernel."""
    f32 = np.float32
    faces = np.asarray(faces, f32)
    fim = np.asarray(fim, np.int32)
    B, nf = faces.shape[:2]
    S = fim.shape[1]
    px = np.flatnonzero(fim.reshape(-1) >= 0)
    face = (px // (S * S)) * nf + fim.reshape(-1)[px]
    z = faces.reshape(-1, 3, 3)[face][:, :, 2]                       # [n,3]
    d = np.asarray(depth_map, f32).reshape(-1)[px]
    w = np.asarray(weight_map, f32).reshape(-1, 3)[px]
    inv = np.asarray(face_inv_map, f32).reshape(-1, 3, 3)[px]        # inv[:, l, k] = face_inv[3 l + k]
    gd = np.asarray(grad_depth_map, f32).reshape(-1)[px]
    d2 = d * d
    gz = ((gd[:, None] * w) * d2[:, None]) / (z * z)                 # g[3k+2]
    tmp = np.zeros((len(px), 2), f32)
    for l in range(3):
        tmp = tmp + (-inv[:, l, :2]) / z[:, l:l + 1]
    gxy = (((((-gd)[:, None, None] * tmp[:, None, :]) * w[:, :, None]) * d2[:, None, None]) * f32(S)) / f32(2.0)   # g[3k+l]
    for a in (gz, tmp, gxy):
        assert a.dtype == f32
    k3 = np.arange(3)
    entry = np.concatenate([np.broadcast_to(3 * k3 + 2, (len(px), 3)),
                            np.broadcast_to((3 * k3[:, None] + np.arange(2)[None, :]).reshape(-1), (len(px), 6))], 1)
    entry = face.astype(np.int64)[:, None] * 9 + entry
    term = np.concatenate([gz, gxy.reshape(-1, 6)], 1)
    return entry.reshape(-1), term.reshape(-1)


def sequential32(entry, term, size, init=None):
    """The terms added one by one in float32, in the given order: what a serial loop over the pixels computes."""
    acc = np.zeros(size, np.float32) if init is None else np.asarray(init, np.float32).reshape(-1).copy()
    np.add.at(acc, entry, np.asarray(term, np.float32))
    return acc


def scatter64(entry, term, size):
    """Per output entry: S = float64 sum of the float32 terms, k = their number, A = float64 sum of their magnitudes,
    (P, N) = float64 sums of the positive terms and of the magnitudes of the negative ones."""
    t = np.asarray(term, np.float32).astype(np.float64)
    r = {'S': np.zeros(size), 'k': np.zeros(size, np.int64), 'A': np.zeros(size), 'P': np.zeros(size), 'N': np.zeros(size)}
    np.add.at(r['S'], entry, t)
    np.add.at(r['k'], entry, 1)
    np.add.at(r['A'], entry, np.abs(t))
    np.add.at(r['P'], entry, np.maximum(t, 0.0))
    np.add.at(r['N'], entry, np.maximum(-t, 0.0))
    return r


def sum_bound(r):
    """|any float32 summation order - S| <= (k - 1) 2^-24 sum|t| per entry (module docstring of the GPU sweep)."""
    return np.maximum(r['k'] - 1, 0) * U32 * r['A']


def assert_exact(term, r, quantum, init=None):
    """Proof that the case is exact in float32 in ANY summation order: every term is a multiple of `quantum` (a power of
    two), and every partial sum — a sum over some subset of the terms of an entry, plus the pre-fill — is bounded by
    max(P, N) + |init|, which stays below 2^24 quanta.  A multiple of 2^-q below 2^(24 - q) in magnitude is a float32 value, so
    no addition ever rounds and S cast to float32 is the one possible result."""
    t = np.asarray(term, np.float32).astype(np.float64)
    assert np.array_equal(np.round(t / quantum) * quantum, t), 'a term is no multiple of the quantum'
    top = np.maximum(r['P'], r['N']) + (0.0 if init is None else np.abs(np.asarray(init, np.float64).reshape(-1)))
    assert top.max(initial=0.0) < 2.0 ** 24 * quantum, 'a partial sum could leave the exact range: %g' % top.max()
    total = r['S'] + (0.0 if init is None else np.asarray(init, np.float64).reshape(-1))
    assert np.array_equal(total.astype(np.float32).astype(np.float64), total)


def _force_repeats(sim, rng):
    """Every third pixel, and the very last one (the only one `only_last_pixel` shows), adds three times into one texel."""
    s = sim.reshape(-1, 8)
    rep = np.zeros(len(s), bool)
    rep[::3] = True
    rep[-1] = True
    s[rep, 1] = s[rep, 0]
    s[rep, 5] = s[rep, 0]
    return sim


def exact_textures_case(fim, nf, ts, seed):
    """sampling weights multiples of 1/8 in [0,1], grad_rgb integers in [-4,4], indices random in [0, ts^3) with repeats
    inside a pixel: products are multiples of 1/8 with |t| <= 4.  Returns the inputs, the float64 reference and proves
    exactness (assert_exact)."""
    rng = np.random.default_rng(seed)
    B, S = fim.shape[:2]
    swm = (rng.integers(0, 9, size=(B, S, S, 8)) / 8.0).astype(np.float32)
    g = rng.integers(-4, 5, size=(B, S, S, 3)).astype(np.float32)
    sim = _force_repeats(rng.integers(0, ts ** 3, size=(B, S, S, 8)).astype(np.int32), rng)
    size = B * nf * ts ** 3 * 3
    entry, term = textures_terms(fim, swm, sim, g, nf, ts)
    r = scatter64(entry, term, size)
    assert_exact(term, r, 1.0 / 8)
    cov = fim.reshape(-1) >= 0
    if cov.any():
        s = sim.reshape(-1, 8)[cov]
        assert (np.sort(s, 1)[:, 1:] == np.sort(s, 1)[:, :-1]).any(), 'no pixel adds twice into one texel'
    return {'sampling_weight_map': swm, 'grad_rgb_map': g, 'sampling_index_map': sim, 'ref64': r,
            'want': r['S'].astype(np.float32).reshape(B, nf, ts, ts, ts, 3)}


def gauss_textures_case(fim, nf, ts, seed):
    rng = np.random.default_rng(seed)
    B, S = fim.shape[:2]
    swm = _floor_mag(rng.normal(size=(B, S, S, 8)))
    g = _floor_mag(rng.normal(size=(B, S, S, 3)))
    sim = _force_repeats(rng.integers(0, ts ** 3, size=(B, S, S, 8)).astype(np.int32), rng)
    entry, term = textures_terms(fim, swm, sim, g, nf, ts)
    assert_no_tiny(term)
    return {'sampling_weight_map': swm, 'grad_rgb_map': g, 'sampling_index_map': sim,
            'ref64': scatter64(entry, term, B * nf * ts ** 3 * 3), 'terms': (entry, term)}


def _floor_mag(x, floor=2.0 ** -8):
    """Gaussian values pushed away from zero (|x| >= 2^-8): products of a handful of them stay far above 2^-60."""
    x = np.asarray(x, np.float64)
    return np.where(np.abs(x) < floor, np.copysign(floor, x), x).astype(np.float32)


def assert_no_tiny(term):
    t = np.abs(np.asarray(term, np.float32).astype(np.float64))
    assert not ((t != 0) & (t < MIN_TERM)).any(), 'a non-zero term below 2^-60: a flushing atomic could drop it'
    assert np.isfinite(t).all()


# =====================================================================================================================
# backward_depth_map: exact and Gaussian inputs
# =====================================================================================================================
def exact_depth_case(fim, nf, seed, prefill=False):
    """z in {1,2,4}, depth in {1,2}, weights multiples of 1/4 (barycentric: they sum to 1), face_inv integers in [-2,2],
    grad_depth integers in [-3,3]: gd w d^2 / z^2 is a multiple of 1/64, tmp = -sum inv / z a multiple of 1/4, and
    -gd tmp w d^2 S / 2 a multiple of 1/32; every intermediate is a small dyadic number (checked: the float32 terms equal
    the same expressions in float64).  prefill: grad_faces starts from small integers instead of zeros."""
    rng = np.random.default_rng(seed)
    B, S = fim.shape[:2]
    faces = rng.normal(size=(B, nf, 3, 3)).astype(np.float32)            # x, y are not read by the kernel
    faces[..., 2] = rng.choice(np.array([1.0, 2.0, 4.0], np.float32), size=(B, nf, 3))
    dm = rng.choice(np.array([1.0, 2.0], np.float32), size=(B, S, S))
    a = rng.integers(0, 5, size=(B, S, S))
    b = rng.integers(0, 5, size=(B, S, S)) * (4 - a) // 4
    wm = (np.stack([a, b, 4 - a - b], -1) / 4.0).astype(np.float32)
    assert wm.min() >= 0 and np.array_equal(wm.sum(-1), np.ones((B, S, S), np.float32))
    fivm = rng.integers(-2, 3, size=(B, S, S, 3, 3)).astype(np.float32)
    gd = rng.integers(-3, 4, size=(B, S, S)).astype(np.float32)
    init = rng.integers(-5, 6, size=(B, nf, 3, 3)).astype(np.float32) if prefill else np.zeros((B, nf, 3, 3), np.float32)
    entry, term = depth_terms(faces, dm, fim, fivm, wm, gd)
    e64, t64 = _depth_terms64(faces, dm, fim, fivm, wm, gd)
    assert np.array_equal(entry, e64) and np.array_equal(term.astype(np.float64), t64), 'a per-pixel term rounds in float32'
    r = scatter64(entry, term, B * nf * 9)
    assert_exact(term, r, 1.0 / 64, init)
    want = (r['S'] + init.reshape(-1)).astype(np.float32).reshape(B, nf, 3, 3)
    return {'faces': faces, 'depth_map': dm, 'weight_map': wm, 'face_inv_map': fivm, 'grad_depth_map': gd, 'init': init,
            'ref64': r, 'want': want}


def _depth_terms64(faces, dm, fim, fivm, wm, gd):
    """depth_terms in float64 (same expressions): equal to the float32 terms iff no float32 operation rounded."""
    faces = np.asarray(faces, np.float64)
    B, nf = faces.shape[:2]
    S = fim.shape[1]
    px = np.flatnonzero(fim.reshape(-1) >= 0)
    face = (px // (S * S)) * nf + fim.reshape(-1)[px]
    z = faces.reshape(-1, 3, 3)[face][:, :, 2]
    d2 = np.asarray(dm, np.float64).reshape(-1)[px] ** 2
    w = np.asarray(wm, np.float64).reshape(-1, 3)[px]
    inv = np.asarray(fivm, np.float64).reshape(-1, 3, 3)[px]
    g = np.asarray(gd, np.float64).reshape(-1)[px]
    gz = g[:, None] * w * d2[:, None] / (z * z)
    tmp = -(inv[:, :, :2] / z[:, :, None]).sum(1)
    gxy = -g[:, None, None] * tmp[:, None, :] * w[:, :, None] * d2[:, None, None] * S / 2.0
    k3 = np.arange(3)
    e = np.concatenate([np.broadcast_to(3 * k3 + 2, (len(px), 3)),
                        np.broadcast_to((3 * k3[:, None] + np.arange(2)[None, :]).reshape(-1), (len(px), 6))], 1)
    return (face.astype(np.int64)[:, None] * 9 + e).reshape(-1), np.concatenate([gz, gxy.reshape(-1, 6)], 1).reshape(-1)


def gauss_depth_case(fim, nf, seed):
    rng = np.random.default_rng(seed)
    B, S = fim.shape[:2]
    faces = rng.normal(size=(B, nf, 3, 3)).astype(np.float32)
    faces[..., 2] = rng.uniform(0.5, 4.0, size=(B, nf, 3))
    dm = rng.uniform(0.5, 4.0, size=(B, S, S)).astype(np.float32)
    wm = _floor_mag(np.abs(rng.normal(size=(B, S, S, 3))))
    fivm = _floor_mag(rng.normal(size=(B, S, S, 3, 3)))
    gd = _floor_mag(rng.normal(size=(B, S, S)))
    entry, term = depth_terms(faces, dm, fim, fivm, wm, gd)
    assert_no_tiny(term)
    return {'faces': faces, 'depth_map': dm, 'weight_map': wm, 'face_inv_map': fivm, 'grad_depth_map': gd,
            'ref64': scatter64(entry, term, B * nf * 9), 'terms': (entry, term)}


# =====================================================================================================================
# constructed geometry for the silhouette sweep
# =====================================================================================================================
def pix_to_ndc(p, S):
    """Pixel-index coordinate -> NDC, the inverse of 0.5 (c S + S - 1); exact for integers when S is a power of two."""
    return ((2.0 * np.asarray(p, np.float64) + 1.0 - S) / S).astype(np.float32)


def is_backface(f):
    f = np.asarray(f, np.float32).reshape(-1, 9)
    return (f[:, 7] - f[:, 1]) * (f[:, 3] - f[:, 0]) < (f[:, 4] - f[:, 1]) * (f[:, 6] - f[:, 0])


def edge_faces(S, seed=0, shift=(0, 0), cover=True):
    """-> (faces [nf,3,3] float32 (x_ndc, y_ndc, z), tags [nf] of str), nf odd.  Faces are laid out in pixel-index
    coordinates on a 64-pixel design grid, scaled by S / 64 in whole-pixel steps where the feature needs pixel centres,
    converted to NDC.  `shift` (whole pixels) moves the constructed faces, `seed` changes the soup: views that differ.  cover = False moves the
    image-covering face off the screen (behind it every alpha is 1 and the alpha map has no gradient)."""
    rng = np.random.default_rng(seed)
    k = S / 64.0
    sx, sy = shift
    tris, tags = [], []

    def add(tag, pts, z, front=True, snap=False):
        pts = np.asarray(pts, np.float64) * k
        if snap:
            pts = np.round(pts)
        pts = pts + np.array([sx, sy], np.float64)
        f = np.zeros((3, 3), np.float32)
        f[:, :2] = pix_to_ndc(pts, S)
        f[:, 2] = z
        if bool(is_backface(f)[0]) == front and not (f[0, :2] == f[1, :2]).all():
            f[[1, 2]] = f[[2, 1]]
        tris.append(f)
        tags.append(tag)

    z = lambda: rng.uniform(1.0, 3.0, size=3)
    # axis-parallel edges: on pixel centres (the crossing is inf * 0 = NaN there) and between them (empty d0 range)
    add('axis_on_centres', [(10, 8), (25, 8), (10, 30)], z(), snap=True)
    add('axis_on_centres', [(40, 50), (40, 30), (58, 50)], z(), snap=True)
    add('axis_between', [(10.5, 40.5), (22.5, 40.5), (10.5, 55.5)], z())
    add('axis_between', [(30.25, 5.5), (30.25, 20.75), (18.5, 20.75)], z())
    # vertices on pixel centres, rational slopes: at the vertex column / row the crossing is the vertex itself (off == 0)
    for i in range(24):
        a = np.array([rng.integers(4, 60), rng.integers(4, 60)])
        d1 = np.array([[8, 4], [4, 8], [6, 3], [2, 8], [8, 8], [-8, 4]][i % 6])
        d2 = np.array([[2, 10], [-6, 2], [-3, 6], [-8, 2], [-4, 4], [-2, -8]][i % 6])
        add('lattice', [a, a + d1, a + d2], rng.uniform(0.3, 0.9, size=3), snap=True)
    # an edge wholly inside pixel coordinate (-1, 0), in x and in y
    add('edge_in_-1_0', [(-0.7, 10.2), (-0.3, 14.9), (12.3, 12.1)], z())
    add('edge_in_-1_0', [(20.2, -0.6), (27.9, -0.2), (24.1, 9.3)], z())
    # partly and wholly off each border
    add('partly_off', [(-9.3, 20.1), (6.2, 17.4), (3.1, 31.8)], z())
    add('partly_off', [(58.4, 22.2), (75.7, 25.1), (60.3, 36.9)], z())
    add('partly_off', [(30.2, -8.8), (44.6, -3.1), (37.5, 7.7)], z())
    add('partly_off', [(12.9, 57.3), (28.8, 60.2), (20.1, 77.4)], z())
    add('wholly_off', [(-30.5, 10.2), (-12.1, 14.4), (-20.7, 33.3)], z())
    add('wholly_off', [(70.5, 40.2), (95.1, 44.4), (80.7, 60.3)], z())
    add('wholly_off', [(20.5, -40.2), (41.1, -34.4), (30.7, -11.3)], z())
    add('wholly_off', [(10.5, 70.2), (31.1, 74.4), (20.7, 99.3)], z())
    add('wholly_off', [(-5000.0, -4000.0), (-4000.0, -4500.0), (-4500.0, -3000.0)], z())
    # zero area: collinear on pixel centres, two coincident vertices, all three coincident
    add('zero_area', [(5, 5), (10, 10), (15, 15)], z(), snap=True)
    add('zero_area', [(33, 12), (33, 12), (47, 19)], z(), snap=True)
    add('zero_area', [(50.5, 50.5), (50.5, 50.5), (50.5, 50.5)], z())
    # the whole image, behind everything
    if cover:
        add('covers_image', [(-40.0, -30.0), (200.0, -30.0), (-40.0, 210.0)], [9.0, 9.5, 10.0])
    else:
        add('wholly_off', [(-400.0, -30.0), (-200.0, -30.0), (-400.0, 210.0)], [9.0, 9.5, 10.0])
    # back faces (their grad_faces rows keep the caller's fill)
    add('back', [(12.2, 12.4), (30.9, 15.1), (18.3, 33.6)], z(), front=False)
    add('back', [(40, 10), (52, 22), (44, 28)], z(), front=False, snap=True)
    # 200 faces smaller than a pixel
    c = rng.uniform(1.0, 62.0, size=(200, 1, 2))
    for i in range(200):
        add('subpixel', c[i] + rng.uniform(-0.45, 0.45, size=(3, 2)), z())
    # a small soup between them
    n_soup = 30 if len(tris) % 2 else 31
    for i in range(n_soup):
        ctr = rng.uniform(-5.0, 69.0, size=(1, 2))
        add('soup', ctr + rng.uniform(-14.0, 14.0, size=(3, 2)), rng.uniform(0.5, 6.0, size=3), front=bool(i % 5))
    order = rng.permutation(len(tris))
    faces = np.stack(tris)[order]
    tags = np.array(tags)[order]
    assert len(faces) % 2 == 1
    return faces, tags


def pixel_map_case(S, B, seed, eps=1e-3, ts=2):
    """Forward maps of `edge_faces` views from the C oracle (index map, texture sampling), random loss gradients, a non-zero
    grad_faces pre-fill.  Everything rnr_backward_pixel_map reads, plus the oracle's result for the three flag pairs."""
    rng = np.random.default_rng(seed)
    # the image-covering face is there in views 0 and 2 of a batch; a lone view goes without (see edge_faces)
    views = [edge_faces(S, seed=seed * 10 + b, shift=(3 * b, 2 * b), cover=(B > 1 and b % 2 == 0)) for b in range(B)]
    faces = np.stack([v[0] for v in views])
    tags = np.stack([v[1] for v in views])
    nf = faces.shape[1]
    r = oras.face_index_map(faces, S, 0.0, 100.0)
    tex = rng.uniform(0, 1, size=(B, nf, ts, ts, ts, 3)).astype(np.float32)
    t = oras.texture_sampling(faces, tex, r['face_index_map'], r['weight_map'], r['depth_map'], S, eps)
    alpha = (r['face_index_map'] >= 0).astype(np.float32)
    c = {'faces': faces, 'tags': tags, 'image_size': S, 'eps': eps, 'face_index_map': r['face_index_map'],
         'rgb_map': t['rgb_map'] * alpha[..., None], 'alpha_map': alpha,
         'grad_rgb_map': rng.normal(size=(B, S, S, 3)).astype(np.float32),
         'grad_alpha_map': rng.normal(size=(B, S, S)).astype(np.float32),
         'init': rng.integers(1, 6, size=(B, nf, 3, 3)).astype(np.float32)}
    return c


def pixel_map_want(c, return_rgb, return_alpha):
    """The oracle's grad_faces on top of the case's pre-fill: rows of back faces (and every row when both flags are 0) keep it."""
    g = oras.backward_pixel_map(c['faces'], c['face_index_map'], c['rgb_map'], c['alpha_map'], c['grad_rgb_map'],
                                c['grad_alpha_map'], c['image_size'], c['eps'], return_rgb, return_alpha)
    keep = is_backface(c['faces']).reshape(c['faces'].shape[:2])
    if not return_rgb and not return_alpha:
        keep[:] = True
    return np.where(keep[..., None, None], c['init'], g)


# =====================================================================================================================
# forward_texture_sampling
# =====================================================================================================================
SENTINEL_F = np.float32(-77.25)
SENTINEL_I = np.int32(-12345)


def texture_sampling_case(S, ts, eps, seed, B=3, nf=13):
    """Synthetic maps for rnr_forward_texture_sampling: textures that differ per view, depth / z above 1 on a third of the
    pixels (upper clamp ts - 1 - eps), weights of exactly 0 and exactly 1.  The LAST face of every view is never shown: with
    eps = 0 a clamped coordinate is exactly ts - 1, the kernel (like the reference) then fetches corner ts of the cube with
    weight 0, i.e. up to ts^2 + ts + 1 texels into the NEXT face's cube — which exists for every face shown, so every fetch
    stays inside `textures`."""
    rng = np.random.default_rng(seed)
    faces = rng.normal(size=(B, nf, 3, 3)).astype(np.float32)
    faces[..., 2] = rng.uniform(1.0, 2.0, size=(B, nf, 3))
    tex = rng.uniform(-1, 1, size=(B, nf, ts, ts, ts, 3)).astype(np.float32)
    fim = rng.integers(0, nf - 1, size=(B, S, S)).astype(np.int32)
    fim[rng.random((B, S, S)) < 0.3] = -1
    fim[B - 1, S - 1, S - 1] = nf - 2                       # the last lane of the ragged last workgroup is covered
    w = rng.dirichlet([1.0, 1.0, 1.0], size=(B, S, S)).astype(np.float32)
    corner = rng.integers(0, 8, size=(B, S, S))
    for k in range(3):                                       # one pixel in eight sits on a vertex: weights (1, 0, 0)
        w[corner == k] = np.eye(3, dtype=np.float32)[k]
    dm = rng.uniform(0.5, 1.0, size=(B, S, S)).astype(np.float32)
    high = rng.random((B, S, S)) < 0.33
    dm[high] = rng.uniform(2.5, 4.0, size=int(high.sum()))  # depth / z >= 1.25: a weight of 1 lands above ts - 1
    return {'faces': faces, 'textures': tex, 'face_index_map': fim, 'weight_map': w, 'depth_map': dm, 'image_size': S,
            'eps': eps, 'texture_size': ts}


def texture_sampling_want(c):
    """C oracle into sentinel-filled outputs (background pixels keep the sentinel) + facts for the non-vacuity asserts."""
    B, S = c['face_index_map'].shape[:2]
    nf, ts = c['faces'].shape[1], c['texture_size']
    rgb = np.full((B, S, S, 3), SENTINEL_F, np.float32)
    sim = np.full((B, S, S, 8), SENTINEL_I, np.int32)
    swm = np.full((B, S, S, 8), SENTINEL_F, np.float32)
    p = oras._p
    assert c['face_index_map'].max() < nf - 1               # see texture_sampling_case: the fetches stay in range
    oras.lib().oracle_texture_sampling(p(c['faces']), p(c['textures']), p(c['face_index_map']), p(c['weight_map']),
                                       p(c['depth_map']), p(rgb), p(sim), p(swm), B, nf, S, ts, ctypes.c_float(c['eps']))
    cov = c['face_index_map'] >= 0
    zf = c['faces'][np.arange(B)[:, None, None], np.maximum(c['face_index_map'], 0)][..., 2]              # [B,S,S,3]
    raw = c['weight_map'] * np.float32(ts - 1) * (c['depth_map'][..., None] / zf)
    facts = {'covered': int(cov.sum()), 'background': int((~cov).sum()),
             'upper_clamped': int(((raw > np.float32(ts - 1) - np.float32(c['eps'])) & cov[..., None]).sum()),
             'weight_zero': int(((c['weight_map'] == 0) & cov[..., None]).sum()),
             'weight_one': int(((c['weight_map'] == 1) & cov[..., None]).sum())}
    assert sim[cov].min() >= 0 and (sim[cov].max() < ts ** 3 or c['eps'] == 0) and sim[cov].max() < 2 * ts ** 3
    return {'rgb_map': rgb, 'sampling_index_map': sim, 'sampling_weight_map': swm}, facts


# =====================================================================================================================
# load_textures / create_texture_image
# =====================================================================================================================
WRAP_REPEAT, WRAP_MIRRORED, WRAP_CLAMP_EDGE, WRAP_CLAMP_BORDER = 0, 1, 2, 3
# the header's rule on exact integers, each coordinate wrapped ONCE with the reference's mod(): x > 0 ? fmod(x, y) : y + fmod(x, y)
WRAPPED_ONCE = {WRAP_REPEAT: {-1.0: 1.0, 0.0: 1.0, 1.0: 0.0, 2.0: 0.0},
                WRAP_MIRRORED: {-1.0: 0.0, 0.0: 0.0, 1.0: 1.0, 2.0: 0.0},
                WRAP_CLAMP_EDGE: {-1.0: 0.0, 0.0: 0.0, 1.0: 1.0, 2.0: 1.0},
                WRAP_CLAMP_BORDER: {-1.0: -1.0, 0.0: 0.0, 1.0: 1.0, 2.0: 2.0}}
INTEGER_UVS = [-1.0, 0.0, 1.0, 2.0]


def load_textures_case(ih, iw, ts, seed, nf=37):
    """uv coordinates on, just below and just above the integers -1, 0, 1, 2, negatives, and ordinary ones; a mixed
    is_update; cubes and an image of random values."""
    rng = np.random.default_rng(seed)
    uv = rng.uniform(-2.5, 3.5, size=(nf, 3, 2)).astype(np.float32)
    ints = np.array(INTEGER_UVS, np.float32)
    special = np.concatenate([ints, np.nextafter(ints, np.float32(-9)), np.nextafter(ints, np.float32(9)),
                              ints - np.float32(1e-3), ints + np.float32(1e-3)]).astype(np.float32)
    flat = uv.reshape(-1)
    where = rng.permutation(flat.size)[:3 * len(special)]
    flat[where] = np.tile(special, 3)
    flat[:len(ints)] = ints                                   # face 0 (updated) carries every integer at least once
    upd = (rng.random(nf) < 0.7).astype(np.int32)
    upd[0], upd[1], upd[nf - 1] = 1, 0, 1
    flat[6:6 + len(ints)] = ints                              # ... and so does face 1, which is NOT updated
    return {'image': rng.uniform(0, 1, size=(ih, iw, 3)).astype(np.float32), 'faces': uv,
            'textures': rng.uniform(2, 3, size=(nf, ts, ts, ts, 3)).astype(np.float32), 'is_update': upd}


def create_texture_image_case(nf, tsi, tile, seed):
    """Tile triangles from the drop-in neural_renderer/save_obj.py, random cubes, an atlas pre-filled with a sentinel."""
    import importlib
    save_obj = importlib.import_module('neural_renderer.save_obj')      # the package re-exports the function under this name
    rng = np.random.default_rng(seed)
    per_row, rows = save_obj._tile_grid(nf)
    corners = save_obj._tile_corners(nf, per_row, tile)
    tex = rng.uniform(0, 1, size=(nf, tsi, tsi, tsi, 3)).astype(np.float32)
    image = np.full((rows * tile, per_row * tile, 3), SENTINEL_F, np.float32)
    return {'vertices_all': corners, 'textures': tex, 'image': image, 'per_row': per_row, 'rows': rows, 'tile': tile}


def create_texture_image_want(c, eps=1e-5):
    """C oracle into a copy of the sentinel-filled atlas + the mask of the pixels of tiles beyond the last face."""
    img = c['image'].copy()
    p = oras._p
    nf, tsi = c['textures'].shape[:2]
    oras.lib().oracle_create_texture_image(p(c['vertices_all']), p(c['textures']), p(img), nf, tsi, img.shape[0],
                                           img.shape[1], ctypes.c_float(eps))
    y, x = np.mgrid[:img.shape[0], :img.shape[1]]
    beyond = (x // c['tile'] + (y // c['tile']) * c['per_row']) >= nf
    return img, beyond


# =====================================================================================================================
# rnr_project_vertices: float64 reference with a running error bound
# =====================================================================================================================
class _E:
    """A float64 value of the exact formula together with a bound on |float32 evaluation - value| (running error analysis):
    an operation on operands a, b with bounds ea, eb propagates them through its partial derivatives (with the second-order
    term kept) and adds its own rounding 2^-24 |computed result| <= 2^-24 (|value| + propagated)."""

    __array_ufunc__ = None      # ndarray (op) _E defers to the reflected method below

    def __init__(self, v, e=None):
        self.v = np.asarray(v, np.float64)
        self.e = np.zeros_like(self.v) if e is None else e

    @staticmethod
    def _wrap(x):
        return x if isinstance(x, _E) else _E(np.asarray(x, np.float64))

    @staticmethod
    def _round(v, prop):
        return _E(v, prop + U32 * (np.abs(v) + prop))

    def __add__(self, o):
        o = _E._wrap(o)
        return _E._round(self.v + o.v, self.e + o.e)
    __radd__ = __add__

    def __sub__(self, o):
        o = _E._wrap(o)
        return _E._round(self.v - o.v, self.e + o.e)

    def __rsub__(self, o):
        return _E._wrap(o) - self

    def __mul__(self, o):
        o = _E._wrap(o)
        return _E._round(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e)
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = _E._wrap(o)
        q = self.v / o.v
        assert (np.abs(o.v) > 2 * o.e).all()
        return _E._round(q, (self.e + np.abs(q) * o.e) / (np.abs(o.v) - o.e))

    def sqrt(self):
        s = np.sqrt(self.v)
        low = np.sqrt(np.maximum(self.v - self.e, 0.0))
        return _E._round(s, np.where(self.e > 0, self.e / np.maximum(s + low, 1e-300), 0.0))


def project_ref(vertices, K, R, t, orig_size, dist_coeffs=None, offset=None, scale=None, eps=1e-9):
    """nr.projection as include/rnr_hip.h states it, evaluated in float64 from the float32 inputs: vertices [nv,3] (or
    [N,nv,3]), K, R [N,3,3], t [N,3], dist_coeffs [N,5], offset / scale [N,2] (u takes component 1, v component 0).
    -> (out [N,nv,3] float64, bound [N,nv,3]): |float32 kernel - out| <= bound for every evaluation that performs the
    formula's operations in binary32 with one correctly rounded result each, whatever the order inside its sums of products
    (the bound of a sum does not depend on the order)."""
    f = lambda x: np.asarray(np.asarray(x, np.float32), np.float64)
    K, R, t = f(K), f(R), f(t).reshape(-1, 3)
    N = K.shape[0]
    v = f(vertices)
    v = np.broadcast_to(v, (N,) + v.shape[-2:])
    vx, vy, vz = (_E(v[..., i]) for i in range(3))
    row = lambda M, i, j: M[:, i, j][:, None]
    cam = [vx * row(R, i, 0) + vy * row(R, i, 1) + vz * row(R, i, 2) + t[:, i][:, None] for i in range(3)]
    x, y, z = cam
    e32 = float(np.float32(eps))
    xn, yn = x / (z + e32), y / (z + e32)
    d = f(dist_coeffs) if dist_coeffs is not None else np.zeros((N, 5))
    k1, k2, p1, p2, k3 = (d[:, i][:, None] for i in range(5))
    r = (xn * xn + yn * yn).sqrt()
    r2 = r * r
    r4 = r2 * r2
    r6 = r4 * r2
    radial = 1.0 + k1 * r2 + k2 * r4 + k3 * r6
    xd = xn * radial + 2.0 * p1 * xn * yn + p2 * (r2 + 2.0 * xn * xn)
    yd = yn * radial + p1 * (r2 + 2.0 * yn * yn) + 2.0 * p2 * xn * yn
    u = xd * row(K, 0, 0) + yd * row(K, 0, 1) + row(K, 0, 2)
    w = xd * row(K, 1, 0) + yd * row(K, 1, 1) + row(K, 1, 2)
    if offset is not None and scale is not None:
        off, sc = f(offset), f(scale)
        u = (u + off[:, 1][:, None]) * sc[:, 1][:, None]
        w = (w + off[:, 0][:, None]) * sc[:, 0][:, None]
    o = float(np.float32(orig_size))
    w = o - w
    u = 2.0 * (u - o / 2.0) / o
    w = 2.0 * (w - o / 2.0) / o
    return np.stack([u.v, w.v, z.v], -1), np.stack([u.e, w.e, z.e], -1)


def projection_case(seed, N=3, nv=300, orig_size=256):
    """Well-conditioned views: z >= 0.5 and |x/z|, |y/z| <= 1 for every vertex in every view; K, R, t, distortion
    (|k| <= 0.1), offset and scale differ per view (and offset / scale per component)."""
    rng = np.random.default_rng(seed)
    ang = rng.uniform(-0.3, 0.3, size=(N, 3))
    R = np.zeros((N, 3, 3))
    for n in range(N):
        cx, cy, cz = np.cos(ang[n])
        sx, sy, sz = np.sin(ang[n])
        R[n] = (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
                @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))
    t = np.stack([rng.uniform(-0.2, 0.2, N), rng.uniform(-0.2, 0.2, N), rng.uniform(3.0, 4.0, N)], -1)
    fx = rng.uniform(200, 300, N)
    K = np.zeros((N, 3, 3))
    K[:, 0, 0], K[:, 1, 1], K[:, 2, 2] = fx, fx * rng.uniform(0.9, 1.1, N), 1.0
    K[:, 0, 1] = rng.uniform(-2, 2, N)
    K[:, 0, 2], K[:, 1, 2] = rng.uniform(120, 136, N), rng.uniform(120, 136, N)
    c = {'vertices': rng.uniform(-1.0, 1.0, size=(nv, 3)).astype(np.float32),
         'vertices_per_view': rng.uniform(-1.0, 1.0, size=(N, nv, 3)).astype(np.float32),
         'K': K.astype(np.float32), 'R': R.astype(np.float32), 't': t.astype(np.float32),
         'dist_coeffs': rng.uniform(-0.1, 0.1, size=(N, 5)).astype(np.float32),
         'offset': rng.uniform(-20, 20, size=(N, 2)).astype(np.float32),
         'scale': rng.uniform(0.5, 1.5, size=(N, 2)).astype(np.float32), 'orig_size': orig_size}
    for vv in (c['vertices'][None], c['vertices_per_view']):
        cam = np.einsum('nij,nvj->nvi', c['R'].astype(np.float64), np.broadcast_to(vv, (N, nv, 3)).astype(np.float64)) \
            + c['t'][:, None, :]
        assert cam[..., 2].min() >= 0.5 and np.abs(cam[..., :2] / cam[..., 2:]).max() <= 1.0
    assert np.abs(c['offset'][:, 0] - c['offset'][:, 1]).min() > 0.01 and np.abs(c['scale'][:, 0] - c['scale'][:, 1]).min() > 1e-3
    return c
