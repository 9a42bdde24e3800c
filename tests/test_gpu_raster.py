"""-m gpu: HIP rasterizer (through the C ABI) vs the reference golden vectors and the C oracle.
Bar: face_index_map / weight_map / depth_map / faces_inv / face_inv_map BIT-EXACT (integer and float maps)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def bits(a):
    """Bit pattern of a float32 array with NaNs canonicalised: IEEE-754 leaves the sign/payload of a generated NaN
    unspecified (x86 SSE produces 0xffc00000 for 0/0, gfx950 0x7fc00000); every non-NaN value is compared bit for bit."""
    a = np.ascontiguousarray(a)
    if a.dtype != np.float32:
        return a
    b = a.view(np.uint32).copy()
    b[np.isnan(a)] = 0x7fc00000
    return b


def run_hip_raster(faces, S, near, far):
    from rnr_amd import ops
    dev = 'cuda:0'
    f = torch.from_numpy(np.ascontiguousarray(faces, np.float32)).to(dev)
    B, nf = f.shape[:2]
    fim = torch.full((B, S, S), -1, dtype=torch.int32, device=dev)
    wm = torch.zeros(B, S, S, 3, device=dev)
    dm = torch.full((B, S, S), far, dtype=torch.float32, device=dev)
    fivm = torch.zeros(B, S, S, 3, 3, device=dev)
    finv = torch.zeros_like(f)
    ops.forward_face_index_map(f, fim, wm, dm, fivm, finv, S, near, far, 1, 1, 1)
    torch.cuda.synchronize()
    return {'face_index_map': fim.cpu().numpy(), 'weight_map': wm.cpu().numpy(), 'depth_map': dm.cpu().numpy(),
            'face_inv_map': fivm.cpu().numpy(), 'faces_inv': finv.cpu().numpy().reshape(B, nf, 9)}


def assert_same(r, g):
    nbad = int((r['face_index_map'] != g['face_index_map']).sum())
    assert nbad == 0, 'face_index_map differs at %d pixels' % nbad
    for k in ['faces_inv', 'weight_map', 'depth_map', 'face_inv_map']:
        assert np.array_equal(bits(r[k]), bits(np.asarray(g[k]).reshape(r[k].shape))), k


@pytest.mark.parametrize('name', ['raster_soup64', 'raster_soup50', 'raster_soup64_nearfar', 'raster_sphere128'])
def test_golden_bit_exact(golden, name):
    g = golden(name)
    r = run_hip_raster(g['faces'], int(g['image_size']), float(g['near']), float(g['far']))
    assert_same(r, g)


FMA_CASES = ['raster_soup64', 'raster_soup50', 'raster_soup64_nearfar', 'raster_sphere128']


@pytest.mark.parametrize('name', FMA_CASES)
def test_index_map_equals_fma_contracted_reference(golden, name):
    """The reference is compiled by nvcc with --fmad=true (neural_renderer/setup.py:14-27 passes no flags); the
    `_fma` fixtures are its kernel bodies built with -ffp-contract=fast -mfma.  The HIP index map (built without
    contraction) must equal that one too; float maps are allowed the drift the two reference builds show between
    themselves (recorded in the fixture)."""
    g, gf = golden(name), golden(name + '_fma')
    assert int(gf['index_flips']) == 0                      # the two reference builds agree on every pixel
    r = run_hip_raster(g['faces'], int(g['image_size']), float(g['near']), float(g['far']))
    assert np.array_equal(r['face_index_map'], gf['face_index_map_fma'])
    cov = r['face_index_map'] >= 0
    ok = np.isfinite(gf['weight_map_fma']).all(-1) & np.isfinite(r['weight_map']).all(-1) & cov
    assert np.abs(r['weight_map'][ok] - gf['weight_map_fma'][ok]).max() <= 2 * float(gf['weight_abs_max']) + 1e-7


def test_sphere512_index_map_equals_both_reference_builds(golden):
    """Bench workload (65 536-face sphere, 512^2, spiral view 37): projected vertices come from the fixture (reference
    projection.py run in the build container), so nothing depends on this host's libm/matmul; the HIP index map must
    equal the reference kernel's under BOTH contraction modes."""
    from rnr_amd import scene
    gf = golden('raster_sphere512_fma')
    assert int(gf['index_flips']) == 0
    assert np.array_equal(gf['face_index_map_nofma'], gf['face_index_map_fma'])
    idx = scene.uv_sphere(128, 256)['f_v_idx']
    faces = gf['v_uvz'][:, idx.astype(np.int64)]            # vertices_to_faces.py:4-46
    r = run_hip_raster(faces, 512, 0.0, 1e5)
    assert np.array_equal(r['face_index_map'], gf['face_index_map_fma'])
    assert 0.4 < (r['face_index_map'] >= 0).mean() < 0.7


def test_sphere512_worst_fma_view_equals_noncontracted_reference(golden):
    """The view of the 200-view sweep in which FMA contraction flips the most face indices (tests/fma_sweep_report.json):
    the HIP index map equals the reference evaluated WITHOUT contraction on all 262 144 pixels, and therefore differs from
    the contracted builds exactly where those differ from it."""
    from rnr_amd import scene
    gf = golden('raster_sphere512_worst_fma')
    idx = scene.uv_sphere(128, 256)['f_v_idx']
    faces = gf['v_uvz'][:, idx.astype(np.int64)]
    r = run_hip_raster(faces, 512, 0.0, 1e5)
    assert np.array_equal(r['face_index_map'], gf['face_index_map_nofma'])
    assert int((r['face_index_map'] != gf['face_index_map_fma']).sum()) == int(gf['index_flips']) > 0
    assert int((r['face_index_map'] != gf['face_index_map_fma_clang']).sum()) == int(gf['index_flips_clang'])


@pytest.mark.parametrize('S,nf,seed,near', [
    pytest.param(17, 50, 1, 0.0, id='17-50-1'), pytest.param(96, 3000, 2, 0.0, id='96-3000-2'),
    pytest.param(256, 20000, 3, 0.0, id='256-20000-3'), pytest.param(33, 1, 4, 0.0, id='33-1-4'),
    (96, 3000, 2, -1.0), (160, 4000, 5, -1.0)])
def test_random_soup_vs_oracle(S, nf, seed, near):
    """Ragged sizes, many overlapping faces, slivers and far-away faces, batch of 2.  near < 0 takes face_setup_kernel +
    bin_faces_kernel instead of the fused setup / splat launch: every z is positive, so the maps are those of near = 0 and
    only the kernels differ (2 620 binned faces in the first such case; 3 368 binned, 711 on the wide list in the second)."""
    from oracle import raster as oras
    rng = np.random.RandomState(seed)
    f = rng.uniform(-1.5, 1.5, size=(2, nf, 3, 3)).astype(np.float32)
    f[..., 2] = rng.uniform(0.2, 9.0, size=(2, nf, 3))
    small = rng.rand(2, nf) < 0.7                      # most faces small (a few pixels), like a real mesh
    c = f[:, :, :1, :2].copy()
    f[..., :2] = np.where(small[..., None, None], c + (f[..., :2] - c) * 0.03, f[..., :2])
    if nf > 10:
        f[0, 3, 1] = f[0, 3, 0]                                    # coincident vertices
        f[0, 4, 2, :2] = f[0, 4, 0, :2] * 0.25 + f[0, 4, 1, :2] * 0.75   # (nearly) collinear
        f[1, 5, :, :2] *= 1e4                                      # huge
        f[1, 6, 0, 0] = np.nan
        f[0, 7, :, 2] = [1e-30, 2.0, 3.0]
    g = oras.face_index_map(f, S, near, 1e5)
    r = run_hip_raster(f, S, near, 1e5)
    assert_same(r, g)
    if nf > 10:
        assert (g['face_index_map'] >= 0).mean() > 0.3


def test_back_faces_never_rasterize():
    """Every face twice, once with reversed winding (what fill_back does, renderer.py:209-211): the culled copies
    must never be picked, in particular not in tile (0,0) (regression: an 'empty' box that still overlapped tile 0)."""
    from oracle import raster as oras
    rng = np.random.RandomState(11)
    f = rng.uniform(-1.2, 1.2, size=(1, 600, 3, 3)).astype(np.float32)
    f[..., 2] = rng.uniform(0.5, 5.0, size=(1, 600, 3))
    both = np.concatenate([f, f[:, :, ::-1, :]], 1)
    g = oras.face_index_map(both, 48, 0.0, 1e5)
    r = run_hip_raster(both, 48, 0.0, 1e5)
    assert_same(r, g)


def test_bin_overflow_falls_back_to_scan():
    """> BIN_CAP (2048) candidates in one tile: that tile must rescan all boxes and still match bit for bit."""
    from oracle import raster as oras
    rng = np.random.RandomState(12)
    S, nf = 64, 6000
    f = np.zeros((1, nf, 3, 3), np.float32)
    c = rng.uniform(-0.4, -0.1, size=(nf, 1, 2))                # all centres inside one 16x16 tile
    f[0, :, :, :2] = c + rng.uniform(-0.08, 0.08, size=(nf, 3, 2))
    f[0, :, :, 2] = rng.uniform(0.5, 5.0, size=(nf, 3))
    f[0, :200, :, :2] = rng.uniform(-1.2, 1.2, size=(200, 3, 2))   # plus some faces elsewhere
    g = oras.face_index_map(f, S, 0.0, 1e5)
    r = run_hip_raster(f, S, 0.0, 1e5)
    assert_same(r, g)


@pytest.mark.parametrize('S,n_wide,n_plain,seed', [(128, 3000, 1500, 21), (64, 900, 5000, 22)])
def test_many_wide_faces_flush_path_vs_oracle(S, n_wide, n_plain, seed):
    """The wide-face list of raster_tile_kernel with FAR more entries than one pass of the workgroup (256) and a candidate queue
    that fills up: thousands of zero-area faces (two coincident vertices -> exact-only boxes; their pass region is a line through
    the image, so each one is a candidate of many tiles) between ordinary faces.  ADVICE r04: the flush decision read the queue
    length without a barrier behind it, so a fast wave could append for the next pass before a slow one had read it and the two
    took different branches around barriers.  Bit-exact against the oracle, five launches in a row (a barrier mismatch shows as a
    wrong winner or a hang), batch of 2 with different face sets."""
    from oracle import raster as oras
    rng = np.random.RandomState(seed)
    nf = n_wide + n_plain
    f = rng.uniform(-1.3, 1.3, size=(2, nf, 3, 3)).astype(np.float32)
    f[..., 2] = rng.uniform(0.3, 8.0, size=(2, nf, 3))
    small = rng.rand(2, nf) < 0.6
    c = f[:, :, :1, :2].copy()
    f[..., :2] = np.where(small[..., None, None], c + (f[..., :2] - c) * 0.05, f[..., :2])
    wide = rng.permutation(nf)[:n_wide]
    f[:, wide, 1] = f[:, wide, 0]                       # coincident vertices: zero area, inf / NaN barycentric inverse
    f[1, wide[: n_wide // 3], 2, :2] = f[1, wide[: n_wide // 3], 0, :2]     # ... and fully collapsed ones in view 1
    g = oras.face_index_map(f, S, 0.0, 1e5)
    for _ in range(5):
        r = run_hip_raster(f, S, 0.0, 1e5)
        assert_same(r, g)
    assert (g['face_index_map'] >= 0).mean() > 0.3


@pytest.mark.parametrize('S,seed,near', [(64, 31, 0.0), (128, 32, 0.0), (48, 33, 0.0), (50, 34, 0.0), (64, 35, -1.0)])
def test_zero_area_faces_through_pixel_centres_vs_oracle(S, seed, near):
    """raster_tile_kernel walks a zero-area wide face (two coincident vertices) along its line and tests the two pixels next to
    the crossing of every row / column instead of all 256 pixels of the tile (r06).  Here the lines pass EXACTLY through pixel
    centres (both vertices sit on centres, rational slopes; at S = 64 / 128 every product of the edge tests is exact), so the
    reference's inside test passes on many pixels and the inf / NaN barycentric arithmetic behind it runs: all three
    coincidence patterns, steep / shallow / axis-parallel lines, end points far outside the image, faces beyond the walk's
    coordinate bound (|x| > 4: ordinary queue entries), ordinary faces in front and behind; S = 50: edge tiles clipped by the
    image; near < 0: the binning path without per-pixel keys, where no face is walked.  Bit-exact against the oracle."""
    from oracle import raster as oras
    rng = np.random.RandomState(seed)
    n_line, n_plain = 360, 120
    nf = n_line + n_plain
    f = rng.uniform(-1.2, 1.2, size=(2, nf, 3, 3)).astype(np.float32)
    f[..., 2] = rng.uniform(0.3, 8.0, size=(2, nf, 3))
    small = rng.rand(2, nf) < 0.5
    c = f[:, :, :1, :2].copy()
    f[..., :2] = np.where(small[..., None, None], c + (f[..., :2] - c) * 0.1, f[..., :2])

    def centre(i):
        return ((2 * i + 1 - S).astype(np.float32) / np.float32(S)).astype(np.float32)
    for b in range(2):
        i0, j0 = rng.randint(0, S, n_line), rng.randint(0, S, n_line)
        p, q = rng.randint(-3, 4, n_line), rng.randint(-3, 4, n_line)
        both0 = (p == 0) & (q == 0)
        p[both0] = 1
        k = rng.choice([1, 2, 5, S, 3 * S], n_line)
        k[:20] = 40 * S                                   # end point beyond |x| = 4: not walked, an ordinary wide-list entry
        a = np.stack([centre(i0), centre(j0)], -1)
        bb = np.stack([centre(i0 + p * k), centre(j0 + q * k)], -1)
        if S in (48, 50):                                 # not a power of two: nudge half of them off the exact centres
            bb[::2] += rng.uniform(-1e-6, 1e-6, size=bb[::2].shape).astype(np.float32)
        pat = rng.randint(0, 3, n_line)                   # which two vertices coincide: (0,1) (1,2) (2,0)
        for t in range(n_line):
            xy = {0: (a[t], a[t], bb[t]), 1: (a[t], bb[t], bb[t]), 2: (a[t], bb[t], a[t])}[pat[t]]
            for vtx in range(3):
                f[b, t, vtx, :2] = xy[vtx]
    perm = rng.permutation(nf)
    f = f[:, perm]
    g = oras.face_index_map(f, S, near, 1e5)
    r = run_hip_raster(f, S, near, 1e5)
    assert_same(r, g)
    # (Evaluated without FMA contraction such a face has den == 0 exactly, its barycentric rows are +-inf / NaN, and a pixel
    # that passes the inside test gets inf - inf = NaN weights and a NaN depth: it never wins.  The walk must not invent a
    # winner either, nor lose an ordinary one — which is what the bit-exact comparison above checks.)
    assert (g['face_index_map'] >= 0).mean() > 0.3


@pytest.mark.parametrize('view', [100, 162])
def test_sphere_512_vs_oracle(view):
    """BASELINE config size: 65 536-face UV sphere at 512^2 (includes the zero-area pole faces).  View 162 looks at a pole
    edge-on: ~250 sliver faces with boxes above 256 pixels are binned into a handful of tiles (215 candidates in one), 66
    non-degenerate slivers ride the wide list beside the 512 zero-area faces whose lines all cross the pole's tile."""
    from oracle import raster as oras
    from oracle import rnr_oracle as orc
    from rnr_amd import scene
    mesh = scene.uv_sphere(128, 256)
    v = scene.spiral_views(512, [view])
    uvz = orc.projection(torch.from_numpy(mesh['v'])[None], torch.from_numpy(v['proj']), torch.from_numpy(v['pose'][:, :3, :3]),
                         torch.from_numpy(v['pose'][:, :3, 3])[:, None, :], torch.zeros(1, 5), 512)
    faces = orc.gather_faces(uvz, torch.from_numpy(mesh['f_v_idx'])[None]).numpy()
    g = oras.face_index_map(faces, 512, 0.0, 1e5)
    r = run_hip_raster(faces, 512, 0.0, 1e5)
    assert_same(r, g)
    cov = (g['face_index_map'] >= 0).mean()
    assert 0.4 < cov < 0.7


def test_coarse_mesh_close_up_vs_oracle():
    """Faces far larger than 16 x 16 pixels (a 12 x 24 UV sphere filling a 512^2 image, plus a soup of mid-size triangles):
    every trusted box above 256 pixels is binned by setup_splat_faces_kernel itself, only untrusted / huge faces take the wide
    list (before, all of them did and were tested against every tile).  Bit-exact like everything else."""
    from oracle import raster as oras
    from oracle import rnr_oracle as orc
    from rnr_amd import scene
    mesh = scene.uv_sphere(12, 24)
    v = scene.spiral_views(512, [5, 300], radius=1.9)
    uvz = orc.projection(torch.from_numpy(mesh['v'])[None], torch.from_numpy(v['proj']), torch.from_numpy(v['pose'][:, :3, :3]),
                         torch.from_numpy(v['pose'][:, :3, 3])[:, None, :], torch.zeros(2, 5), 512)
    faces = orc.gather_faces(uvz, torch.from_numpy(mesh['f_v_idx'])[None]).numpy()
    g = oras.face_index_map(faces, 512, 0.0, 1e5)
    r = run_hip_raster(faces, 512, 0.0, 1e5)
    assert_same(r, g)
    assert (g['face_index_map'] >= 0).mean() > 0.5
    rng = np.random.RandomState(21)
    f = rng.uniform(-1.2, 1.2, size=(1, 400, 3, 3)).astype(np.float32)
    c = f[:, :, :1, :2].copy()
    f[..., :2] = c + (f[..., :2] - c) * rng.uniform(0.05, 0.6, size=(1, 400, 1, 1)).astype(np.float32)   # 20 ... 300 px across
    f[..., 2] = rng.uniform(0.5, 5.0, size=(1, 400, 3))
    g = oras.face_index_map(f, 384, 0.0, 1e5)
    r = run_hip_raster(f, 384, 0.0, 1e5)
    assert_same(r, g)


def test_dense_mesh_subpixel_faces_vs_oracle():
    """409 600 faces at 256^2: faces far smaller than a pixel, > 1000 candidates per 16x16 tile and list overflow at the
    poles (the scan fallback) in the same image; batch of two views.  Still bit-exact."""
    from oracle import raster as oras
    from oracle import rnr_oracle as orc
    from rnr_amd import scene
    mesh = scene.uv_sphere(320, 640)
    assert mesh['f_v_idx'].shape[0] == 409600
    v = scene.spiral_views(256, [0, 250])
    uvz = orc.projection(torch.from_numpy(mesh['v'])[None], torch.from_numpy(v['proj']), torch.from_numpy(v['pose'][:, :3, :3]),
                         torch.from_numpy(v['pose'][:, :3, 3])[:, None, :], torch.zeros(2, 5), 256)
    faces = orc.gather_faces(uvz, torch.from_numpy(mesh['f_v_idx'])[None]).numpy()
    g = oras.face_index_map(faces, 256, 0.0, 1e5)
    r = run_hip_raster(faces, 256, 0.0, 1e5)
    assert_same(r, g)


def test_texture_sampling_golden(golden):
    from rnr_amd import ops
    g = golden('raster_texsample32')
    dev = 'cuda:0'
    T = lambda k, dt=None: torch.from_numpy(np.ascontiguousarray(g[k])).to(dev)
    S = int(g['image_size'])
    rgb = torch.zeros(1, S, S, 3, device=dev)
    sim = torch.zeros(1, S, S, 8, dtype=torch.int32, device=dev)
    swm = torch.zeros(1, S, S, 8, device=dev)
    ops.forward_texture_sampling(T('faces'), T('textures'), T('face_index_map'), T('weight_map'), T('depth_map'), rgb, sim,
                                 swm, S, float(g['eps']))
    assert np.array_equal(sim.cpu().numpy(), g['sampling_index_map'])
    assert np.array_equal(bits(swm.cpu().numpy()), bits(g['sampling_weight_map']))
    assert np.array_equal(bits(rgb.cpu().numpy()), bits(g['rgb_map']))


def _t(a, dt=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda:0', dt).contiguous()


def run_hip_backward(g, rr, ra, faces=None):
    from rnr_amd import ops
    f = _t(g['faces'] if faces is None else faces)
    S = int(g['image_size'])
    gf = torch.zeros_like(f)
    ops.backward_pixel_map(f, _t(g['face_index_map'], torch.int32), _t(g['rgb_map']), _t(g['alpha_map']),
                           _t(g['grad_rgb_map']), _t(g['grad_alpha_map']), gf, S, float(g['eps']), rr, ra)
    torch.cuda.synchronize()
    return gf.cpu().numpy()


@pytest.mark.parametrize('name', ['raster_bwd_soup48', 'raster_bwd_soup64_ts2'])
def test_backward_pixel_map_bit_exact(golden, name):
    """Silhouette-sweep gradient: bit-identical to the reference kernel (golden) for every flag combination."""
    g = golden(name)
    for tag, rr, ra in [('both', 1, 1), ('alpha', 0, 1), ('rgb', 1, 0)]:
        r = run_hip_backward(g, rr, ra)
        assert np.array_equal(bits(r), bits(g['grad_faces_pixel_' + tag])), tag


@pytest.mark.parametrize('name', ['raster_bwd_soup48', 'raster_bwd_soup64_ts2'])
def test_backward_textures_and_depth(golden, name):
    """Atomic accumulations: unordered float sums, compared with a tolerance scaled by the sum of magnitudes."""
    from rnr_amd import ops
    g = golden(name)
    S, nf, ts = int(g['image_size']), g['faces'].shape[1], int(g['texture_size'])
    fim = _t(g['face_index_map'], torch.int32)
    gt = torch.zeros(2, nf, ts, ts, ts, 3, device='cuda:0')
    ops.backward_textures(fim, _t(g['sampling_weight_map']), _t(g['sampling_index_map'], torch.int32),
                          _t(g['grad_rgb_map']), gt, nf)
    ref = g['grad_textures']
    assert np.abs(gt.cpu().numpy() - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max())
    gf = torch.zeros(2, nf, 3, 3, device='cuda:0')
    ops.backward_depth_map(_t(g['faces']), _t(g['depth_map']), fim, _t(g['face_inv_map']), _t(g['weight_map']),
                           _t(g['grad_depth_map']), gf, S)
    ref = g['grad_faces_depth']
    assert np.abs(gf.cpu().numpy() - ref).max() <= 2e-5 * np.abs(ref).max()
    # accumulates on top of what grad_faces holds (rasterize.py:145-152 calls it after backward_pixel_map)
    gf2 = torch.ones(2, nf, 3, 3, device='cuda:0')
    ops.backward_depth_map(_t(g['faces']), _t(g['depth_map']), fim, _t(g['face_inv_map']), _t(g['weight_map']),
                           _t(g['grad_depth_map']), gf2, S)
    assert np.abs(gf2.cpu().numpy() - 1.0 - ref).max() <= 2e-5 * np.abs(ref).max()


def test_backward_sphere_vs_oracle():
    """A projected mesh at 256^2 (faces of a few pixels, the realistic case) with SSAA-free maps: forward on the HIP
    rasterizer, all three backward kernels vs the C oracle; pixel-map gradient bit-exact."""
    from oracle import raster as oras
    from rnr_amd import ops, scene
    S, eps = 256, 1e-4
    mesh = scene.uv_sphere(48, 96)
    views = scene.spiral_views(S, [5, 300])
    v = torch.from_numpy(mesh['v']).cuda()
    uvz = ops.project_vertices(v, torch.from_numpy(views['proj']).cuda(), torch.from_numpy(views['pose'][:, :3, :3]).contiguous().cuda(),
                               torch.from_numpy(views['pose'][:, :3, 3]).contiguous().cuda(), S)
    fidx = torch.from_numpy(mesh['f_v_idx']).long().cuda()
    faces = uvz[:, fidx].contiguous()                      # [2, nf, 3, 3]
    nf = faces.shape[1]
    r = run_hip_raster(faces.cpu().numpy(), S, 0.0, 1e5)
    rng = np.random.RandomState(3)
    tex = rng.uniform(0, 1, size=(2, nf, 2, 2, 2, 3)).astype(np.float32)
    t = oras.texture_sampling(faces.cpu().numpy(), tex, r['face_index_map'], r['weight_map'], r['depth_map'], S, eps)
    alpha = (r['face_index_map'] >= 0).astype(np.float32)
    g = {'faces': faces.cpu().numpy(), 'image_size': S, 'eps': eps, 'face_index_map': r['face_index_map'],
         'rgb_map': t['rgb_map'] * alpha[..., None], 'alpha_map': alpha,
         'grad_rgb_map': rng.normal(size=(2, S, S, 3)).astype(np.float32),
         'grad_alpha_map': rng.normal(size=(2, S, S)).astype(np.float32)}
    want = oras.backward_pixel_map(g['faces'], g['face_index_map'], g['rgb_map'], g['alpha_map'], g['grad_rgb_map'],
                                   g['grad_alpha_map'], S, eps, 1, 1)
    got = run_hip_backward(g, 1, 1)
    assert np.array_equal(bits(got), bits(want))
    assert (want != 0).sum() > 1000
    gd = rng.normal(size=(2, S, S)).astype(np.float32)
    want_d = oras.backward_depth_map(g['faces'], r['depth_map'], r['face_index_map'], r['face_inv_map'], r['weight_map'], gd, S)
    gf = torch.zeros(2, nf, 3, 3, device='cuda:0')
    ops.backward_depth_map(faces, _t(r['depth_map']), _t(r['face_index_map'], torch.int32), _t(r['face_inv_map']),
                           _t(r['weight_map']), _t(gd), gf, S)
    assert np.abs(gf.cpu().numpy() - want_d).max() <= 2e-5 * np.abs(want_d).max()


def test_rasterize_function_autograd():
    """nr.rasterize_rgbad is differentiable end to end through RasterizeFunction (rasterize.py:15-152): gradients of
    a scalar loss reach faces and textures and equal the three kernels chained by hand (flip + SSAA handled by torch)."""
    import neural_renderer as nr
    from oracle import raster as oras
    rng = np.random.RandomState(11)
    nf, S, ts = 40, 32, 2
    f = rng.uniform(-0.9, 0.9, size=(1, nf, 3, 3)).astype(np.float32)
    f[..., 2] = rng.uniform(1.0, 3.0, size=(1, nf, 3))
    faces = torch.from_numpy(f).cuda().requires_grad_(True)
    tex = torch.rand(1, nf, ts, ts, ts, 3, device='cuda:0', requires_grad=True)
    out = nr.rasterize_rgbad(faces, tex, image_size=S, anti_aliasing=False, near=0.1, far=100.0, eps=1e-3,
                             background_color=(0, 0, 0))
    wr = torch.randn_like(out['rgb']); wa = torch.randn_like(out['alpha']); wd = torch.randn_like(out['depth'])
    loss = (out['rgb'] * wr).sum() + (out['alpha'] * wa).sum() + (out['depth'] * wd).sum()
    loss.backward()
    assert faces.grad is not None and tex.grad is not None
    # by hand on the oracle: un-flip the loss weights into the extension's row order
    r = oras.face_index_map(f, S, 0.1, 100.0)
    t = oras.texture_sampling(f, tex.detach().cpu().numpy(), r['face_index_map'], r['weight_map'], r['depth_map'], S, 1e-3)
    alpha = (r['face_index_map'] >= 0).astype(np.float32)
    g_rgb = wr.flip(2).permute(0, 2, 3, 1).contiguous().cpu().numpy()
    g_a = wa.flip(1).contiguous().cpu().numpy()
    g_d = wd.flip(1).contiguous().cpu().numpy()
    gf = oras.backward_pixel_map(f, r['face_index_map'], t['rgb_map'] * alpha[..., None], alpha, g_rgb, g_a, S, 1e-3, 1, 1)
    gf = oras.backward_depth_map(f, r['depth_map'], r['face_index_map'], r['face_inv_map'], r['weight_map'], g_d, S, grad_faces=gf)
    gt = oras.backward_textures(r['face_index_map'], t['sampling_weight_map'], t['sampling_index_map'], g_rgb, nf, ts)
    assert np.abs(faces.grad.cpu().numpy() - gf).max() <= 1e-4 * max(1.0, np.abs(gf).max())
    assert np.abs(tex.grad.cpu().numpy() - gt).max() <= 1e-5 * max(1.0, np.abs(gt).max())


def test_argument_checks():
    from rnr_amd import ops
    f = torch.zeros(1, 4, 3, 3)
    with pytest.raises(RuntimeError):
        ops.forward_face_index_map(f, f, f, f, f, f, 8, 0.0, 1.0, 1, 1, 1)      # CPU tensors are rejected


def test_frame_prepare_and_prepared_raster_argument_checks():
    """frame_prepare strides the poses by 16 floats (a [N,3,4] pose used to project wrongly and read out of bounds),
    dereferenced lp_basis / lp_coeff without a None check, and rasterize_gbuffer(prepared=True) without the workspace frame_prepare
    cleared ran on uninitialised counters: all three raise now."""
    from rnr_amd import ops, scene
    dev = 'cuda:0'
    m = scene.uv_sphere(8, 16)
    dm = ops.DeviceMesh(m['v'], m['vt'], m['vn'], m['f_v_idx'], m['f_vt_idx'], m['f_vn_idx'], dev)
    v = {k: torch.from_numpy(x).to(dev) for k, x in scene.spiral_views(32, [3, 9]).items()}
    v_uvz = torch.empty(2, dm.num_vertices, 3, device=dev)
    with pytest.raises(ValueError, match='pose'):
        ops.frame_prepare(dm, v['proj'], v['pose'][:, :3].contiguous(), 32, v_uvz=v_uvz)          # [N,3,4]
    with pytest.raises(ValueError, match='pose'):
        ops.frame_prepare(dm, v['proj'], v['pose'][:1].contiguous(), 32, v_uvz=v_uvz)             # fewer poses than K
    with pytest.raises(ValueError, match='lp_basis'):
        ops.frame_prepare(dm, v['proj'], v['pose'], 32, v_uvz=v_uvz, light_probe=torch.empty(10, 3, device=dev))
    ops.frame_prepare(dm, v['proj'], v['pose'], 32, v_uvz=v_uvz)                                   # the valid call still works
    with pytest.raises(ValueError, match='workspace'):
        ops.rasterize_gbuffer(dm, v_uvz, None, 32, prepared=True)
    gb = ops.rasterize_gbuffer(dm, v_uvz, None, 32, maps=['face_index_map'])
    assert int((gb['face_index_map'] >= 0).sum()) > 0


def test_gbuffer_vs_reference_module(golden):
    """Fused raster + interpolation vs network.Rasterizer.forward.
    (A) vs the oracle on THIS host, same projected vertices in: index map / alpha / raw weights / depth bit-exact,
        interpolated maps to 2e-6 (different association of three-term sums only);
    (B) vs the golden vectors produced by the reference's own Python in the build container: the projection there
        went through a different CPU's matmul rounding, so silhouette slivers move by ~1e-4 in barycentrics and a
        few pixels may flip: index mismatch < 0.2 %, smooth maps 1e-4, weights 5e-4."""
    from oracle import rnr_oracle as orc
    from rnr_amd import ops
    g = golden('rasterizer_module64')
    dev = 'cuda:0'
    mesh = ops.DeviceMesh(g['buf_vertices'][0], g['mesh_vt'], g['buf_vertices_normals'][0], g['mesh_f_v_idx'],
                          g['mesh_f_vt_idx'], g['mesh_f_vn_idx'], dev)
    mesh_t = {k: torch.from_numpy(g['mesh_' + k]) for k in ['v', 'vt', 'vn', 'f_v_idx', 'f_vt_idx', 'f_vn_idx']}
    mesh_t['v'], mesh_t['vn'] = torch.from_numpy(g['buf_vertices'][0]), torch.from_numpy(g['buf_vertices_normals'][0])
    S = int(g['image_size'])
    proj = torch.from_numpy(g['proj'])
    pose = torch.from_numpy(g['pose'])
    for i in range(2):
        o = orc.rasterizer_forward(mesh_t, proj[i:i + 1], pose[i:i + 1], S)
        v_cpu = orc.projection(mesh_t['v'][None], proj[i:i + 1], pose[i:i + 1, :3, :3], pose[i:i + 1, :3, 3][:, None, :],
                               torch.zeros(1, 5), S)
        gb = ops.rasterize_gbuffer(mesh, v_cpu.contiguous().to(dev), pose[i:i + 1].to(dev), S)
        torch.cuda.synchronize()
        c = lambda k: gb[k][0].cpu()
        assert torch.equal(c('face_index_map'), o['face_index_map'][0])
        assert torch.equal(c('alpha'), o['alpha'][0])
        assert np.array_equal(bits(c('raw_weight_map').numpy()), bits(o['raw_weight_map'][0].numpy()))
        assert np.array_equal(bits(c('depth').numpy()), bits(o['depth'][0, ..., 0].numpy()))
        for k in ['weight_map', 'uv_map', 'normal_map', 'normal_map_cam', 'position_map', 'position_map_cam']:
            ref = o[k][0].reshape(c(k).shape)
            d = (c(k) - ref).abs()
            if k == 'uv_map':
                d = torch.minimum(d, 1.0 - d)
            assert d.max() < 2e-6 * max(1.0, float(ref.abs().max())), (k, d.max())
        # (B) reference golden
        ref_idx = g['view%d_face_index_map' % i][0]
        mism = ref_idx != c('face_index_map').numpy()
        assert mism.mean() < 2e-3, mism.sum()
        ok = ~mism
        for k, tol in [('uv_map', 1e-4), ('normal_map', 1e-4), ('position_map', 1e-4), ('depth', 1e-4), ('weight_map', 5e-4)]:
            ref = g['view%d_%s' % (i, k)][0]
            d = np.abs(c(k).numpy().reshape(ref.shape) - ref)[ok]
            if k == 'uv_map':
                d = np.minimum(d, 1.0 - d)
            assert d.max() < tol * max(1.0, np.abs(ref[ok]).max()), (k, d.max())
    # (C) the reference's own projected NDC vertices (fixture `v_ndc`, captured at the nr.Renderer boundary) fed to the
    # HIP kernel: no host matmul in between, so the integer maps must equal the reference golden EXACTLY and the
    # interpolated maps to float rounding (pointwise three-term sums in a different association)
    for i in range(2):
        v_ref = torch.from_numpy(g['view%d_v_ndc' % i]).contiguous().to(dev)
        gb = ops.rasterize_gbuffer(mesh, v_ref, pose[i:i + 1].to(dev), S)
        torch.cuda.synchronize()
        c = lambda k: gb[k][0].cpu().numpy()
        assert np.array_equal(c('face_index_map'), g['view%d_face_index_map' % i][0])
        assert np.array_equal(c('alpha'), g['view%d_alpha' % i][0])
        for k, tol in [('uv_map', 2e-6), ('normal_map', 2e-6), ('normal_map_cam', 2e-6), ('position_map', 2e-6),
                       ('position_map_cam', 4e-6), ('depth', 2e-6), ('weight_map', 2e-6)]:
            ref = g['view%d_%s' % (i, k)][0]
            d = np.abs(c(k).reshape(ref.shape) - ref)
            if k == 'uv_map':
                d = np.minimum(d, 1.0 - d)
            assert d.max() <= tol * max(1.0, np.abs(ref).max()), (k, d.max())
    # HIP projection kernel vs the oracle's (well-conditioned vertices)
    v_hip = ops.project_vertices(mesh.v, proj.to(dev), pose[:, :3, :3].contiguous().to(dev),
                                 pose[:, :3, 3].contiguous().to(dev), S)
    v_ref = torch.cat([orc.projection(mesh_t['v'][None], proj[i:i + 1], pose[i:i + 1, :3, :3],
                                      pose[i:i + 1, :3, 3][:, None, :], torch.zeros(1, 5), S) for i in range(2)])
    assert torch.allclose(v_hip.cpu(), v_ref, atol=5e-6, rtol=1e-5)
