"""-m gpu: the fused G-buffer (raster.hip, raster_tile_kernel<1>: the MODE 1 epilogue) against the float64 reference
oracle/gbuffer64.py, swept over what the epilogue and the raster paths in front of it branch on: image sizes that are not
multiples of the 16 x 16 tile (the last, partial tile row and column, and their vertical flip), batches of views with a pose
each, the face-parallel splat path (near >= 0) and the binning path (near < 0), faces above 256 pixels, wide / untrusted
faces, bin overflow (> 2048 candidates in one tile), faces clipped by near and far, N * nf on both sides of the 131 072
at which setup_splat_faces_kernel switches from four lanes per face to one, and a last face at z = 0, where the background
values (face index -1 wraps to face nf - 1) are NaN in the reference too.

The attribute mesh (attr_mesh) has nv == nvt == nvn and independently permuted f_vt_idx / f_vn_idx, so uv or normals fetched
through the wrong index array stay in bounds and come out wrong; vt spans [-1.5, 2.5] with exact integers and faces on the
seam; vertex normals are neither unit nor outward, some faces carry exactly opposite normals, all-zero normals, or normals
below 1e-6 and below the 1e-12 clamp of F.normalize.

Exact (bit for bit, NaN payloads canonicalised): face_index_map, alpha, depth, raw_weight_map against the C oracle, and
weight_map against the float32 oracle: raster.hip evaluates ((1/z) * w) * depth in the operation order of network.py:176-180
(rnr_oracle.rasterizer_forward), correctly rounded (no contraction, -ffp-contract=off; hipcc's default correctly rounded
float division).  Every output of the product's call sequence (frame_prepare + rasterize_gbuffer(prepared=True), four maps)
and of every single-map call equals the all-maps call bit for bit, NaN payloads included.

Tolerances (uv, normal, position maps and their camera-space forms against float64) are bounds derived from the float32
arithmetic of raster.hip's MODE 1 epilogue, in units of EPS = 2^-24 (half an ulp of 1), never from a measured error.  Every
float32 +, -, *, / and sqrt there is correctly rounded: <= 1 EPS relative each.  Bounds are first order; each rounds its
constant up by at least one EPS, which covers the second-order terms at the magnitudes here.  The float64 reference's own
error (~2^-50 relative) is far below one EPS.  With w_k the exact weights (1/z_k) w_k depth of the float32 inputs:
  * weights, raster.hip `wp = ((1.0f / f[2]) * bw0) * depth`: three roundings, wp_k = w_k (1 + t), |t| <= 3 EPS.
  * interpolation, `a[0] * wp0 + b[0] * wp1 + c[0] * wp2` (uv, normal, position; left to right): three products (1 EPS
    each) and two additions (<= 2 EPS of the sum of the magnitudes), plus the weights' 3 EPS:
    |x' - x| <= 6 EPS sum_k |a_k w_k|  ->  7 EPS * A with A = the reference's sum_k |a_k w_k| (uv_abs, normal_abs,
    position_abs).  position_map: 7 EPS * A.
  * uv wrap, `u - floorf(u)`: floorf is exact; the subtraction is exact by Sterbenz's lemma except for u in [-1, 0), where
    the result in (0, 1] rounds by <= 1 EPS.  uv is compared modulo 1 (the wrap of u and of u + 7 EPS A may differ by
    exactly 1): uv_map: 7 EPS * A + 1 EPS.
  * normalisation, `inv = 1.0f / fmaxf(sqrtf(n0 * n0 + n1 * n1 + n2 * n2), 1e-12f); n *= inv` (F.normalize): the sum of
    squares 3 EPS, sqrtf halves that and adds 1 (2.5 EPS), the clamp is exact, the reciprocal and the product 1 EPS each:
    the kernel returns f(n') (1 + e) with f(x) = x / max(|x|, c), c = fl32(1e-12), |e| <= 4.5 EPS.  f is Lipschitz near x
    with constant 2 / max(|x|, c): |f(x') - f(x)| <= 2 |x' - x| / max(|x|, c) (x and x' on either side of the clamp
    included).  With the vector interpolation error |n' - n| <= 7 EPS |A| (A = normal_abs):
    normal_map: Dn = 14 EPS |A| / max(|n|, c) + 5 EPS (as a vector norm, hence per component).  Where |n| is at the
    level of its own rounding (cancelling normals) the bound is vacuous, as it should be; where n is exactly 0 (all three
    normals 0) both are exactly 0.
  * normal_map_cam, `c0 = R[0] * n0 + R[1] * n1 + R[2] * n2`, normalised again: the rows of R (a float32 rotation, ||R|| <=
    1 + 2 EPS) map the normal's error Dn to <= Dn (1 + 2 EPS); three products and two additions of terms summing to <= |R_i|
    |n| <= 1 add <= 3 EPS per component, 5.2 EPS as a vector; the second normalisation doubles it over max(|R n|, c) and
    adds 4.5 EPS:  normal_map_cam: 2 (Dn + 6 EPS) / max(|n|, c) + 5 EPS, n the reference's normalised normal.
  * position_map_cam, `R[0] * p0 + R[1] * p1 + R[2] * p2 + T[0]`: the error 7 EPS * A_j of p_j times |R_ij|, plus three
    products and three additions of four terms (<= 4 EPS of their magnitudes):
    position_map_cam_i: sum_j |R_ij| 7 EPS A_j + 5 EPS (sum_j |R_ij p_j| + |T_i|).
NaN positions must match exactly; infinities must be equal; the bounds apply where both values are finite.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EPS = 2.0 ** -24
CLAMP = float(np.float32(1e-12))
PIPELINE_MAPS = ['face_index_map', 'alpha', 'uv_map', 'normal_map']       # pipeline.RNRPipeline._gb_maps
PREFILL_NAN = 0x7fa5a5a5                                                    # a NaN no kernel generates: unwritten pixels show


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def bits(a):
    """float32 bit patterns with NaNs canonicalised (the sign / payload of a generated NaN is unspecified: x86 and gfx950
    differ), as test_gpu_raster.bits."""
    a = np.ascontiguousarray(a)
    if a.dtype != np.float32:
        return a
    b = a.view(np.uint32).copy()
    b[np.isnan(a)] = 0x7fc00000
    return b


def raw_bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


# ------------------------------------------------------------------------------------------------
# meshes
# ------------------------------------------------------------------------------------------------
def _unit(rng, n):
    v = rng.standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _soup(rng, n, centre, r_lo, r_hi, size_lo, size_hi):
    """n triangles with their own vertices: centres at distance [r_lo, r_hi] from `centre`, edge lengths log-uniform in
    [size_lo, size_hi], random winding (about half of them are back faces in any view)."""
    c = centre + _unit(rng, n) * rng.uniform(r_lo, r_hi, (n, 1))
    size = np.exp(rng.uniform(np.log(size_lo), np.log(size_hi), (n, 1, 1)))
    return (c[:, None, :] + rng.standard_normal((n, 3, 3)) * size * 0.6).reshape(-1, 3)


def attr_mesh(seed=0):
    """A closed coarse sphere (shared vertices, zero-area pole faces), a soup of 700 triangles from sub-pixel to larger than
    the image's tiles, a cluster of 2300 overlapping large triangles (> 2048 candidates of one tile), two huge triangles
    (untrusted boxes, crossing the near plane) and a small last face, each soup face with vertices of its own.
    nv == nvt == nvn; f_vt_idx = perm_t[f_v_idx], f_vn_idx = perm_n[f_v_idx] with independent permutations.
    Returns (mesh dict of numpy arrays, vertex ids of the last face)."""
    from rnr_amd import scene
    rng = np.random.default_rng(seed)
    sph = scene.uv_sphere(12, 24)
    parts = [sph['v'].astype(np.float64),
             _soup(rng, 700, np.zeros(3), 1.05, 1.5, 0.004, 0.6),
             _soup(rng, 2300, np.array([0.25, 0.2, 0.3]), 0.0, 0.15, 0.5, 0.8),
             _soup(rng, 2, np.zeros(3), 0.0, 1.0, 30.0, 30.0),
             _soup(rng, 1, np.zeros(3), 1.1, 1.2, 0.3, 0.3)]
    v = np.concatenate(parts).astype(np.float32)
    nv0 = sph['v'].shape[0]
    n_soup = (v.shape[0] - nv0) // 3
    f_v = np.concatenate([sph['f_v_idx'], nv0 + np.arange(3 * n_soup).reshape(-1, 3)]).astype(np.int32)
    nv, nf = v.shape[0], f_v.shape[0]
    soup_faces = np.arange(sph['f_v_idx'].shape[0], nf - 1)            # faces with vertices of their own (not the last)
    perm_t, perm_n = rng.permutation(nv), rng.permutation(nv)
    f_vt, f_vn = perm_t[f_v].astype(np.int32), perm_n[f_v].astype(np.int32)

    # texture coordinates: [-1.5, 2.5], a sixth of the components exact integers, faces whose u is one integer at all three
    # corners (interpolated u within rounding of the seam) and faces straddling an integer
    vt = rng.uniform(-1.5, 2.5, (nv, 2))
    snap = rng.random((nv, 2)) < 1 / 6
    vt[snap] = rng.integers(-1, 3, int(snap.sum()))
    pick = rng.permutation(soup_faces)
    for k in pick[:60]:
        vt[f_vt[k], 0] = float(rng.integers(-1, 3))
    for k in pick[60:120]:
        m = float(rng.integers(-1, 3))
        vt[f_vt[k], 0] = [m - 0.03, m + 0.05, m]
    # vertex normals: random directions (not outward), lengths 0.2 ... 5; then per-face special cases
    vn = _unit(rng, nv) * np.exp(rng.uniform(np.log(0.2), np.log(5.0), (nv, 1)))
    for k in pick[120:170]:                                             # below 1e-6: F.normalize still makes them unit
        vn[f_vn[k]] = _unit(rng, 3) * rng.uniform(1e-9, 1e-7, (3, 1))
    for k in pick[170:200]:                                             # below the 1e-12 clamp: x / 1e-12
        vn[f_vn[k]] = _unit(rng, 3) * rng.uniform(2e-15, 2e-14, (3, 1))
    for k in pick[200:240]:                                             # exactly opposite: the sum cancels along a line
        d = _unit(rng, 1)[0] * rng.uniform(0.5, 2.0)
        vn[f_vn[k]] = [d, -d, 0.3 * _unit(rng, 1)[0] * rng.random()]
    for k in pick[240:260]:                                             # all zero: the normal is exactly 0
        vn[f_vn[k]] = 0.0
    mesh = {'v': v, 'vt': vt.astype(np.float32), 'vn': vn.astype(np.float32), 'f_v_idx': f_v, 'f_vt_idx': f_vt,
            'f_vn_idx': f_vn}
    return mesh, f_v[-1].copy()


_MESHES = {}


def get_mesh(kind):
    """(mesh, last-face vertex ids or None), cached per session."""
    if kind not in _MESHES:
        from rnr_amd import scene
        if kind == 'attr':
            _MESHES[kind] = attr_mesh(0)
        else:
            nlat, nlon = {'sphere_coarse': (12, 24), 'sphere': (128, 256)}[kind]
            _MESHES[kind] = (scene.uv_sphere(nlat, nlon), None)
    return _MESHES[kind]


# ------------------------------------------------------------------------------------------------
# bounds (module docstring)
# ------------------------------------------------------------------------------------------------
def bounds(ref, pose):
    """Per-pixel bounds [N,S,S,k] (float64) of |kernel - reference| for the interpolated maps."""
    R = pose[:, :3, :3].double()
    t = pose[:, :3, 3].double()
    nmag = ref['normal_raw'].norm(dim=-1, keepdim=True).clamp(min=CLAMP)
    Dn = 14 * EPS * ref['normal_abs'].norm(dim=-1, keepdim=True) / nmag + 5 * EPS
    nu = ref['normal_map'].norm(dim=-1, keepdim=True).clamp(min=CLAMP)
    P = 7 * EPS * ref['position_abs']
    Rabs = R.abs()
    pc = (torch.einsum('nij,nhwj->nhwi', Rabs, P) +
          5 * EPS * (torch.einsum('nij,nhwj->nhwi', Rabs, ref['position_map'].abs()) + t.abs()[:, None, None, :]))
    return {'uv_map': 7 * EPS * ref['uv_abs'] + EPS,
            'normal_map': Dn.expand(ref['normal_map'].shape),
            'normal_map_cam': (2 * (Dn + 6 * EPS) / nu + 5 * EPS).expand(ref['normal_map'].shape),
            'position_map': P,
            'position_map_cam': pc}


def check_against_reference(got, ref, pose, tag):
    """got: dict name -> CPU tensor [N,S,S(,k)] of the kernel; ref: gbuffer64.rasterizer_forward."""
    for k in ['face_index_map', 'alpha', 'depth', 'raw_weight_map']:
        assert np.array_equal(bits(got[k].numpy()), bits(ref[k].numpy())), (tag, k)
    assert np.array_equal(bits(got['weight_map'].numpy()), bits(ref['weight_map32'].numpy())), (tag, 'weight_map')
    tol = bounds(ref, pose)
    for k, b in tol.items():
        g, r = got[k].double(), ref[k]
        gn, rn = torch.isnan(g), torch.isnan(r)
        assert torch.equal(gn, rn), (tag, k, int((gn != rn).sum()))
        ginf, rinf = torch.isinf(g), torch.isinf(r)
        assert torch.equal(ginf, rinf) and torch.equal(g[ginf], r[rinf]), (tag, k)
        fin = torch.isfinite(g) & torch.isfinite(r)
        d = (g - r).abs()
        if k == 'uv_map':
            assert bool(((g[fin] >= 0) & (g[fin] <= 1)).all()), (tag, 'uv_map outside [0, 1]')
            d = torch.minimum(d, 1.0 - d)             # both in [0, 1]: compared modulo 1
        bad = fin & ~(d <= b)
        assert not bool(bad.any()), (tag, k, int(bad.sum()), float(d[bad].max()), float(b[bad][d[bad].argmax()]))


# ------------------------------------------------------------------------------------------------
# calls
# ------------------------------------------------------------------------------------------------
def prefilled(maps, N, S):
    from rnr_amd import ops
    out = {}
    for m in maps:
        dt, tail = ops.GBUFFER_MAPS[m]
        if dt == torch.int32:
            out[m] = torch.full((N, S, S) + tail, -7, dtype=torch.int32, device=DEV)
        else:
            out[m] = torch.full((N, S, S) + tail, PREFILL_NAN, dtype=torch.int32, device=DEV).view(torch.float32)
    return out


def run_case(kind, S, view_ids, near, far, radius, zero_last):
    from rnr_amd import _lib, ops, scene
    from oracle import gbuffer64 as g64
    mesh, last = get_mesh(kind)
    N = len(view_ids)
    dm = ops.DeviceMesh(mesh['v'], mesh['vt'], mesh['vn'], mesh['f_v_idx'], mesh['f_vt_idx'], mesh['f_vn_idx'], DEV)
    views = scene.spiral_views(S, view_ids, radius=radius)
    K, pose = T(views['proj']).to(DEV), T(views['pose']).to(DEV)
    # the product's sequence: projection and workspace clearing in one launch, then the raster with four maps
    ws = torch.empty(_lib.load().rnr_gbuffer_workspace_bytes(N, dm.num_faces, S), dtype=torch.uint8, device=DEV)
    v_uvz = torch.empty(N, dm.num_vertices, 3, device=DEV)
    ops.frame_prepare(dm, K, pose, S, v_uvz=v_uvz, workspace=ws)
    if zero_last:
        v_uvz[:, torch.from_numpy(last.astype(np.int64)).to(DEV), 2] = 0.0
    prep = ops.rasterize_gbuffer(dm, v_uvz, None, S, near, far, maps=PIPELINE_MAPS, out=prefilled(PIPELINE_MAPS, N, S),
                                 workspace=ws, prepared=True)
    full = ops.rasterize_gbuffer(dm, v_uvz, pose, S, near, far, out=prefilled(list(ops.GBUFFER_MAPS), N, S))
    alone = {m: ops.rasterize_gbuffer(dm, v_uvz, pose, S, near, far, maps=[m], out=prefilled([m], N, S))[m]
             for m in ops.GBUFFER_MAPS}
    torch.cuda.synchronize()
    for m in PIPELINE_MAPS:
        assert torch.equal(raw_bits(prep[m]), raw_bits(full[m])), ('prepared', m)
    for m in ops.GBUFFER_MAPS:
        assert torch.equal(raw_bits(alone[m]), raw_bits(full[m])), ('alone', m)
    mesh_t = {k: T(x) for k, x in mesh.items()}
    ref = g64.rasterizer_forward(mesh_t, v_uvz.cpu(), pose.cpu(), S, near, far)
    got = {m: x.cpu() for m, x in full.items()}
    return got, ref, pose.cpu()


# (mesh, S, views, near, far, camera radius, last face at z = 0)
CASES = [
    ('attr', 17, [5], 0.0, 1e5, 3.5, False),                        # one tile and a one-pixel partial row / column
    ('attr', 33, [5, 130, 290], 0.0, 1e5, 3.5, True),              # background NaN (splat path)
    ('attr', 50, [20, 60, 200, 400, 610], -1.0, 1e5, 3.5, False),   # binning path, 5 views
    ('attr', 64, [40, 170, 333], 3.1, 3.9, 3.5, False),            # faces clipped by near and by far
    ('attr', 100, [77], -1.0, 1e5, 3.5, True),                      # background NaN (binning path)
    ('attr', 130, [1, 90, 180, 270, 360], 0.0, 1e5, 3.0, False),    # 130 = 8 * 16 + 2
    ('sphere_coarse', 130, [5, 150, 300], 0.0, 1e5, 1.9, False),    # faces far above 256 pixels, pole faces
    ('sphere', 64, [12, 250], 0.0, 1e5, 3.0, False),                # N * nf = 131 072: four lanes per face
    ('sphere', 100, [3, 200, 420], 0.0, 1e5, 3.0, False),           # N * nf = 196 608: one lane per face
    ('sphere', 512, [37], 0.0, 1e5, 3.0, False),                    # the benchmark's view size
]


@pytest.mark.parametrize('case', CASES, ids=lambda c: '%s_S%d_N%d_near%g%s' % (c[0], c[1], len(c[2]), c[3],
                                                                               '_zlast' if c[6] else ''))
def test_gbuffer_sweep_vs_float64(case):
    """rasterize_gbuffer (all ten maps, a pose per view), the product's frame_prepare + prepared four-map call and each map
    requested alone, against gbuffer64 (module docstring for what is exact and the bounds of the rest)."""
    kind, S, view_ids, near, far, radius, zero_last = case
    got, ref, pose = run_case(kind, S, view_ids, near, far, radius, zero_last)
    check_against_reference(got, ref, pose, kind)
    fim = ref['face_index_map']
    cov = float((fim >= 0).double().mean())
    assert cov > 0.1, cov                                           # the views see the mesh
    bg = fim < 0
    if bool(bg.any()):          # background: 0 weights, or NaN behind a last face at z = 0
        assert bool(torch.isnan(ref['uv_map'][bg]).all()) == zero_last
    else:
        assert kind == 'sphere_coarse'                              # the close-up fills the image


def test_dropin_rasterizer_batch_vs_float64(tmp_path):
    """network.Rasterizer (the drop-in module) at N = 3 on the attribute mesh read back from an OBJ file: the 14 outputs of
    network.py:214 view by view — the G-buffer maps against gbuffer64 as in the sweep, the mesh gathers (faces_v_idx, faces_v,
    faces_vt) exactly, v_uvz and v_front_mask (view 0 only, as the reference) exactly against the float32 oracle."""
    import network
    from oracle import gbuffer64 as g64
    from oracle import rnr_oracle as orc
    from rnr_amd import ops, scene
    mesh, _ = get_mesh('attr')
    fp = str(tmp_path / 'attr.obj')
    scene.write_obj(fp, mesh)
    S = 50
    ras = network.Rasterizer(fp, S).to(DEV)
    m = {'v': ras.vertices[0].cpu(), 'vt': ras.vertices_texcoords[0].cpu(), 'vn': ras.vertices_normals[0].cpu(),
         'f_v_idx': ras.faces[0].cpu(), 'f_vt_idx': ras.faces_vt_idx[0].cpu(), 'f_vn_idx': ras.faces_vn_idx[0].cpu()}
    for k in m:                                                     # %.9g round-trips float32: the OBJ is the mesh
        assert np.array_equal(m[k].numpy(), mesh[k]), k
    views = scene.spiral_views(S, [8, 140, 275], radius=3.5)
    proj, pose = T(views['proj']).to(DEV), T(views['pose']).to(DEV)
    with torch.no_grad():
        out = ras(proj, pose, None, None, None)
    assert len(out) == 14
    v_ndc = ops.project_vertices(ras.vertices[0].contiguous(), proj, pose[:, :3, :3].contiguous(),
                                 pose[:, :3, 3].contiguous(), S)
    torch.cuda.synchronize()
    names = ['uv_map', 'alpha', 'face_index_map', 'weight_map', 'faces_v_idx', 'normal_map', 'normal_map_cam', 'faces_v',
             'faces_vt', 'position_map', 'position_map_cam', 'depth', 'v_uvz', 'v_front_mask']
    o = dict(zip(names, [x.cpu() for x in out]))
    o32 = orc.rasterizer_forward(m, proj.cpu(), pose.cpu(), S, v_uvz_ndc=v_ndc.cpu())
    for k in ['faces_v_idx', 'faces_v', 'faces_vt', 'v_uvz', 'v_front_mask']:
        assert tuple(o[k].shape) == tuple(o32[k].shape), k
        assert np.array_equal(bits(o[k].numpy()), bits(o32[k].numpy())), k
    for i in range(3):
        ref = g64.rasterizer_forward(m, v_ndc[i:i + 1].cpu(), pose[i:i + 1].cpu(), S)
        got = {k: o[k][i:i + 1] for k in ['uv_map', 'alpha', 'face_index_map', 'normal_map', 'normal_map_cam', 'position_map',
                                           'position_map_cam']}
        got['weight_map'] = o['weight_map'][i:i + 1, ..., 0]
        got['depth'] = o['depth'][i:i + 1, ..., 0]
        got['raw_weight_map'] = ref['raw_weight_map']             # not among the 14 outputs
        check_against_reference(got, ref, pose[i:i + 1].cpu(), 'view%d' % i)
