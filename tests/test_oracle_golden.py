"""Pins the ORACLE (oracle/) to the reference: every function is checked against vectors produced by the
reference's own code (tests/golden/make_golden.py).  CPU only.

Tolerances: integer / index outputs and the C rasterizer's float maps are bit-exact; torch-CPU float32
restatements match the reference's torch-CPU float32 to <= 1e-5 abs (they run the same ATen kernels in a
possibly different association order)."""
import numpy as np
import pytest
import torch

from oracle import raster as oras
from oracle import rnr_oracle as orc


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def T(x):
    return torch.from_numpy(np.asarray(x))


@pytest.mark.parametrize('name', ['raster_soup64', 'raster_soup50', 'raster_soup64_nearfar', 'raster_sphere128'])
def test_raster_c_bit_exact(golden, name):
    g = golden(name)
    r = oras.face_index_map(g['faces'], int(g['image_size']), float(g['near']), float(g['far']))
    assert np.array_equal(r['face_index_map'], g['face_index_map'])
    for k in ['faces_inv', 'weight_map', 'depth_map', 'face_inv_map']:
        assert np.array_equal(bits(r[k]), bits(g[k])), k
    cov = g['face_index_map'] >= 0
    assert cov.any()
    w = g['weight_map'][cov]
    ok = np.isfinite(w).all(-1)
    assert np.allclose(w[ok].sum(-1), 1.0, atol=1e-6)     # known-answer property


@pytest.mark.parametrize('name', ['raster_soup64', 'raster_soup50', 'raster_soup64_nearfar', 'raster_sphere128'])
def test_raster_index_map_independent_of_fma_contraction(golden, name):
    """nvcc builds the reference with --fmad=true; the `_fma` fixtures (kernel bodies built -ffp-contract=fast -mfma)
    show the integer output is the same as without contraction, and the oracle reproduces it."""
    g, gf = golden(name), golden(name + '_fma')
    assert int(gf['index_flips']) == 0
    assert np.array_equal(g['face_index_map'], gf['face_index_map_fma'])
    r = oras.face_index_map(g['faces'], int(g['image_size']), float(g['near']), float(g['far']))
    assert np.array_equal(r['face_index_map'], gf['face_index_map_fma'])


def test_raster_sphere512_fma_fixture(golden):
    """Bench-size case: both reference builds agree on all 262 144 pixels; the C oracle agrees with them."""
    from rnr_amd import scene
    gf = golden('raster_sphere512_fma')
    assert int(gf['index_flips']) == 0
    assert np.array_equal(gf['face_index_map_nofma'], gf['face_index_map_fma'])
    idx = scene.uv_sphere(128, 256)['f_v_idx']
    faces = gf['v_uvz'][:, idx.astype(np.int64)]
    r = oras.face_index_map(faces, 512, 0.0, 1e5)
    assert np.array_equal(r['face_index_map'], gf['face_index_map_fma'])


def test_oracle_frame512_nf64_vs_reference_run(golden):
    """The oracle at the BENCHMARKED size against a reference-run frame (fixture frame512_nf64: the reference's own modules
    on bench.py's scene, 65 536 faces, C = 24, nf0 = 64, 512^2, spiral view 111): the restatement is pinned where the HIP
    path is measured, not only at 64^2 / nf0 = 4.  Integer witnesses equal, frame to 3e-5."""
    from rnr_amd import scene
    from rnr_amd.rays import ray_pivots
    g = golden('frame512_nf64')
    S, vid = int(g['image_size']), int(g['view'])
    torch.set_num_threads(min(32, __import__('os').cpu_count() or 8))
    mesh_t = {k: torch.as_tensor(v) for k, v in scene.uv_sphere(128, 256).items()}
    views = {k: torch.from_numpy(v) for k, v in scene.spiral_views(S, [vid]).items()}
    basis = torch.from_numpy(orc.sh_basis(10, orc.lp_recon_dirs().numpy()).astype(np.float32))
    lp = orc.reconstruct_lp(torch.from_numpy(scene.synthetic_sh_coeff(2, 10, 1))[0], basis)[None]
    res = orc.render_frame(mesh_t, views, S, scene.synthetic_textures(512, int(g['tex_ch']), 4, 0),
                           scene.unet_state_dict(108, 78, int(g['nf0']), 5, 0), lp, ray_pivots(6, 2, 5), ray_pivots(6, 2, 10))
    img = res['image']
    oy, ox = [int(x) for x in g['crop_origin']]
    assert float((img[:, :, ::4, ::4] - torch.from_numpy(g['image_stride4'])).abs().max()) <= 3e-5
    assert float((img[:, :, oy:oy + 128, ox:ox + 128] - torch.from_numpy(g['image_crop'])).abs().max()) <= 3e-5
    assert np.allclose(img.double().sum(dim=(0, 2, 3)).numpy(), g['image_sum'], rtol=1e-5)


def test_raster_sphere512_worst_fma_view(golden):
    """The view of the 200-view FMA sweep (tests/fma_sweep_report.json) where contraction moves the most face indices: the
    g++ and clang++ contracted builds of the reference's kernel bodies differ from the non-contracted one (and possibly
    from each other) at a handful of pixels.  The C oracle is the NON-contracted evaluation, exactly."""
    from rnr_amd import scene
    gf = golden('raster_sphere512_worst_fma')
    flips = int(gf['index_flips'])
    assert flips > 0 and flips == int((gf['face_index_map_nofma'] != gf['face_index_map_fma']).sum())
    assert flips <= 16 and int(gf['index_flips_clang']) <= 16            # single pixels, not regions
    idx = scene.uv_sphere(128, 256)['f_v_idx']
    faces = gf['v_uvz'][:, idx.astype(np.int64)]
    r = oras.face_index_map(faces, 512, 0.0, 1e5)
    assert np.array_equal(r['face_index_map'], gf['face_index_map_nofma'])
    # what flips: single pixels where a degenerate pole face of the UV sphere (two coincident vertices: an ill-conditioned
    # barycentric inverse, inf / NaN weights) wins or loses against the background or a neighbour depending on how a*b+c is
    # rounded — 3 of the 4 here are background <-> pole-face pixels, 1 is a regular face <-> pole-face pixel
    a, b = gf['face_index_map_nofma'], gf['face_index_map_fma']
    nf = 65536
    pole = lambda f: ((f >= 0) & (f < 512)) | (f >= nf - 512)                       # the two pole fans of uv_sphere(128, 256)
    fa, fb = a[a != b], b[a != b]
    assert (pole(fa) | pole(fb)).all()              # every flip has a degenerate pole face on one side


def test_raster_texture_sampling_bit_exact(golden):
    g = golden('raster_texsample32')
    r = oras.texture_sampling(g['faces'], g['textures'], g['face_index_map'], g['weight_map'], g['depth_map'],
                              int(g['image_size']), float(g['eps']))
    assert np.array_equal(r['sampling_index_map'], g['sampling_index_map'])
    assert np.array_equal(bits(r['rgb_map']), bits(g['rgb_map']))
    assert np.array_equal(bits(r['sampling_weight_map']), bits(g['sampling_weight_map']))


@pytest.mark.parametrize('name', ['raster_bwd_soup48', 'raster_bwd_soup64_ts2'])
def test_raster_backward_c_bit_exact(golden, name):
    """Backward kernels (rasterize_cuda_kernel.cu:244-592): the C restatement reproduces the reference kernels' serial
    run bit for bit (pixel map: fixed accumulation order; textures / depth: the serial order of the golden run)."""
    from oracle import raster as oras
    g = golden(name)
    S, eps, nf = int(g['image_size']), float(g['eps']), g['faces'].shape[1]
    for tag, rr, ra in [('both', 1, 1), ('alpha', 0, 1), ('rgb', 1, 0)]:
        o = oras.backward_pixel_map(g['faces'], g['face_index_map'], g['rgb_map'], g['alpha_map'], g['grad_rgb_map'],
                                    g['grad_alpha_map'], S, eps, rr, ra)
        assert np.array_equal(o.view(np.uint32), g['grad_faces_pixel_' + tag].view(np.uint32)), tag
    o = oras.backward_textures(g['face_index_map'], g['sampling_weight_map'], g['sampling_index_map'], g['grad_rgb_map'],
                               nf, int(g['texture_size']))
    assert np.array_equal(o, g['grad_textures'])
    o = oras.backward_depth_map(g['faces'], g['depth_map'], g['face_index_map'], g['face_inv_map'], g['weight_map'],
                                g['grad_depth_map'], S)
    assert np.array_equal(o, g['grad_faces_depth'])
    assert np.abs(g['grad_faces_pixel_both']).max() > 1 and np.abs(g['grad_faces_depth']).max() > 1      # not vacuous


def test_texture_kernels_c_bit_exact(golden):
    """load_textures / create_texture_image restatements vs the reference kernels' outputs (serial shim run)."""
    from oracle import raster as oras
    g = golden('load_textures40')
    for w in range(4):
        for b in (1, 0):
            t, f = oras.load_textures(g['image'], g['faces_uv'], g['textures_in'], g['is_update'], w, b)
            assert np.array_equal(t, g['textures_w%d_b%d' % (w, b)]), (w, b)
            assert np.array_equal(f, g['faces_w%d' % w]), w
    skipped = g['is_update'] == 0
    assert skipped.any() and np.all(g['textures_w0_b1'][skipped] == 0.5)          # untouched faces keep their cubes
    g = golden('create_texture_image')
    for tag in 'ab':
        img = oras.create_texture_image(g['vertices_' + tag], g['textures_' + tag], g['image_' + tag].shape[:2], float(g['eps']))
        assert np.array_equal(img, g['image_' + tag]), tag


def test_projection(golden):
    """Without distortion bit for bit.  With distortion the reference's sqrt and r ** 4, r ** 6 went through the recording
    host's libraries (MKL's sqrt, vectorised pow), which round faithfully, not correctly, and differently per CPU; the oracle
    rounds them correctly on every host.  So every vertex must equal the oracle with each of r, r^4, r^6 moved by at most
    one ulp, and most of them with none moved."""
    import itertools
    g = golden('projection')
    a = orc.projection(T(g['vertices']), T(g['K']), T(g['R']), T(g['t']), torch.zeros(1, 5), int(g['orig_size']))
    assert torch.equal(a, T(g['out_nodist']))
    ref = T(g['out_dist'])
    same = {}
    for u in itertools.product((0, -1, 1), repeat=3):
        b = orc.projection(T(g['vertices']), T(g['K']), T(g['R']), T(g['t']), T(g['dist']), int(g['orig_size']),
                           T(g['offset']), T(g['scale']), ulps=u)
        same[u] = (b == ref).all(-1)
    assert torch.stack(list(same.values())).any(0).all()
    assert float(same[(0, 0, 0)].float().mean()) > 0.95


def _mesh(g):
    return {k: T(g['mesh_' + k]) for k in ['v', 'vt', 'vn', 'f_v_idx', 'f_vt_idx', 'f_vn_idx']}


def test_rasterizer_module(golden):
    g = golden('rasterizer_module64')
    mesh = _mesh(g)
    grt = T(g['global_RT'])
    # network.py:126-128
    v = torch.matmul(grt, torch.cat((mesh['v'], torch.ones(mesh['v'].shape[0], 1)), 1).t()).t()[:, :3]
    vn = torch.nn.functional.normalize(torch.matmul(grt[:3, :3], mesh['vn'].t()).t(), dim=1)
    assert torch.allclose(v, T(g['buf_vertices'])[0], atol=1e-6)
    mesh['v'], mesh['vn'] = T(g['buf_vertices'])[0], T(g['buf_vertices_normals'])[0]
    assert torch.allclose(vn, mesh['vn'], atol=1e-6)
    for i in range(2):
        out = orc.rasterizer_forward(mesh, T(g['proj'][i:i + 1]), T(g['pose'][i:i + 1]), int(g['image_size']))
        assert torch.equal(out['face_index_map'], T(g['view%d_face_index_map' % i]))
        assert torch.equal(out['alpha'], T(g['view%d_alpha' % i]))
        assert torch.equal(out['v_front_mask'], T(g['view%d_v_front_mask' % i]))
        assert torch.equal(out['faces_v_idx'], T(g['view%d_faces_v_idx' % i]))
        for k in ['uv_map', 'weight_map', 'normal_map', 'normal_map_cam', 'faces_v', 'faces_vt', 'position_map',
                  'position_map_cam', 'depth', 'v_uvz']:
            ref = T(g['view%d_%s' % (i, k)])
            assert out[k].shape == ref.shape, k
            assert torch.allclose(out[k], ref, atol=2e-5, rtol=1e-5), (k, (out[k] - ref).abs().max())
    assert (g['view0_alpha'] > 0).mean() > 0.2      # the sphere is actually visible (winding/cull sanity)


def test_rasterizer_module_on_reference_ndc_vertices(golden):
    """Same fixture, but the reference's own projected NDC vertices (captured at the nr.Renderer boundary) go straight
    into the oracle: no host matmul in between, hence the float maps must agree to the last bits of pointwise math."""
    g = golden('rasterizer_module64')
    mesh = _mesh(g)
    mesh['v'], mesh['vn'] = T(g['buf_vertices'])[0], T(g['buf_vertices_normals'])[0]
    for i in range(2):
        out = orc.rasterizer_forward(mesh, T(g['proj'][i:i + 1]), T(g['pose'][i:i + 1]), int(g['image_size']),
                                     v_uvz_ndc=T(g['view%d_v_ndc' % i]))
        assert torch.equal(out['face_index_map'], T(g['view%d_face_index_map' % i]))
        assert torch.equal(out['v_uvz'], T(g['view%d_v_uvz' % i]))
        for k in ['uv_map', 'weight_map', 'normal_map', 'position_map', 'depth']:
            ref = T(g['view%d_%s' % (i, k)])
            assert torch.allclose(out[k], ref, atol=1e-6, rtol=1e-6), (k, (out[k] - ref).abs().max())


def test_resize_area_restatement():
    """oracle.resize_area (cv2 INTER_AREA restated; cv2 parity unpinned): integer ratios == plain box mean; constant
    images stay constant for every ratio (weights sum to 1); shrink weights partition the source exactly."""
    rng = np.random.RandomState(3)
    img = rng.rand(24, 40, 3).astype(np.float32)
    assert np.abs(orc.resize_area(img, 6, 10) - img.reshape(6, 4, 10, 4, 3).mean((1, 3))).max() < 1e-6
    assert np.abs(orc.resize_area(img, 24, 20) - img.reshape(24, 20, 2, 3).mean(2)).max() < 1e-6
    for hw in [(7, 11), (23, 39), (48, 80), (30, 20), (5, 64)]:
        const = orc.resize_area(np.full((24, 40, 2), 0.75, np.float32), *hw)
        assert np.abs(const - 0.75).max() < 1e-6, hw
    out = orc.resize_area(img, 7, 11)
    assert abs(float(out.mean()) - float(img.mean())) < 1e-6        # fractional cells tile the source: mean preserved
    assert np.array_equal(orc.resize_area(img, 24, 40), img)         # identity


def test_interpolate_bilinear(golden):
    g = golden('bilinear')
    out = orc.interpolate_bilinear(T(g['data']), T(g['x']), T(g['y']))
    assert torch.allclose(out, T(g['out']), atol=1e-6)


def test_texture_mapper(golden):
    g = golden('texture_mapper')
    tex = [T(g['tex%d' % i]) for i in range(4)]
    assert torch.allclose(orc.texture_mapper(tex, T(g['uv']), T(g['sh']), 6), T(g['out_sh6']), atol=1e-6)
    assert torch.allclose(orc.texture_mapper(tex, T(g['uv']), T(g['sh']), 3), T(g['out_sh3']), atol=1e-6)
    assert torch.allclose(orc.texture_mapper(tex, T(g['uv']), None), T(g['out_nosh']), atol=1e-6)


def test_shading_geometry(golden):
    g = golden('shading_geometry64')
    tbn = orc.tbn_map(T(g['normal_map']), T(g['face_index_map']), T(g['faces_v'])[0], T(g['faces_vt'])[0])
    assert torch.allclose(tbn, T(g['tbn']), atol=1e-6)
    vd, vdc = orc.view_dir_map((64, 64), T(g['proj_inv']), T(g['R_inv']))
    assert torch.allclose(vd, T(g['view_dir']), atol=1e-6)
    assert torch.allclose(vdc, T(g['view_dir_cam']), atol=1e-6)
    Rs, piv = orc.ray_sampler_pivots(6, 2, 5)
    assert torch.allclose(Rs, T(g['Rs_spec']), atol=1e-7) and torch.allclose(piv, T(g['pivots_spec']), atol=1e-7)
    Rd, pivd = orc.ray_sampler_pivots(6, 2, 10)
    assert torch.allclose(Rd, T(g['Rs_diff']), atol=1e-7) and torch.allclose(pivd, T(g['pivots_diff']), atol=1e-7)
    alpha = T(g['alpha'])[..., None]
    vt = T(g['view_tangent'])
    d, uv, dt = orc.ray_sampler('reflect', piv, T(g['tbn']), vt, alpha)
    assert torch.allclose(d, T(g['rays_dir_spec']), atol=2e-6)
    assert torch.allclose(uv, T(g['rays_uv_spec']), atol=2e-6)
    assert torch.allclose(dt, T(g['rays_dir_tangent_spec']), atol=2e-6)
    d, uv, _ = orc.ray_sampler('diffuse', pivd, T(g['tbn']), vt, alpha)
    assert torch.allclose(d, T(g['rays_dir_diff']), atol=2e-6)
    assert torch.allclose(uv, T(g['rays_uv_diff']), atol=2e-6)
    assert torch.allclose(orc.spherical_mapping(T(g['sm_dirs'])), T(g['sm_uv']), atol=1e-7)
    assert torch.allclose(orc.spherical_mapping_inv(T(g['sm_inv_uv'])), T(g['sm_inv_dirs']), atol=1e-7)


def _sd(g):
    return {k[3:]: T(g[k]) for k in g.files if k.startswith('sd:')}


def test_unet(golden):
    g = golden('unet_nf4')
    y = orc.unet_forward(_sd(g), T(g['x']))
    assert torch.allclose(y, T(g['y']), atol=2e-5), (y - T(g['y'])).abs().max()
    g = golden('unet_dnr_nf4')
    y = orc.unet_forward(_sd(g), T(g['x']))
    assert torch.allclose(y, T(g['y']), atol=2e-5)


def test_ray_renderer(golden):
    g = golden('ray_renderer')
    out = orc.ray_renderer(T(g['albedo_specular']), T(g['rays_uv']), T(g['rays_lt']), T(g['lp']),
                           albedo_diffuse=T(g['albedo_diffuse']), num_ray_diffuse=13, seperate_albedo=True)
    for a, k in zip(out, ['out', 'out_specular', 'out_diffuse', 'ltt_specular', 'ltt_diffuse', 'rays_color']):
        assert torch.allclose(a, T(g[k]), atol=2e-6), k
    out = orc.ray_renderer(T(g['albedo_specular']), T(g['rays_uv']), T(g['rays_lt']), T(g['lp']))
    assert torch.allclose(out[0], T(g['out_nodiffuse']), atol=2e-6)


def test_sh_linear(golden):
    g = golden('sh_linear')
    assert torch.allclose(orc.reconstruct_sh(T(g['coeff']), T(g['basis'])), T(g['recon3']), atol=1e-5)
    assert torch.allclose(orc.reconstruct_sh(T(g['coeff'])[0], T(g['basis'])), T(g['recon2']), atol=1e-5)
    assert torch.allclose(orc.fit_sh_coeff(T(g['samples']), T(g['basis'])), T(g['fit3']), atol=1e-5)
    assert torch.allclose(orc.fit_sh_coeff(T(g['samples'])[0], T(g['basis'])), T(g['fit2']), atol=1e-5)


def test_sh_basis_independent_checks():
    """sh_basis is PARITY-UNPINNED vs pyshtools; check it against scipy's complex harmonics with the
    Condon-Shortley factor removed, the closed-form lmax = 2 table and the quadrature
    orthonormality the reference relies on (sph_harm.py:80-86)."""
    from scipy.special import sph_harm_y
    from rnr_amd import scene
    d = scene.sphere_samples(4096).astype(np.float64)
    B = orc.sh_basis(10, d)
    G = 4 * np.pi / d.shape[0] * B.T.dot(B)
    assert np.abs(G - np.eye(121)).max() < 5e-3
    theta = np.arctan2(np.hypot(d[:, 0], d[:, 1]), d[:, 2])
    phi = np.arctan2(d[:, 1], d[:, 0])
    col = 0
    for l in range(11):
        for m in range(-l, l + 1):
            y = sph_harm_y(l, abs(m), theta, phi)
            cs = (-1.0) ** abs(m)
            ref = y.real if m == 0 else (np.sqrt(2) * cs * (y.real if m > 0 else y.imag))
            assert np.abs(B[:, col] - ref).max() < 1e-9, (l, m)
            col += 1
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    table = np.stack([0.2820948 + 0 * x, 0.4886025 * y, 0.4886025 * z, 0.4886025 * x, 1.0925484 * x * y,
                      1.0925484 * y * z, 0.3153916 * (3 * z * z - 1), 1.0925484 * x * z,
                      0.5462742 * (x * x - y * y)], -1)
    dn = d / np.linalg.norm(d, axis=1, keepdims=True)
    assert np.abs(B[:, :9] - table).max() < 1e-6


def test_frame_assembly(golden):
    """test_rnr.py:303-377 end to end (channel order of the network input, rays_lt scaling, albedo slices)."""
    g = golden('frame64')
    gm = golden('rasterizer_module64')
    mesh = _mesh(gm)
    mesh['v'], mesh['vn'] = T(gm['buf_vertices'])[0], T(gm['buf_vertices_normals'])[0]
    views = {k: T(gm[k]) for k in ['proj', 'pose', 'proj_inv', 'R_inv']}
    tex = [T(g['tex%d' % i]) for i in range(4)]
    _, ps = orc.ray_sampler_pivots(6, 2, 5)
    _, pd = orc.ray_sampler_pivots(6, 2, 10)
    out = orc.render_frame(mesh, views, 64, tex, _sd(g), T(g['lp']), ps, pd)
    assert torch.allclose(out['sh_basis_map'], T(g['sh_basis_map']), atol=1e-6)
    assert torch.allclose(out['net_in'], T(g['net_in']).float(), atol=2e-3)       # stored as fp16
    assert torch.allclose(out['unet_out'], T(g['net_out']).float(), atol=2e-3)
    assert torch.allclose(out['image'], T(g['image']), atol=5e-5), (out['image'] - T(g['image'])).abs().max()
    assert orc.psnr(out['image'], T(g['image'])) > 80


def _circular_u_close(a, b, atol):
    """|a - b| <= atol for the u coordinate of the spherical mapping, allowing the 1.0 jump of atan2 at the seam only where the
    two evaluations put the direction on different sides of it (|z| at rounding level)."""
    d = (a - b).abs()
    return torch.minimum(d, (d - 1.0).abs()) <= atol


def test_shade64_pinned_to_oracle_and_fixtures(golden):
    """oracle/shade64.py (the float64 reference of the shading sweeps) against the float32 oracle and the reference-generated
    fixtures, at the fixtures' tolerances: float64 evaluation moves nothing beyond float32 rounding, and the float32 tap
    expressions it keeps are the reference's."""
    from oracle import shade64 as o64
    g = golden('bilinear')
    assert torch.allclose(o64.bilinear(T(g['data']), T(g['x']), T(g['y'])).float(), T(g['out']), atol=1e-6)
    g = golden('texture_mapper')
    tex = [T(g['tex%d' % i]) for i in range(4)]
    for sh_start, key in ((6, 'out_sh6'), (3, 'out_sh3')):
        got = o64.texture_mapper(tex, T(g['uv']), T(g['sh']), sh_start)
        assert torch.allclose(got.float(), T(g[key]), atol=1e-6), key
        assert torch.allclose(got.float(), orc.texture_mapper(tex, T(g['uv']), T(g['sh']), sh_start), atol=1e-6)
    assert torch.allclose(o64.texture_mapper(tex, T(g['uv'])).float(), T(g['out_nosh']), atol=1e-6)
    g = golden('shading_geometry64')
    tan = o64.face_tangents(T(g['faces_v'])[0], T(g['faces_vt'])[0])
    assert torch.allclose(tan.float(), orc.face_tangents(T(g['faces_v'])[0], T(g['faces_vt'])[0]), atol=1e-6)
    tbn = o64.tbn_map(T(g['normal_map']), T(g['face_index_map']), tan)
    assert torch.allclose(tbn.float(), T(g['tbn']), atol=1e-6)
    vd, vdc = o64.view_dir_map((64, 64), T(g['proj_inv']), T(g['R_inv']))
    assert torch.allclose(vd.float(), T(g['view_dir']), atol=1e-6) and torch.allclose(vdc.float(), T(g['view_dir_cam']), atol=1e-6)
    alpha = T(g['alpha'])
    for reflect, piv, tag in ((True, T(g['pivots_spec']), 'spec'), (False, T(g['pivots_diff']), 'diff')):
        d, uv, dt = o64.ray_sampler(reflect, piv, T(g['tbn']), T(g['view_tangent']), alpha)
        assert torch.allclose(d.float(), T(g['rays_dir_' + tag]), atol=2e-6), tag
        ref_uv = T(g['rays_uv_' + tag])
        assert _circular_u_close(uv[..., 0, :].float(), ref_uv[..., 0, :], 2e-6).all(), tag
        assert torch.allclose(uv[..., 1, :].float(), ref_uv[..., 1, :], atol=2e-6), tag
        if reflect:
            assert torch.allclose(dt.float(), T(g['rays_dir_tangent_spec']), atol=2e-6)
    assert torch.allclose(o64.spherical_uv(T(g['sm_dirs']), 0).float(), T(g['sm_uv']), atol=1e-7)
    g = golden('ray_renderer')
    out = o64.ray_renderer(T(g['albedo_specular']), T(g['rays_uv']), T(g['rays_lt']), T(g['lp']),
                           albedo_diffuse=T(g['albedo_diffuse']), num_ray_diffuse=13, seperate_albedo=True)
    for a, k in zip(out, ['out', 'out_specular', 'out_diffuse', 'ltt_specular', 'ltt_diffuse', 'rays_color']):
        assert torch.allclose(a.float(), T(g[k]), atol=2e-6), k
    out = o64.ray_renderer(T(g['albedo_specular']), T(g['rays_uv']), T(g['rays_lt']), T(g['lp']))
    assert torch.allclose(out[0].float(), T(g['out_nodiffuse']), atol=2e-6)
    g = golden('sh_linear')
    assert torch.allclose(o64.sh_reconstruct(T(g['basis']), T(g['coeff'])[0]).float(), T(g['recon2']), atol=1e-5)
    assert torch.allclose(o64.sh_fit(T(g['samples'])[0], T(g['basis'])).float(), T(g['fit2']), atol=1e-5)
    # the assembled network input of the reference frame (frame64: the reference's own run, stored as fp16) from the
    # reference G-buffer of view 0, and the float32 oracle on the same maps
    gf, gm = golden('frame64'), golden('rasterizer_module64')
    tex = [T(gf['tex%d' % i]) for i in range(4)]
    _, ps = orc.ray_sampler_pivots(6, 2, 5)
    _, pd = orc.ray_sampler_pivots(6, 2, 10)
    gb = {k: T(gm['view0_' + k]) for k in ['face_index_map', 'alpha', 'uv_map', 'normal_map', 'faces_v', 'faces_vt']}
    tan = o64.face_tangents(gb['faces_v'][0], gb['faces_vt'][0])
    o = o64.shade_inputs(gb['face_index_map'], gb['alpha'], gb['uv_map'], gb['normal_map'], tan, T(gm['proj_inv'][:1]),
                         T(gm['R_inv'][:1]), tex, ps, pd, 6)
    net_in = o['net_in'].permute(0, 3, 1, 2)
    assert torch.allclose(net_in.float(), T(gf['net_in'][:1]).float(), atol=2e-3)
    assert torch.allclose(o['sh_basis_map'].float(), T(gf['sh_basis_map'][:1]), atol=1e-6)
    o32 = orc.shade_inputs(gb, T(gm['proj_inv'][:1]), T(gm['R_inv'][:1]), tex, ps, pd)
    assert torch.allclose(net_in.float(), o32['net_in'], atol=2e-5)
    assert torch.allclose(o['neural_img'].float(), o32['neural_img'], atol=2e-5)
    assert _circular_u_close(o['rays_uv'][..., 0, :].float(), o32['rays_uv'][..., 0, :], 2e-5).all()
    assert torch.allclose(o['rays_uv'][..., 1, :].float(), o32['rays_uv'][..., 1, :], atol=2e-5)


def test_gbuffer64_pinned_to_oracle_and_fixture(golden):
    """oracle/gbuffer64.py (the float64 reference of the G-buffer sweep) against the float32 oracle and the reference-generated
    fixture: the C oracle's maps and the float32 weights identical, the float64 maps equal to float32 rounding.  Then the
    same geometry with its attributes scrambled, two views in one call: vt and vn rows permuted independently (index arrays
    remapped, so f_vt_idx, f_vn_idx and f_v_idx differ), vt stretched to [-1.5, 2.5], normals of random length and sign —
    what the fixture's sphere (one index array, vt in [0, 1], unit normals) cannot tell apart."""
    from oracle import gbuffer64 as g64
    g = golden('rasterizer_module64')
    mesh = _mesh(g)
    mesh['v'], mesh['vn'] = T(g['buf_vertices'])[0], T(g['buf_vertices_normals'])[0]
    S = int(g['image_size'])

    def close(a, b, atol, k):
        d = (a.double() - b.double().reshape(a.shape)).abs()
        if k == 'uv_map':
            d = torch.minimum(d, 1.0 - d)
        return bool((d <= atol).all())

    maps = ['uv_map', 'normal_map', 'normal_map_cam', 'position_map', 'position_map_cam', 'weight_map']
    for i in range(2):
        v, pose = T(g['view%d_v_ndc' % i]), T(g['pose'][i:i + 1])
        o = g64.rasterizer_forward(mesh, v, pose, S)
        r = orc.rasterizer_forward(mesh, T(g['proj'][i:i + 1]), pose, S, v_uvz_ndc=v)
        for k in ['face_index_map', 'alpha', 'raw_weight_map']:
            assert torch.equal(o[k], r[k]), k
        assert torch.equal(o['depth'], r['depth'][..., 0])
        assert torch.equal(o['weight_map32'], r['weight_map'][..., 0])
        for k in maps:
            assert close(o[k], r[k], 1e-6 * max(1.0, float(r[k].abs().max())), k), k
            assert close(o[k], T(g['view%d_%s' % (i, k)]), 1e-6 * max(1.0, float(r[k].abs().max())), k), k
    rng = np.random.default_rng(5)
    nv = mesh['v'].shape[0]
    pt, pn = torch.from_numpy(rng.permutation(nv)), torch.from_numpy(rng.permutation(nv))
    m2 = dict(mesh)
    m2['vt'] = torch.empty_like(mesh['vt'])
    m2['vt'][pt] = mesh['vt'] * 4.0 - 1.5
    scale = torch.from_numpy((np.exp(rng.uniform(np.log(1e-3), np.log(10.0), (nv, 1))) *
                              rng.choice([-1.0, 1.0], (nv, 1))).astype(np.float32))
    m2['vn'] = torch.empty_like(mesh['vn'])
    m2['vn'][pn] = mesh['vn'] * scale
    m2['f_vt_idx'], m2['f_vn_idx'] = pt[mesh['f_vt_idx'].long()].int(), pn[mesh['f_vn_idx'].long()].int()
    v = torch.cat([T(g['view%d_v_ndc' % i]) for i in range(2)])
    pose = T(g['pose'])
    o = g64.rasterizer_forward(m2, v, pose, S)
    r = orc.rasterizer_forward(m2, T(g['proj']), pose, S, v_uvz_ndc=v)
    assert torch.equal(o['weight_map32'], r['weight_map'][..., 0])
    # float32 rounding of the oracle's three-term sums and normalisations: relative to the magnitudes summed, and for the
    # normals to the normal's length (a direction from a short sum of long terms is only as good as their cancellation)
    cond_n = (o['normal_abs'].norm(dim=-1) / o['normal_raw'].norm(dim=-1).clamp(min=1e-12))[..., None]
    for k, atol in [('uv_map', 1e-6 * (o['uv_abs'] + 1)), ('position_map', 1e-6 * (o['position_abs'] + 1)),
                    ('normal_map', 1e-6 * (cond_n + 1)), ('normal_map_cam', 2e-6 * (cond_n + 1))]:
        assert close(o[k], r[k], atol, k), k
    assert float(o['uv_abs'].max()) > 1.5 and bool((o['normal_raw'].norm(dim=-1) < 0.1).any())    # the scramble is in effect


def _bn64_input(N, H, W, C, c_pad, seed):
    """float32 NHWC map with the channels a BatchNorm statistics test needs: mean/std 0 ... 1e4, a constant, an all-zero one."""
    g = torch.Generator().manual_seed(seed)
    ratios = [0.0, 1.0, 30.0, 1e3, 1e4]
    x = torch.zeros(N, H, W, c_pad)
    for c in range(C - 2):
        r = ratios[c % len(ratios)]
        x[..., c] = (torch.randn(N, H, W, generator=g) * 0.5 + 0.5 * r + 0.1 * c).float()
    x[..., C - 2] = 2.75            # constant: variance exactly 0
    x[..., C - 1] = 0.0             # all zero
    x[..., C:] = float('nan')       # padding channels are never read
    return x


def test_bn64_pinned_to_torch_batch_norm():
    """oracle/bn64.py against torch.nn.functional.batch_norm(training=True) in float64, per view and over the whole batch:
    y = scale * x + shift must equal torch's normalised output, and the statistics torch reports must match; every term is
    float64 on exact float32 inputs, so 1e-12 relative to the channel's magnitude (|mean| + std) covers both summation orders."""
    import torch.nn.functional as F
    from oracle import bn64
    N, H, W, C, cp = 3, 5, 7, 12, 16
    x = _bn64_input(N, H, W, C, cp, seed=1)
    g = torch.Generator().manual_seed(2)
    gamma = torch.rand(C, generator=g) * 2 - 0.5
    gamma[3] = 0.0
    gamma[4] = -1.25
    beta = torch.randn(C, generator=g)
    eps = 1e-5
    xd = x[..., :C].double().permute(0, 3, 1, 2)
    mag = xd.abs().amax(dim=(0, 2, 3))
    ref = bn64.per_view(x, C, gamma, beta, eps)
    for n in range(N):
        y = F.batch_norm(xd[n:n + 1], None, None, gamma.double(), beta.double(), training=True, eps=eps)
        got = ref['scale'][n][None, :, None, None] * xd[n:n + 1] + ref['shift'][n][None, :, None, None]
        assert torch.allclose(got, y, rtol=0, atol=1e-9), n
        assert torch.allclose(ref['mean'][n], xd[n].mean(dim=(1, 2)), rtol=1e-13, atol=1e-13 * float(mag.max()))
        assert torch.allclose(ref['var'][n], xd[n].var(dim=(1, 2), unbiased=False), rtol=1e-12, atol=1e-20)
    assert torch.equal(ref['var'][:, C - 2], torch.zeros(N, dtype=torch.float64))
    assert torch.equal(ref['s1'][:, C - 1], torch.zeros(N, dtype=torch.float64))
    assert torch.allclose(ref['s2'], (xd * xd).sum(dim=(2, 3)), rtol=1e-14)
    allb = bn64.batch_all(x, C, gamma, beta, eps)
    y = F.batch_norm(xd, None, None, gamma.double(), beta.double(), training=True, eps=eps)
    got = allb['scale'][None, :, None, None] * xd + allb['shift'][None, :, None, None]
    assert torch.allclose(got, y, rtol=0, atol=1e-9)
    assert allb['count'] == N * H * W and float(allb['var'][C - 2]) == 0.0


def test_bn64_running_buffers_pinned_to_torch_batchnorm2d():
    """bn64.batch_all's running_mean / running_var update (momentum 0.1, unbiased variance) against torch.nn.BatchNorm2d in
    float64 train mode, over two calls, with num_batches_tracked counting them; the float64 results agree to 1e-12."""
    from oracle import bn64
    N, H, W, C, cp = 2, 4, 6, 10, 16
    bn = torch.nn.BatchNorm2d(C, momentum=0.1).double().train()
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(C, generator=g))
        bn.running_mean.copy_(torch.randn(C, generator=g))
        bn.running_var.copy_(torch.rand(C, generator=g) + 0.1)
    rm, rv = bn.running_mean.clone(), bn.running_var.clone()
    for call in range(2):
        x = _bn64_input(N, H, W, C, cp, seed=10 + call)
        ref = bn64.batch_all(x, C, bn.weight.detach(), bn.bias.detach(), bn.eps, rm, rv, bn.momentum)
        with torch.no_grad():
            bn(x[..., :C].double().permute(0, 3, 1, 2))
        mag = 1.0 + bn.running_mean.abs() + bn.running_var
        assert torch.allclose(ref['running_mean'], bn.running_mean, rtol=0, atol=1e-12 * float(mag.max()))
        assert torch.allclose(ref['running_var'], bn.running_var, rtol=1e-12, atol=1e-12)
        rm, rv = ref['running_mean'], ref['running_var']
    assert int(bn.num_batches_tracked) == 2
