"""-m gpu: photographs in.  rnr_photo_prepare (8-bit interleaved -> [3,S,S] float32: / 255, square crop, INTER_AREA, ** gamma in one
launch) against its numpy restatement and against rnr_resize_area bit for bit; its memory guards and refusals;
dataio.ViewDataset(load_img=True) lining photograph and camera up exactly, also through the real rasterizer;
rnr_amd.capture.view_maps against the files rnr_amd.precompute.export_view_maps writes; and one training step fed by both.

The restatement: capture.crop_geometry, u8.astype(float32) / 255, the window's first three channels, oracle.resize_area,
np.power in float64 rounded to float32, transpose.  Tolerances: gamma = 1 within 2e-6 of it (what tests/test_gpu_lighting.py derives
for this resize at peak 1: same float32 weights, another summation order at most) and bit-equal to rnr_resize_area on the float
window; gamma = 2.2 within 1 float32 ulp (the float64 power's own error is far below half a float32 ulp, so only a tie can move the
rounding)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# (h, w, channels, S)
SWEEP = [(128, 160, 3, 64),     # landscape, integer ratio
         (53, 37, 4, 10),       # portrait, odd side, RGBA, fractional cells, y0 != 0
         (20, 31, 3, 32),       # enlarging branch
         (97, 131, 3, 8),       # twelve-pixel cells
         (33, 33, 3, 33),       # odd square: window 32 enlarged to 33
         (66, 67, 4, 33)]       # 1089 outputs: several workgroups with a ragged last one
SWEEP_IDS = ['%dx%dx%d-%d' % s for s in SWEEP]


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _photo(h, w, c):
    return np.random.RandomState(h * 131 + w * 7 + c).randint(0, 256, (h, w, c)).astype(np.uint8)


def _window(u8):
    """-> (crop (y0, x0, side, side), the float32 window [side,side,3] the reference resizes)."""
    from rnr_amd import capture
    _, _, y0, x0, side = capture.crop_geometry(u8.shape[0], u8.shape[1])
    f = u8.astype(np.float32) / 255.
    return (y0, x0, side, side), np.ascontiguousarray(f[y0:y0 + side, x0:x0 + side, :3])


def _restatement(u8, S, gamma):
    from oracle import rnr_oracle as orc
    _, win = _window(u8)
    r = orc.resize_area(win, S, S)
    if gamma != 1:
        r = np.power(r.astype(np.float64), gamma).astype(np.float32)
    assert np.isfinite(r).all()
    return np.ascontiguousarray(r.transpose(2, 0, 1))


# ------------------------------------------------------------------------------------------------
# 1. the 256 values
# ------------------------------------------------------------------------------------------------
def test_all_256_byte_values_are_numpys_quotients():
    from rnr_amd import ops
    vals = np.arange(256, dtype=np.uint8)
    src = np.stack([vals, vals[::-1], np.roll(vals, 77)], -1).reshape(16, 16, 3)
    out = ops.photo_prepare(T(src).to(DEV), (0, 0, 16, 16), (16, 16), 1.0).cpu().numpy()
    want = np.arange(256, dtype=np.float32) / np.float32(255)
    assert out.shape == (3, 16, 16) and out.dtype == np.float32
    for c in range(3):
        assert np.array_equal(_bits(out[c]), _bits(want[src[..., c]])), c


# ------------------------------------------------------------------------------------------------
# 2. size sweep
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', SWEEP, ids=SWEEP_IDS)
def test_size_sweep(shape):
    from rnr_amd import ops
    h, w, c, S = shape
    u8 = _photo(h, w, c)
    crop, win = _window(u8)
    dev = T(u8).to(DEV)
    got1 = ops.photo_prepare(dev, crop, (S, S), 1.0).cpu().numpy()
    via_resize = ops.resize_area(T(win).to(DEV), S, S).permute(2, 0, 1).contiguous().cpu().numpy()
    ref1 = _restatement(u8, S, 1.0)
    err1 = float(np.abs(got1 - ref1).max())
    nbits = int((_bits(got1) != _bits(via_resize)).sum())
    got22 = ops.photo_prepare(dev, crop, (S, S), 2.2).cpu().numpy()
    ref22 = _restatement(u8, S, 2.2)
    ulp = float((np.abs(got22.astype(np.float64) - ref22.astype(np.float64)) / np.spacing(np.abs(ref22)).astype(np.float64)).max())
    print('%s: gamma 1: %d elements differ from rnr_resize_area in bits, max |err| vs restatement %.3e; gamma 2.2: max %.2f ulp'
          % (shape, nbits, err1, ulp))
    assert got1.shape == (3, S, S) and np.isfinite(got1).all() and np.isfinite(got22).all()
    assert nbits == 0
    assert err1 <= 2e-6
    assert ulp <= 1.0
    # out=: the same bits into a caller's tensor
    out = torch.full((3, S, S), float('nan'), device=DEV)
    assert ops.photo_prepare(dev, crop, (S, S), 2.2, out=out) is out
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(got22))


# ------------------------------------------------------------------------------------------------
# 3. memory guards
# ------------------------------------------------------------------------------------------------
def _guarded_call(u8, S, gamma, override=None):
    from rnr_amd.testing import EntryCalls, In, Out
    crop, _ = _window(u8)
    args = dict(src=In(T(u8)), src_h=u8.shape[0], src_w=u8.shape[1], src_channels=u8.shape[2], crop_y0=crop[0], crop_x0=crop[1],
                crop_h=crop[2], crop_w=crop[3], gamma=gamma, dst=Out((3, S, S)), dst_h=S, dst_w=S)
    args.update(override or {})
    ec = EntryCalls(True)
    return ec, args


@pytest.mark.parametrize('shape', [SWEEP[1], SWEEP[2]], ids=[SWEEP_IDS[1], SWEEP_IDS[2]])
def test_memory_guards(shape):
    """dst carved from a sentinel-filled allocation one float off 16-byte alignment, src one byte off: the sentinels on both sides
    of both are unchanged, src is unchanged, and the values are those of the plain call."""
    from rnr_amd import ops
    h, w, c, S = shape
    u8 = _photo(h, w, c)
    ec, args = _guarded_call(u8, S, 2.2)
    ec.call('rnr_photo_prepare', **args)
    assert ec.dev['src'].data_ptr() % 2 == 1 and ec.dev['dst'].data_ptr() % 8 == 4
    assert ec.report() == {'src': None, 'dst': None}, ec.report()
    assert torch.equal(ec.dev['src'].cpu(), T(u8))
    plain = ops.photo_prepare(T(u8).to(DEV), _window(u8)[0], (S, S), 2.2).cpu().numpy()
    assert np.array_equal(_bits(ec.results()['dst'].numpy()), _bits(plain))


# ------------------------------------------------------------------------------------------------
# 4. refusals
# ------------------------------------------------------------------------------------------------
REFUSALS = {
    'channels=1': dict(src_channels=1), 'channels=2': dict(src_channels=2),
    'window above': dict(crop_y0=-1), 'window left': dict(crop_x0=-1),
    'window below': dict(crop_y0=1), 'window right': dict(crop_x0=12),         # 1 + 20 > 20 rows, 12 + 20 > 31 columns
    'gamma=0': dict(gamma=0.0), 'gamma<0': dict(gamma=-2.2), 'gamma=nan': dict(gamma=float('nan')), 'gamma=inf': dict(gamma=float('inf')),
    'dst off by two bytes': 'align',
    'src NULL': dict(src=None), 'dst NULL': dict(dst=None),
    'src_h=0': dict(src_h=0), 'src_w=0': dict(src_w=0), 'crop_h=0': dict(crop_h=0), 'crop_w=0': dict(crop_w=0),
    'dst_h=0': dict(dst_h=0), 'dst_w=0': dict(dst_w=0),
}


@pytest.mark.parametrize('tag', sorted(REFUSALS))
def test_refusals_launch_nothing(tag):
    """Refused with the function's name in rnr_last_error; dst still holds the sentinel and every guard is intact."""
    from rnr_amd import _lib
    from rnr_amd.testing import SENTINEL, Out
    u8 = _photo(20, 31, 3)                 # the valid call: window rows [0, 20), columns [5, 25) of 20 x 31, to 8 x 8
    over = REFUSALS[tag]
    if over == 'align':
        over = dict(dst=Out((3, 8, 8), align=(4, 2)))
    ec, args = _guarded_call(u8, 8, 1.0, over)
    rc = ec.call('rnr_photo_prepare', check=False, **args)
    err = _lib.load().rnr_last_error().decode()
    assert rc != 0, 'rnr_photo_prepare accepted %s' % tag
    assert 'rnr_photo_prepare' in err, err
    if tag.endswith('two bytes'):
        assert 'aligned' in err, err
    assert all(v is None for v in ec.report().values()), ec.report()
    if 'dst' in ec.dev:
        raw = ec.dev['dst'].cpu().view(-1).view(torch.uint8).numpy()
        word = np.frombuffer(SENTINEL.to_bytes(4, 'little'), np.uint8)
        assert np.array_equal(raw, np.tile(word, raw.size // 4)), 'dst was written'


# ------------------------------------------------------------------------------------------------
# 5. photograph and camera line up, exactly
# ------------------------------------------------------------------------------------------------
def _save_capture(root, calib, photos):
    """calib.mat and rgb0/<name>.png under root -> (calib path, image dir)."""
    import scipy.io
    from PIL import Image
    img_dir = os.path.join(root, 'rgb0')
    os.makedirs(img_dir, exist_ok=True)
    calib_fp = os.path.join(root, 'calib.mat')
    scipy.io.savemat(calib_fp, calib)
    for i, p in enumerate(photos):
        Image.fromarray(p).save(os.path.join(img_dir, '%05d.png' % i))
    return calib_fp, img_dir


def test_photograph_and_camera_line_up(golden, tmp_path):
    import dataio
    g = golden('dataio_views')
    calib = {k[6:]: g[k][:1] if k[6:] in ('poses', 'projs', 'img_hws', 'dist_coeffs') else g[k] for k in g.files
             if k.startswith('calib:')}
    calib['img_hws'] = np.array([[128, 160]])
    photo = np.zeros((128, 160, 3), np.uint8)
    photo[40:44, 56:60] = 255
    calib_fp, img_dir = _save_capture(str(tmp_path), calib, [photo])
    ds = dataio.ViewDataset(str(tmp_path), calib_fp, 'convert', [64, 64], 'all', load_img=True, img_dir=img_dir)
    v = ds.read_view(0)
    img = v['img_gt']
    assert img.dtype == torch.float32 and tuple(img.shape) == (3, 64, 64) and not img.is_cuda
    want = torch.zeros(3, 64, 64)
    want[:, 20:22, 20:22] = 1.0
    assert torch.equal(img, want)
    # the block's centre (row 42, column 58) in the photograph -> the resized image, by the camera's own offset and scale
    off, sc = v['offset'].numpy(), v['scale'].numpy()
    assert ((42 + off[0]) * sc[0], (58 + off[1]) * sc[1]) == (21.0, 21.0)
    assert ds[0][0]['img_fn'] == '00000.png' and torch.equal(ds[0][0]['img_gt'], want)


# ------------------------------------------------------------------------------------------------
# 6 - 8. through the real rasterizer
# ------------------------------------------------------------------------------------------------
CAM_KEYS = ['proj', 'pose', 'proj_inv', 'R_inv']


@pytest.fixture(scope='module')
def sphere_capture(tmp_path_factory):
    """The mesh and the two views of the rasterizer_module64 fixture as a capture on disk: calib.mat whose ORIGINAL intrinsics
    are chosen so that the crop arithmetic for a 128 x 160 photograph gives the fixture's proj back (doubled focal lengths,
    cx * 2 + 16, cy * 2), poses = pose . global_RT, and as photographs the rasterizer's 64^2 alpha of each view, every pixel 2 x 2,
    16 zero columns left and right, times 255."""
    import network
    from rnr_amd import scene
    root = str(tmp_path_factory.mktemp('sphere_capture'))
    gm = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'rasterizer_module64.npz'))
    obj = os.path.join(root, 'sphere.obj')
    scene.write_obj(obj, {k: gm['mesh_' + k] for k in ['v', 'vt', 'vn', 'f_v_idx', 'f_vt_idx', 'f_vn_idx']})
    ras = network.Rasterizer(obj_fp=obj, img_size=64, global_RT=T(gm['global_RT'])).to(DEV)
    cams = {k: T(gm[k]) for k in CAM_KEYS}
    with torch.no_grad():
        alpha = ras(proj=cams['proj'].to(DEV), pose=cams['pose'].to(DEV), dist_coeffs=None, offset=None, scale=None)[1]
    alpha = alpha.cpu()
    assert tuple(alpha.shape) == (2, 64, 64) and bool(((alpha == 0) | (alpha == 1)).all()) and 0.1 < float(alpha.mean()) < 0.9
    projs = gm['proj'].astype(np.float64).copy()
    projs[:, 0, 0] *= 2
    projs[:, 1, 1] *= 2
    projs[:, 0, 2] = projs[:, 0, 2] * 2 + 16
    projs[:, 1, 2] = projs[:, 1, 2] * 2
    calib = {'global_RT': gm['global_RT'].astype(np.float64), 'projs': projs,
             'poses': np.matmul(gm['pose'].astype(np.float64), gm['global_RT'].astype(np.float64)),
             'img_hws': np.array([[128, 160]] * 2), 'dist_coeffs': np.zeros((2, 5))}
    photos = []
    for a in alpha.numpy():
        p = np.zeros((128, 160), np.uint8)
        p[:, 16:144] = (np.repeat(np.repeat(a, 2, 0), 2, 1) * 255).astype(np.uint8)
        photos.append(np.stack([p, p, p], -1))
    calib_fp, img_dir = _save_capture(root, calib, photos)
    return dict(root=root, calib_fp=calib_fp, img_dir=img_dir, gm=gm, ras=ras, alpha=alpha, cams=cams)


def _sphere_dataset(sc, device):
    import dataio
    return dataio.ViewDataset(sc['root'], sc['calib_fp'], 'convert', [64, 64], 'all', load_img=True, img_dir=sc['img_dir'],
                              device=device)


def test_dataset_through_the_real_rasterizer(sphere_capture):
    sc = sphere_capture
    on_dev, on_cpu = _sphere_dataset(sc, DEV), _sphere_dataset(sc, None)
    assert len(on_dev) == len(on_cpu) == 2
    for i in range(2):
        v, c = on_dev[i][0], on_cpu[i][0]
        for k in CAM_KEYS:
            assert not v[k].is_cuda and v[k].dtype == torch.float32
            assert np.allclose(v[k].numpy(), sc['gm'][k][i], rtol=1e-6, atol=1e-6), (i, k)
            assert torch.equal(v[k], c[k])
        assert v['img_gt'].device == torch.device(DEV) and c['img_gt'].device.type == 'cpu'
        assert tuple(v['img_gt'].shape) == (3, 64, 64) and v['img_gt'].dtype == torch.float32
        for ch in range(3):
            assert np.array_equal(_bits(v['img_gt'][ch].cpu().numpy()), _bits(sc['alpha'][i].numpy())), (i, ch)
        assert torch.equal(v['img_gt'].cpu(), c['img_gt'])


MAP_SHAPES = {'TBN_map': (64, 64, 3, 3), 'uv_map': (64, 64, 2), 'sh_basis_map': (64, 64, 9), 'normal_map': (64, 64, 3),
              'view_dir_map': (64, 64, 3), 'view_dir_map_tangent': (64, 64, 3), 'alpha_map': (64, 64)}


def test_view_maps_are_what_export_view_maps_writes(sphere_capture, tmp_path):
    """Every key bit-equal to the array export_view_maps writes for that view (uv_map: uv - floor(uv) of the file; alpha_map: the
    rasterizer's own), and the N = 2 call bit-equal to the two N = 1 calls."""
    import scipy.io
    from rnr_amd import capture, precompute
    sc = sphere_capture
    cams = sc['cams']
    both = capture.view_maps(sc['ras'], *[cams[k] for k in CAM_KEYS])
    assert set(both) == set(MAP_SHAPES)
    differ = []
    for i in range(2):
        one = capture.view_maps(sc['ras'], *[cams[k][i:i + 1] for k in CAM_KEYS])
        out = str(tmp_path / ('precomp%d' % i))
        precompute.export_view_maps(sc['ras'], {k: cams[k][i:i + 1] for k in CAM_KEYS}, out, '00000')
        for key, shape in MAP_SHAPES.items():
            t = one[key]
            assert t.device == torch.device(DEV) and t.dtype == torch.float32 and tuple(t.shape) == (1,) + shape, key
            assert type(t) is torch.Tensor and tuple(both[key].shape) == (2,) + shape
            if not np.array_equal(_bits(both[key][i].cpu().numpy()), _bits(t[0].cpu().numpy())):
                differ.append('view %d %s: N = 2 differs from N = 1' % (i, key))
            if key == 'alpha_map':
                want = sc['alpha'][i].numpy()
            else:
                want = scipy.io.loadmat('%s/%s/00000.mat' % (out, key))[key]
                assert want.dtype == np.float32, key
                if key == 'uv_map':
                    want = want - np.floor(want)
            if not np.array_equal(_bits(t[0].cpu().numpy()), _bits(want)):
                d = np.abs(t[0].cpu().numpy().astype(np.float64) - want)
                differ.append('view %d %s: %d elements differ from the exported file, max |d| %.3e'
                              % (i, key, int((_bits(t[0].cpu().numpy()) != _bits(want)).sum()), float(np.nanmax(d))))
        uv = one['uv_map']
        assert float(uv.min()) >= 0.0 and float(uv.max()) < 1.0
    assert not differ, '\n' + '\n'.join(differ)


def test_one_training_step_from_the_capture(sphere_capture):
    """Dataset + view_maps feed the graph of train_rnr.py:512-618 on small modules: loss_g is finite and every live U-Net
    parameter, every texture level and the lighting coefficients receive a finite gradient that is not identically zero."""
    import network
    import sph_harm
    from rnr_amd import capture, losses
    sc = sphere_capture
    ds = _sphere_dataset(sc, DEV)
    views = [ds[i][0] for i in range(2)]
    batch = {k: torch.stack([v[k] for v in views]) for k in CAM_KEYS + ['img_gt']}
    maps = capture.view_maps(sc['ras'], *[batch[k] for k in CAM_KEYS])
    img_gt = batch['img_gt']
    assert img_gt.device == torch.device(DEV) and tuple(img_gt.shape) == (2, 3, 64, 64)
    N, H, W, C = 2, 64, 64, 16
    rng = torch.Generator().manual_seed(11)
    torch.cuda.manual_seed(11)
    tm = network.TextureMapper(16, C, 4, apply_sh=True)
    with torch.no_grad():
        for l, p in enumerate(tm.textures):
            p.copy_((0.2 + 0.8 * torch.rand(p.shape, generator=rng)) * (1.0 if l == 0 else 0.1))
    sampler, sampler_diffuse = network.RaySampler(2, 1, 5), network.RaySampler(2, 1, 10, mode='diffuse')
    R, nd = sampler.num_ray + sampler_diffuse.num_ray, sampler_diffuse.num_ray
    net = network.RenderingNet(nf0=4, in_channels=3 * R + 6 + C, out_channels=3 * R, num_down_unet=5, use_gcn=False)   # 64 -> 2 x 2
    net.train()
    l_dir = torch.nn.functional.normalize(torch.randn(3, 50, generator=rng), dim=0)
    lighting = network.LightingSH(l_dir, lmax=2, num_lighting=1, fix_params=False, lp_recon_h=16, lp_recon_w=32)
    with torch.no_grad():
        lighting.coeff.copy_(torch.randn(1, 9, 3, generator=rng) * 0.3 + 0.2)
    tm, net, lighting = tm.to(DEV), net.to(DEV).enable_hip_backward(), lighting.to(DEV)
    sampler, sampler_diffuse = sampler.to(DEV), sampler_diffuse.to(DEV)
    rr = network.RayRenderer(lighting, network.Interpolater())
    l_init, l_mask = torch.rand(50, 3, generator=rng).to(DEV), (torch.rand(50, generator=rng) > 0.4).to(DEV)

    alpha_map = maps['alpha_map'][:, None]                                                           # train_rnr.py:499
    neural = tm(maps['uv_map'], maps['sh_basis_map'], sh_start_ch=6)                                 # :512
    with torch.no_grad():
        a_hw1 = alpha_map.permute((0, 2, 3, 1)).contiguous()
        rays_dir, rays_uv, _ = sampler(maps['TBN_map'], maps['view_dir_map_tangent'], a_hw1)         # :517
        rays_dir_d, rays_uv_d, _ = sampler_diffuse(maps['TBN_map'], maps['view_dir_map_tangent'], a_hw1)
        rays_dir, rays_uv = torch.cat((rays_dir, rays_dir_d), dim=-1), torch.cat((rays_uv, rays_uv_d), dim=-1)
    assert rays_uv.shape[-1] == R
    net_in = torch.cat((rays_dir.permute((0, -1, -2, 1, 2)).reshape((N, -1, H, W)), maps['normal_map'].permute((0, 3, 1, 2)),
                        maps['view_dir_map'].permute((0, 3, 1, 2)), neural), dim=1)                  # :530
    rays_lt = (net(net_in, None).reshape((N, R, -1, H, W)) * 0.5 + 0.5) * 2.0                        # :534-536
    out = rr(neural[:, 3:6], rays_uv, rays_lt, lighting_idx=0, albedo_diffuse=neural[:, :3], num_ray_diffuse=nd,
             seperate_albedo=True)[0]                                                                # :539
    l_est = sph_harm.reconstruct_sh(lighting.get_lighting_params(0), lighting.basis_val)             # :562
    loss_g, terms = losses.training_objective(out, img_gt, alpha_map, rays_lt, tm, l_est, l_init, l_mask)
    loss_g.backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss_g)) and all(bool(torch.isfinite(v)) for v in terms.values()), (loss_g, terms)
    live = dict(net.net._live_params())
    assert len(live) >= 10
    named = [('unet ' + k, p) for k, p in live.items()] + [('texture level %d' % l, p) for l, p in enumerate(tm.textures)] + \
        [('coeff', lighting.coeff)]
    for name, p in named:
        assert p.grad is not None, name
        assert bool(torch.isfinite(p.grad).all()), name
        assert float(p.grad.abs().max()) > 0.0, name
