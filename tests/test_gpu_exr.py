"""-m gpu: OpenEXR in.  rnr_exr_unpack (chunk payloads -> raw scanlines: copy, or prefix sum mod 256 + interleave) against the numpy
decoder of tests/exr_ref.py byte for byte; rnr_photo_prepare_hdr (HALF / FLOAT source -> [3,h,w] float32: window, INTER_AREA,
** gamma) against numpy's float16 -> float32 for all 65 536 patterns and against rnr_resize_area on the restatement's float
window bit for bit; guard bands, tracers and refusals of both; ViewDataset / LightProbeStitcher / LightProbeDataset fed by .exr
files against the same arrays fed as float.

The one pattern the resize arithmetic does not hand through: -0 (0x8000).  resize_area_pixel accumulates from +0, and
(+0) + (-0 * 1) = +0 in IEEE arithmetic, in rnr_resize_area as in this kernel, so 'numpy's bits' and 'rnr_resize_area's bits'
cannot both hold there.  test_all_65536_half_values asserts numpy's bits for the other 65 535 patterns, +0 for that one, and
rnr_resize_area's bits for all of them.

gamma 2.2, 'the same pow': the float32 nearest to the device's float64 pow, which only the device evaluates — the reference value
is rnr_resize_area's output sent through the kernel's own identity path (window = size, interleaved float addressing), and
numpy's float64 power within 1 float32 ulp beside it, as tests/test_gpu_capture.py derives."""
import os

import numpy as np
import pytest
import torch

import exr_ref as er

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _radiance(h, w, seed, dtype=np.float32):
    """Positive radiance up to about 50, mostly below 1."""
    rng = np.random.RandomState(seed)
    return (rng.rand(h, w) ** 4 * 50 + 1e-3).astype(dtype)


def _unpack_file(fp):
    from rnr_amd import exr, ops
    header, payload, table = exr.load(fp)
    raw = ops.exr_unpack(torch.frombuffer(payload, dtype=torch.uint8).to(DEV), torch.tensor(table, dtype=torch.int64).to(DEV),
                         header.height * header.row_bytes)
    return header, raw


# ------------------------------------------------------------------------------------------------
# 1. all 65 536 half values
# ------------------------------------------------------------------------------------------------
def test_all_65536_half_values(tmp_path):
    from rnr_amd import ops
    halves = np.arange(65536, dtype=np.uint16).reshape(256, 256).view(np.float16)
    chans = {'R': halves, 'G': halves[::-1, ::-1].copy(), 'B': np.roll(halves, 77, 1)}
    fp = str(tmp_path / 'halves.exr')
    how = er.write(fp, chans, compression=er.ZIPS)               # one scanline per chunk
    assert len(how) == 256
    out = ops.read_exr(fp, DEV).cpu().numpy()
    assert out.shape == (3, 256, 256) and out.dtype == np.float32
    via_resize = ops.resize_area(T(np.stack([chans[k].astype(np.float32) for k in 'RGB'], -1)).to(DEV), 256, 256).cpu().numpy()
    for c, k in enumerate('RGB'):
        want = chans[k].astype(np.float32)
        nan = np.isnan(want)
        assert nan.sum() == 2046 and np.array_equal(np.isnan(out[c]), nan), k
        neg_zero = chans[k].view(np.uint16) == 0x8000
        assert neg_zero.sum() == 1
        same = _bits(out[c]) == _bits(want)
        assert same[~nan & ~neg_zero].all(), (k, int((~same[~nan & ~neg_zero]).sum()))
        assert _bits(out[c])[neg_zero][0] == 0, k                                   # +0: see the module docstring
        assert np.array_equal(_bits(out[c])[~nan], _bits(via_resize[..., c])[~nan]), k
        assert np.array_equal(np.isnan(via_resize[..., c]), nan), k


# ------------------------------------------------------------------------------------------------
# 2. unpack
# ------------------------------------------------------------------------------------------------
def _pass_bytes():
    from rnr_amd import _lib
    return _lib.EXR_PASS_BYTES


def test_unpack_chunk_lengths_around_one_pass():
    """One call, one row per length: 1, 2, 3 bytes, one below / at / one above the span of one workgroup pass, two passes and one
    over, several passes with an odd length; coded and copied rows alternate in a second set; destinations in decreasing order with
    16-byte gaps that must keep their fill."""
    from rnr_amd import ops
    P = _pass_bytes()
    assert P == 8192
    lengths = [1, 2, 3, 511, 512, P - 1, P, P + 1, 2 * P, 2 * P + 1, 5 * P + 333]
    rng = np.random.RandomState(7)
    rows, payload, want, pos = [], [], [], 0
    for coded in (1, 0):
        for n in lengths:
            raw = rng.randint(0, 256, n).astype(np.uint8).tobytes()
            data = er.encode_chunk(raw)[1] if coded else raw
            rows.append([pos, 0, n, coded])
            payload.append(data + b'\x5a' * 3)                   # sources at every alignment
            want.append(raw)
            pos += n + 3
    total = sum(r[2] + 16 for r in rows)
    dst = total
    for r in rows:                                               # decreasing destinations
        dst -= r[2] + 16
        r[1] = dst + 16
    out = torch.full((total,), 0xA5, dtype=torch.uint8, device=DEV)
    ops.exr_unpack(T(np.frombuffer(bytearray(b''.join(payload)), np.uint8)).to(DEV), torch.tensor(rows, dtype=torch.int64).to(DEV), out=out)
    got = out.cpu().numpy()
    for r, w in zip(rows, want):
        assert got[r[1]:r[1] + r[2]].tobytes() == w, r
        assert (got[r[1] - 16:r[1]] == 0xA5).all(), r
    # the decoder restated on the host agrees with the restatement used above
    from rnr_amd import exr
    assert exr.unpack_chunk(er.encode_chunk(want[6])[1]) == want[6]


def _file_cases():
    half = lambda h, w, s: _radiance(h, w, s, np.float16)
    smooth = lambda h, w: (np.add.outer(np.arange(h), np.arange(w)) * 0.125 + 1).astype(np.float16)
    rgb16 = lambda h, w: {k: half(h, w, i) for i, k in enumerate('RGB')}
    return {
        'zips-69x9': (rgb16(9, 69), dict(compression=er.ZIPS)),
        'zip-41x37': ({k: smooth(37, 41) for k in 'RGB'}, dict(compression=er.ZIP)),                # last chunk of 5 lines
        'none-37x21-window': (rgb16(21, 37), dict(compression=er.NONE, origin=(-3, 11))),
        'zip-mixed-storage-decreasing': ({'R': smooth(37, 31), 'G': smooth(37, 31).astype(np.float32), 'B': half(37, 31, 5),
                                          'A': smooth(37, 31), 'Z': np.arange(37 * 31, dtype=np.uint32).reshape(37, 31)},
                                         dict(compression=er.ZIP, decreasing=True, origin=(5, 7), force_raw=(1,))),
        'zips-noise-and-ramp-rows': ({k: np.concatenate([smooth(5, 64), half(4, 64, 9 + i)]) for i, k in enumerate('RGB')}, dict(compression=er.ZIPS)),
    }


@pytest.mark.parametrize('case', sorted(_file_cases()))
def test_unpack_files(case, tmp_path):
    chans, kw = _file_cases()[case]
    fp = str(tmp_path / (case + '.exr'))
    how = er.write(fp, chans, **kw)
    print(case, how)
    if case == 'zip-mixed-storage-decreasing':
        assert how == ['deflate', 'raw', 'deflate']
    if case == 'zips-noise-and-ramp-rows':
        assert how == ['deflate'] * 5 + ['raw'] * 4
    if case == 'zips-69x9':
        assert how == ['raw'] * 9
    if case == 'zip-41x37':
        assert how == ['deflate'] * 3
    want, info = er.raw_scanlines(fp)
    header, raw = _unpack_file(fp)
    assert (header.height, header.width, header.row_bytes) == (info['height'], info['width'], info['row_bytes'])
    assert raw.cpu().numpy().tobytes() == want.tobytes()


# ------------------------------------------------------------------------------------------------
# 3. prepare
# ------------------------------------------------------------------------------------------------
# (h, w, S): test_gpu_capture.SWEEP shrunk
SWEEP = [(32, 40, 16),      # landscape, integer ratio
         (53, 37, 10),      # portrait, odd side, fractional cells, y0 != 0
         (20, 31, 32),      # enlarging branch
         (39, 61, 4),       # wide cells (9.5 pixels)
         (33, 33, 33),      # odd square: window 32 enlarged to 33
         (34, 67, 33)]      # 1089 outputs: several workgroups with a ragged last one
LAYOUTS = ['half', 'half-float-half', 'interleaved-float']


def _source(h, w, layout, tmp_path):
    """-> (device byte buffer, row_bytes, channel layout, float32 [h,w,3] RGB the restatement decodes)."""
    from rnr_amd import _lib, exr
    if layout == 'interleaved-float':
        f = np.stack([_radiance(h, w, 20 + i) for i in range(3)], -1)
        lay = tuple((4 * k, 12, _lib.EXR_FLOAT) for k in range(3))
        return T(f).view(torch.uint8).reshape(-1).to(DEV), 12 * w, lay, f
    chans = {k: _radiance(h, w, 30 + i, np.float16) for i, k in enumerate('RGB')}
    if layout == 'half-float-half':                    # list order B (HALF), G (FLOAT), R (HALF): with odd w the G run starts at 2 mod 4
        chans['G'] = _radiance(h, w, 41, np.float32)
    fp = str(tmp_path / ('%s_%dx%d.exr' % (layout, h, w)))
    er.write(fp, chans, compression=er.ZIP)
    header, raw = _unpack_file(fp)
    lay = exr.rgb_layout(header)
    if layout == 'half-float-half' and w % 2:
        assert lay[1][0] % 4 == 2 and header.row_bytes % 4 == 0
    if layout == 'half' and w % 2:
        assert header.row_bytes % 4 == 2
    return raw, header.row_bytes, lay, er.rgb(fp)


@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('shape', SWEEP, ids=['%dx%d-%d' % s for s in SWEEP])
def test_prepare_sweep(shape, layout, tmp_path):
    from rnr_amd import _lib, capture, ops
    h, w, S = shape
    src, row_bytes, lay, f = _source(h, w, layout, tmp_path)
    _, _, y0, x0, side = capture.crop_geometry(h, w)
    win = np.ascontiguousarray(f[y0:y0 + side, x0:x0 + side])
    resized = ops.resize_area(T(win).to(DEV), S, S)                                          # [S,S,3]
    got1 = ops.photo_prepare_hdr(src, (h, w), row_bytes, lay, (y0, x0, side, side), (S, S), 1.0).cpu().numpy()
    assert got1.shape == (3, S, S) and np.isfinite(got1).all()
    assert np.array_equal(_bits(got1), _bits(resized.permute(2, 0, 1).cpu().numpy()))
    got22 = ops.photo_prepare_hdr(src, (h, w), row_bytes, lay, (y0, x0, side, side), (S, S), 2.2).cpu().numpy()
    ident = tuple((4 * k, 12, _lib.EXR_FLOAT) for k in range(3))
    same_pow = ops.photo_prepare_hdr(resized.contiguous().view(torch.uint8).reshape(-1), (S, S), 12 * S, ident, (0, 0, S, S), (S, S),
                                     2.2).cpu().numpy()
    assert np.array_equal(_bits(got22), _bits(same_pow))
    ref22 = np.power(resized.permute(2, 0, 1).cpu().numpy().astype(np.float64), 2.2).astype(np.float32)
    ulp = float((np.abs(got22.astype(np.float64) - ref22.astype(np.float64)) / np.spacing(np.abs(ref22)).astype(np.float64)).max())
    print(shape, layout, 'gamma 2.2: max %.2f ulp from the float64 power' % ulp)
    assert ulp <= 1.0
    out = torch.full((3, S, S), float('nan'), device=DEV)
    assert ops.photo_prepare_hdr(src, (h, w), row_bytes, lay, (y0, x0, side, side), (S, S), 2.2, out=out) is out
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(got22))


def test_negative_and_non_finite_radiance():
    """-1, +-inf and NaN at identity size: gamma 1 hands them through; under gamma 2.2 a negative finite base is NaN and both infinities give +inf, as numpy's float64 power has it."""
    from rnr_amd import _lib, ops
    f = np.ones((4, 4, 3), np.float32)
    f[0, 0, 0], f[1, 1, 1], f[2, 2, 2], f[3, 3, 0] = -1.0, np.inf, -np.inf, np.nan
    ident = tuple((4 * k, 12, _lib.EXR_FLOAT) for k in range(3))
    src = T(f).view(torch.uint8).reshape(-1).to(DEV)
    g1 = ops.photo_prepare_hdr(src, (4, 4), 48, ident, (0, 0, 4, 4), (4, 4), 1.0).cpu().numpy()
    assert np.array_equal(_bits(g1), _bits(f.transpose(2, 0, 1)))
    with np.errstate(invalid='ignore'):
        want = np.power(f.transpose(2, 0, 1).astype(np.float64), 2.2).astype(np.float32)
    g22 = ops.photo_prepare_hdr(src, (4, 4), 48, ident, (0, 0, 4, 4), (4, 4), 2.2).cpu().numpy()
    assert np.array_equal(np.isnan(g22), np.isnan(want)) and np.isnan(g22).sum() == 2
    assert np.array_equal(g22[~np.isnan(want)], want[~np.isnan(want)]) and g22[1, 1, 1] == np.inf


# ------------------------------------------------------------------------------------------------
# 4. guard bands and tracers
# ------------------------------------------------------------------------------------------------
def _footprint(s, side, S):
    """Output indices whose cell [d * sc, (d + 1) * sc) overlaps source pixel s by more than the kernel's 1e-3 threshold."""
    sc = side / S
    return {d for d in range(S) if min((d + 1) * sc, s + 1) - max(d * sc, s) > 1e-3}


def test_guard_bands_and_tracers(tmp_path):
    """Both entry points on guarded operands (payload and raw at odd addresses, the table at 8 mod 16, dst at 4 mod 8): every guard
    intact, the inputs unchanged, the bytes and bits those of the plain calls; one NaN (G) and one 1000.0 (R) in the 53 x 37 source
    reach exactly the output pixels whose footprint covers them."""
    from rnr_amd import capture, exr, ops
    from rnr_amd.testing import EntryCalls, In, Out
    h, w, S = 53, 37, 10
    smooth = (np.add.outer(np.arange(h), np.arange(w) * 0.5) / 128 + 0.0625).astype(np.float32)       # deflate shrinks it
    chans = {'R': smooth.astype(np.float16), 'G': smooth * 0.75, 'B': (smooth * 0.5).astype(np.float16)}
    assert max(float(c.max()) for c in chans.values()) < 1.0
    _, _, y0, x0, side = capture.crop_geometry(h, w)
    assert (y0, x0, side) == (8, 0, 36)
    ty, tx, ny, nx = 8 + 3, 18, 8 + 20, 8            # 1000.0 at window (3, 18): a cell boundary in y (3.6); NaN at window (20, 8)
    clean = {k: v.copy() for k, v in chans.items()}
    chans['R'][ty, tx] = 1000.0
    chans['G'][ny, nx] = np.nan
    fp = str(tmp_path / 'tracer.exr')
    assert set(er.write(fp, chans, compression=er.ZIP, force_raw=(2,))) == {'deflate', 'raw'}
    header, payload, table = exr.load(fp)
    raw_bytes = header.height * header.row_bytes
    ec = EntryCalls(True)
    ec.call('rnr_exr_unpack', payload=In(T(np.frombuffer(payload, np.uint8))), table=In(torch.tensor(table, dtype=torch.int64)),
            num_chunks=len(table), raw=Out((raw_bytes,), torch.uint8))
    assert ec.dev['payload'].data_ptr() % 2 == 1 and ec.dev['raw'].data_ptr() % 2 == 1 and ec.dev['table'].data_ptr() % 16 == 8
    (ro, rs, rt), (go, gs, gt), (bo, bs, bt) = exr.rgb_layout(header)
    ec.call('rnr_photo_prepare_hdr', src='@raw', src_h=h, src_w=w, row_bytes=header.row_bytes, r_offset=ro, r_stride=rs, r_type=rt,
            g_offset=go, g_stride=gs, g_type=gt, b_offset=bo, b_stride=bs, b_type=bt, crop_y0=y0, crop_x0=x0, crop_h=side,
            crop_w=side, gamma=1.0, dst=Out((3, S, S)), dst_h=S, dst_w=S)
    assert ec.dev['dst'].data_ptr() % 8 == 4
    assert all(v is None for v in ec.report().values()), ec.report()
    assert ec.dev['payload'].cpu().numpy().tobytes() == bytes(payload)
    assert ec.dev['table'].cpu().tolist() == [list(r) for r in table]
    assert ec.dev['raw'].cpu().numpy().tobytes() == er.raw_scanlines(fp)[0].tobytes()
    got = ec.results()['dst'].numpy()
    plain = ops.read_exr(fp, DEV, (y0, x0, side, side), (S, S), 1.0).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(plain))
    # tracers
    fp0 = str(tmp_path / 'clean.exr')
    er.write(fp0, clean, compression=er.ZIP)
    base = ops.read_exr(fp0, DEV, (y0, x0, side, side), (S, S), 1.0).cpu().numpy()
    assert np.isfinite(base).all() and base.max() < 1.0
    hot = {(dy, dx) for dy in _footprint(ty - y0, side, S) for dx in _footprint(tx - x0, side, S)}
    nan = {(dy, dx) for dy in _footprint(ny - y0, side, S) for dx in _footprint(nx - x0, side, S)}
    assert len(hot) == 2 and len(nan) == 1
    assert {tuple(p) for p in np.argwhere(got[0] > 1.0)} == hot
    assert {tuple(p) for p in np.argwhere(np.isnan(got[1]))} == nan
    assert {tuple(p) for p in np.argwhere(_bits(got[0]) != _bits(base[0]))} == hot
    assert {tuple(p) for p in np.argwhere(_bits(got[1]) != _bits(base[1]))} == nan
    assert np.array_equal(_bits(got[2]), _bits(base[2]))


# ------------------------------------------------------------------------------------------------
# 5. refusals
# ------------------------------------------------------------------------------------------------
def _prepare_args(over=None):
    """The valid call: 20 x 31 half RGB planar rows (62 bytes a channel, 186 a row), window rows [0, 20), columns [5, 25), to 8 x 8."""
    from rnr_amd.testing import In, Out
    raw = np.random.RandomState(3).randint(0, 0x3c00, (20, 93)).astype(np.uint16)
    args = dict(src=In(T(raw).view(torch.uint8).reshape(-1)), src_h=20, src_w=31, row_bytes=186, r_offset=124, r_stride=2, r_type=1,
                g_offset=62, g_stride=2, g_type=1, b_offset=0, b_stride=2, b_type=1, crop_y0=0, crop_x0=5, crop_h=20, crop_w=20,
                gamma=1.0, dst=Out((3, 8, 8)), dst_h=8, dst_w=8)
    args.update(over or {})
    return args


PREPARE_REFUSALS = {
    'type=0 (UINT)': dict(r_type=0), 'type=3': dict(g_type=3), 'type=-1': dict(b_type=-1),
    'offset<0': dict(b_offset=-2), 'stride below the size': dict(g_stride=1), 'float stride 2': dict(g_type=2),
    'row does not fit': dict(r_offset=126), 'float row does not fit': dict(r_type=2, r_stride=4, r_offset=64),
    'row_bytes=0': dict(row_bytes=0), 'row_bytes<0': dict(row_bytes=-186),
    'window above': dict(crop_y0=-1), 'window left': dict(crop_x0=-1), 'window below': dict(crop_y0=1), 'window right': dict(crop_x0=12),
    'gamma=0': dict(gamma=0.0), 'gamma<0': dict(gamma=-2.2), 'gamma=nan': dict(gamma=float('nan')), 'gamma=inf': dict(gamma=float('inf')),
    'dst off by two bytes': 'align',
    'src NULL': dict(src=None), 'dst NULL': dict(dst=None),
    'src_h=0': dict(src_h=0), 'src_w=0': dict(src_w=0), 'crop_h=0': dict(crop_h=0), 'crop_w=0': dict(crop_w=0),
    'dst_h=0': dict(dst_h=0), 'dst_w=0': dict(dst_w=0),
}


def _untouched(ec, name):
    from rnr_amd.testing import SENTINEL
    raw = ec.dev[name].cpu().view(-1).view(torch.uint8).numpy()
    word = np.frombuffer(SENTINEL.to_bytes(4, 'little'), np.uint8)
    assert np.array_equal(raw, np.tile(word, raw.size // 4 + 1)[:raw.size]), '%s was written' % name


@pytest.mark.parametrize('tag', sorted(PREPARE_REFUSALS))
def test_prepare_refusals_launch_nothing(tag):
    """Refused with the function's name in rnr_last_error; dst still holds the sentinel and every guard is intact."""
    from rnr_amd import _lib
    from rnr_amd.testing import EntryCalls, Out
    over = PREPARE_REFUSALS[tag]
    if over == 'align':
        over = dict(dst=Out((3, 8, 8), align=(4, 2)))
    ec = EntryCalls(True)
    rc = ec.call('rnr_photo_prepare_hdr', check=False, **_prepare_args(over))
    err = _lib.load().rnr_last_error().decode()
    assert rc != 0, 'rnr_photo_prepare_hdr accepted %s' % tag
    assert 'rnr_photo_prepare_hdr' in err, err
    if tag.endswith('two bytes'):
        assert 'aligned' in err, err
    assert all(v is None for v in ec.report().values()), ec.report()
    if 'dst' in ec.dev:
        _untouched(ec, 'dst')


def test_the_valid_prepare_call_of_the_refusal_table_runs():
    from rnr_amd.testing import EntryCalls
    ec = EntryCalls(True)
    assert ec.call('rnr_photo_prepare_hdr', **_prepare_args()) == 0
    assert bool(torch.isfinite(ec.results()['dst']).all()) and all(v is None for v in ec.report().values())


@pytest.mark.parametrize('tag', ['payload NULL', 'table NULL', 'raw NULL', 'num_chunks=0', 'num_chunks<0', 'table off by four bytes'])
def test_unpack_refusals_launch_nothing(tag):
    from rnr_amd import _lib
    from rnr_amd.testing import EntryCalls, In, Out
    args = dict(payload=In(T(np.arange(64, dtype=np.uint8))), table=In(torch.tensor([[0, 0, 64, 1]], dtype=torch.int64)), num_chunks=1,
                raw=Out((64,), torch.uint8))
    args.update({'payload NULL': dict(payload=None), 'table NULL': dict(table=None), 'raw NULL': dict(raw=None),
                 'num_chunks=0': dict(num_chunks=0), 'num_chunks<0': dict(num_chunks=-1),
                 'table off by four bytes': dict(table=In(torch.tensor([[0, 0, 64, 1]], dtype=torch.int64), align=(8, 4)))}[tag])
    ec = EntryCalls(True)
    rc = ec.call('rnr_exr_unpack', check=False, **args)
    err = _lib.load().rnr_last_error().decode()
    assert rc != 0 and 'rnr_exr_unpack' in err, (tag, err)
    if tag.endswith('four bytes'):
        assert 'aligned' in err, err
    assert all(v is None for v in ec.report().values()), ec.report()
    if 'raw' in ec.dev:
        _untouched(ec, 'raw')


# ------------------------------------------------------------------------------------------------
# 6. end to end
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def exr_capture(tmp_path_factory):
    """Two 41 x 53 photographs (half R and B, float G, radiance up to about 50, data window from (3, -2), the second in decreasing
    line order) and the golden calibration."""
    import scipy.io
    root = tmp_path_factory.mktemp('exr_capture')
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'dataio_views.npz'))
    calib_fp = str(root / 'calib.mat')
    scipy.io.savemat(calib_fp, {k[6:]: g[k] for k in g.files if k.startswith('calib:')})
    img_dir = str(root / 'rgb0')
    os.makedirs(img_dir)
    photos = []
    for i in range(2):
        # a highlight of radiance 50 on a dim smooth ground (deflate shrinks it), noise in the last rows (that chunk is stored raw)
        yy, xx = np.mgrid[0:41, 0:53].astype(np.float32)
        glow = 50 * np.exp(-((xx - 20 - 9 * i) ** 2 + (yy - 15) ** 2) / 60) + 0.05 + yy / 256
        chans = {'R': glow.astype(np.float16), 'G': (glow * 0.5).astype(np.float32), 'B': (glow * 0.25).astype(np.float16)}
        for c in chans.values():
            c[32:] = _radiance(9, 53, 50 + i, c.dtype)
        assert max(float(c.max()) for c in chans.values()) > 20
        how = er.write(os.path.join(img_dir, 'view_%d.exr' % i), chans, compression=er.ZIP, origin=(3, -2), decreasing=bool(i),
                       force_raw=(2,))
        assert how == ['deflate', 'deflate', 'raw'], how
        photos.append(np.stack([chans[k].astype(np.float32) for k in 'RGB'], -1))
    return dict(root=str(root), calib_fp=calib_fp, img_dir=img_dir, photos=photos)


def _as_float(photo, S, gamma):
    """The same arrays fed as float: interleaved float32 [H,W,3] through the same crop, size and gamma."""
    from rnr_amd import _lib, capture, ops
    h, w = photo.shape[:2]
    _, _, y0, x0, side = capture.crop_geometry(h, w)
    ident = tuple((4 * k, 12, _lib.EXR_FLOAT) for k in range(3))
    return ops.photo_prepare_hdr(T(photo).view(torch.uint8).reshape(-1).to(DEV), (h, w), 12 * w, ident, (y0, x0, side, side), (S, S), gamma)


@pytest.mark.parametrize('gamma', [1.0, 2.2])
def test_exr_capture_through_view_dataset(exr_capture, gamma):
    import dataio
    from rnr_amd import ops
    c = exr_capture
    for device in (None, DEV):
        ds = dataio.ViewDataset(c['root'], c['calib_fp'], 'convert', [32, 32], 'all', load_img=True, img_dir=c['img_dir'],
                                img_gamma=gamma, device=device)
        assert len(ds) == 2 and ds.img_idx2fn == ['view_0.exr', 'view_1.exr']
        for i in range(2):
            v = ds[i][0]
            img = v['img_gt']
            assert img.dtype == torch.float32 and tuple(img.shape) == (3, 32, 32) and img.is_cuda == (device is not None)
            assert np.array_equal(v['scale'].numpy(), np.array([32 / 40, 32 / 40], np.float32))
            want = _as_float(c['photos'][i], 32, gamma).cpu().numpy()
            assert np.array_equal(_bits(img.cpu().numpy()), _bits(want)), (device, i)
            if gamma == 1.0:
                win = c['photos'][i][0:40, 6:46]
                via = ops.resize_area(T(win).to(DEV), 32, 32).permute(2, 0, 1).cpu().numpy()
                assert np.array_equal(_bits(img.cpu().numpy()), _bits(via)) and float(img.max()) > 5.0


def test_exr_capture_through_the_stitcher(exr_capture):
    """The photographs through ViewDataset -> LightProbeStitcher.add give the probe of the float arrays fed directly, bit for bit."""
    import dataio
    from rnr_amd.lighting import LightProbeStitcher
    c = exr_capture
    ds = dataio.ViewDataset(c['root'], c['calib_fp'], 'convert', [32, 32], 'all', load_img=True, img_dir=c['img_dir'], device=DEV)
    views = [ds[i][0] for i in range(2)]
    Pi, Ri = torch.stack([v['proj_inv'] for v in views]).to(DEV), torch.stack([v['R_inv'] for v in views]).to(DEV)
    background = torch.ones(2, 32, 32, dtype=torch.uint8, device=DEV)
    background[:, 10:20, 12:22] = 0
    probes = []
    for images in (torch.stack([v['img_gt'] for v in views]), torch.stack([_as_float(p, 32, 1.0) for p in c['photos']])):
        st = LightProbeStitcher(16, 32, device=DEV)
        st.add(images, Pi, Ri, background=background)
        probes.append(st.result())
    a, b = probes
    assert int(a.count.sum()) > 0 and float(a.lp.max()) > 1.0
    assert np.array_equal(_bits(a.lp.cpu().numpy()), _bits(b.lp.cpu().numpy()))
    assert torch.equal(a.mask, b.mask) and torch.equal(a.count, b.count)


@pytest.mark.parametrize('gamma', [1.0, 2.2])
def test_exr_probe_through_light_probe_dataset(tmp_path, gamma):
    """a.exr (FLOAT channels, so the same float32 values) and b.npy through LightProbeDataset: the same item at gamma 1 bit for bit,
    within 16 float32 ulp at gamma 2.2 (the .npy reader uses numpy's float32 **, which lies up to 10 ulp from the correctly rounded
    power, include/rnr_hip.h; the kernel's is within 1) - and the same LightingLP."""
    import dataio
    import network
    from rnr_amd import scene
    probe = np.stack([_radiance(24, 48, 80 + i) for i in range(3)], -1)
    er.write(str(tmp_path / 'a.exr'), {k: probe[..., i].copy() for i, k in enumerate('RGB')}, compression=er.ZIP)
    np.save(str(tmp_path / 'b.npy'), probe)
    ds = dataio.LightProbeDataset(str(tmp_path), img_gamma=gamma)
    assert [os.path.basename(f) for f in ds.lp_fp_all] == ['a.exr', 'b.npy']
    a, b = ds[0]['lp_img'], ds[1]['lp_img']
    assert a.dtype == torch.float32 and tuple(a.shape) == (3, 24, 48) and not a.is_cuda and float(a.max()) > 5.0
    if gamma == 1.0:
        assert np.array_equal(_bits(a.numpy()), _bits(b.numpy()))
    else:
        ulp = float((np.abs(a.numpy().astype(np.float64) - b.numpy().astype(np.float64)) / np.spacing(b.numpy()).astype(np.float64)).max())
        print('gamma 2.2: .exr item within %.2f ulp of the .npy item' % ulp)
        assert ulp <= 16.0
    l_dir = T(scene.sphere_samples(64)).t().contiguous()
    lps = [network.LightingLP(l_dir, num_channel=3, lp_dataloader=[{'lp_img': t[None]}], fix_params=True, lp_img_h=12, lp_img_w=24,
                              device=DEV) for t in (a, b)]
    if gamma == 1.0:
        assert torch.equal(lps[0].lps, lps[1].lps) and torch.equal(lps[0].l_samples, lps[1].l_samples)
    else:
        assert torch.allclose(lps[0].lps, lps[1].lps, rtol=4e-6, atol=0) and torch.allclose(lps[0].l_samples, lps[1].l_samples, rtol=1e-5)
