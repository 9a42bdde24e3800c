"""-m gpu: OpenEXR out.  rnr_exr_pack (float32 RGB images -> the bytes an OpenEXR file hands to deflate, or stores raw) against
the numpy restatement of tests/exr_ref.py byte for byte: the float -> half conversion on every finite half, its float32
neighbours, every tie and the ties' neighbours; every geometry x type x chunking x source layout; its inverse rnr_exr_unpack;
batches; guard bands, tracers and refusals.  Then the files: ops.write_exr / write_exr_batch read back by the restatement and by
ops.read_exr, StitchedProbe.save(exr=True) / load(source='exr') / LightProbeDataset, and an HDR frame whose maximum survives.

Expected half bits: numpy's astype(np.float16) for every input that is not a NaN (round to nearest even, subnormals, overflow to
inf: IEEE, whichever of numpy's software and the host's hardware conversion runs); for a NaN the rule of include/rnr_hip.h written
out here in integers, sign | 0x7c00 | (mantissa >> 13), lowest bit set when that field is 0 (a hardware conversion may quieten
NaNs differently, so numpy is not asked)."""
import os

import numpy as np
import pytest
import torch

import exr_ref as er

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
HALF, FLOAT = 1, 2


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def expected_half_bits(f):
    """float32 array -> uint16 array of the same shape (module docstring)."""
    f = np.ascontiguousarray(f, dtype=np.float32)
    bits = f.view(np.uint32)
    nan = (bits & 0x7fffffff) > 0x7f800000
    with np.errstate(over='ignore', invalid='ignore'):
        out = np.where(nan, np.float32(0), f).astype(np.float16).view(np.uint16).copy()
    field = ((bits & 0x007fffff) >> 13).astype(np.uint16)
    rule = ((bits >> 16) & 0x8000).astype(np.uint16) | np.uint16(0x7c00) | field | (field == 0).astype(np.uint16)
    out[nan] = rule[nan]
    return out


def expected_raw(rgb, ptype):
    """rgb float32 [3,H,W] -> (uint8 [H * row_bytes], row_bytes): per scanline the run of B, of G, of R values, little endian."""
    vals = expected_half_bits(rgb).astype('<u2') if ptype == HALF else _u32(rgb).astype('<u4')
    rows = np.ascontiguousarray(vals[::-1].transpose(1, 0, 2))                      # [H, (B, G, R), W]
    return rows.reshape(-1).view(np.uint8), rows.shape[1] * rows.shape[2] * rows.itemsize


def expected_bytes(rgb, ptype, lines, coded):
    """What rnr_exr_pack must write for one image: raw, or every chunk of `lines` scanlines through exr_ref.encode_chunk."""
    raw, row_bytes = expected_raw(rgb, ptype)
    if not coded:
        return raw.tobytes()
    step = lines * row_bytes
    return b''.join(er.encode_chunk(raw[p:p + step].tobytes())[1] for p in range(0, raw.size, step))


def _pixels(h, w, seed):
    """float32 [3,h,w]: radiance up to about 50, mostly below 1; one value in eight any bit pattern (NaNs, infinities, subnormals,
    values past 65504, both signs)."""
    rng = np.random.RandomState(seed)
    a = (rng.rand(3, h, w) ** 4 * 50 + 1e-3).astype(np.float32)
    wild = rng.randint(0, 1 << 32, (3, h, w), dtype=np.uint64).astype(np.uint32).view(np.float32)
    return np.where(rng.rand(3, h, w) < 0.125, wild, a)


# ------------------------------------------------------------------------------------------------
# 1. every half
# ------------------------------------------------------------------------------------------------
def test_every_half_its_neighbours_and_every_tie():
    from rnr_amd import ops
    mag = np.arange(0x7c00, dtype=np.uint16)                                         # every finite half magnitude
    val = mag.view(np.float16).astype(np.float64)
    nxt = np.append(val[1:], 65536.0)                                                # the next half in magnitude; past 65504: 2^16
    mid = ((val + nxt) / 2).astype(np.float32)
    assert np.array_equal(mid.astype(np.float64), (val + nxt) / 2) and mid[-1] == 65520.0       # a half has 11 bits: the tie is exact
    exact = val.astype(np.float32)
    inf = np.float32(np.inf)
    pos = np.concatenate([exact, np.nextafter(exact, -inf), np.nextafter(exact, inf), mid, np.nextafter(mid, -inf), np.nextafter(mid, inf)])
    special = np.array([65519.996, 65520.0, np.finfo(np.float32).max, np.inf, 2.0 ** -25, np.nextafter(np.float32(2.0 ** -25), inf),
                        0.0], np.float32)
    sub = np.array([1, 2, 0x400000, 0x7fffff, 0x800000], np.uint32).view(np.float32)                  # float32 subnormals, the first normal
    nans = np.array([0x7f800001, 0x7f802000, 0x7fc00000, 0xff800001, 0xffc12000, 0x7fffffff], np.uint32).view(np.float32)
    both = np.concatenate([pos, special, sub])
    values = np.concatenate([both, -both, nans])
    vbits = values.view(np.uint32)
    assert vbits[both.size + pos.size + 6] == 0x80000000 and 3.8e5 < values.size < 4.2e5
    W = 512
    H = -(-values.size // (3 * W))
    img = np.zeros(3 * H * W, np.float32)
    img[:values.size] = values
    img = img.reshape(3, H, W)
    out = ops.exr_pack(T(img)[None].to(DEV), HALF, 1, 0, channels_last=False).cpu().numpy()
    got = out.reshape(-1).view('<u2').reshape(H, 3, W)[:, ::-1].transpose(1, 0, 2).reshape(-1)[:values.size]
    want = expected_half_bits(values)
    # the rule on the NaNs and the three values the header spells out
    assert list(want[-6:]) == [0x7c01, 0x7c01, 0x7e00, 0xfc01, 0xfe09, 0x7fff]
    assert list(expected_half_bits(np.array([65519.996, 65520.0, 2.0 ** -25, -0.0], np.float32))) == [0x7bff, 0x7c00, 0, 0x8000]
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(hex(int(vbits[i])), hex(int(got[i])), hex(int(want[i]))) for i in bad[:8]]
    # exact values come back as themselves
    assert np.array_equal(got[:mag.size], mag) and np.array_equal(got[both.size:both.size + mag.size], mag | 0x8000)


# ------------------------------------------------------------------------------------------------
# 2. geometry x type x chunking x layout
# ------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (1, 5), (2, 3), (15, 7), (16, 16), (17, 33), (33, 700), (5, 2731)]
LAYOUTS = ['chw', 'hwc', 'hw4', 'crop']
TRACERS = (float('nan'), 1000.0)


def _source(rgb, layout):
    """rgb float32 [3,H,W] -> (a device view of those values addressed as the layout says, channels_last).  Everything the view
    does not address holds NaN and 1000.0."""
    _, h, w = rgb.shape
    if layout == 'chw':
        return T(rgb).to(DEV), False
    if layout == 'hwc':
        return T(rgb.transpose(1, 2, 0)).to(DEV), True
    if layout == 'hw4':                             # channels 0..2 of an [H, W + 3, 4] buffer
        buf = torch.empty(h, w + 3, 4)
        buf[..., 0::2], buf[..., 1::2] = TRACERS
        buf[:, :w, :3] = T(rgb.transpose(1, 2, 0))
        return buf.to(DEV)[:, :w, :3], True
    big = torch.empty(3, h + 5, w + 7)              # a crop out of a larger image
    big[:, 0::2], big[:, 1::2] = TRACERS
    big[:, 2:2 + h, 3:3 + w] = T(rgb)
    return big.to(DEV)[:, 2:2 + h, 3:3 + w], False


@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('lines', [1, 16])
@pytest.mark.parametrize('ptype', [HALF, FLOAT], ids=['half', 'float'])
@pytest.mark.parametrize('shape', SHAPES, ids=['%dx%d' % s for s in SHAPES])
def test_geometry_type_chunking_layout(shape, ptype, lines, layout):
    from rnr_amd import ops
    h, w = shape
    rgb = _pixels(h, w, 1000 * h + w)
    src, channels_last = _source(rgb, layout)
    assert src.is_contiguous() or layout in ('hw4', 'crop')
    ptr = src.data_ptr()
    for coded in (1, 0):
        got = ops.exr_pack(src[None], ptype, lines, coded, channels_last=channels_last)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (1, h * 3 * w * (2 if ptype == HALF else 4))
        assert got.cpu().numpy().tobytes() == expected_bytes(rgb, ptype, lines, coded), (coded,)
    assert src.data_ptr() == ptr


def test_the_cases_cover_the_kernels_paths():
    """(33, 700) under ZIP: a chunk of 33 600 values, several workgroups, and a last chunk of one line; (5, 2731) under ZIPS: the
    half point of a HALF chunk at byte 8193, an odd address two bytes past two workgroups' worth."""
    from rnr_amd import _lib
    seg = _lib.EXR_PACK_SEGMENT
    assert seg == 4096
    assert 16 * 700 * 3 == 33600 and 33600 > 8 * seg and 33 % 16 == 1
    assert 2731 * 3 == 8193 and 8193 % 2 == 1 and 8193 > 2 * seg


# ------------------------------------------------------------------------------------------------
# 3. the inverse
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ptype', [HALF, FLOAT], ids=['half', 'float'])
@pytest.mark.parametrize('shape, lines', [((17, 33), 16), ((33, 700), 16), ((5, 2731), 1), ((15, 7), 1)])
def test_unpack_inverts_pack(shape, lines, ptype):
    """coded = 1 through the merged rnr_exr_unpack, with the table rnr_amd.exr.load builds for such a file, gives coded = 0."""
    from rnr_amd import ops
    h, w = shape
    rgb = _pixels(h, w, 77 + h)
    src = T(rgb).to(DEV)[None]
    coded = ops.exr_pack(src, ptype, lines, 1, channels_last=False)
    raw, row_bytes = expected_raw(rgb, ptype)
    table, pos = [], 0
    for y in range(0, h, lines):
        n = min(lines, h - y) * row_bytes
        table.append((pos, y * row_bytes, n, 1))
        pos += n
    back = ops.exr_unpack(coded.view(-1), torch.tensor(table, dtype=torch.int64).to(DEV), h * row_bytes)
    assert back.cpu().numpy().tobytes() == raw.tobytes()
    assert torch.equal(back, ops.exr_pack(src, ptype, lines, 0, channels_last=False).view(-1))


# ------------------------------------------------------------------------------------------------
# 4. batch
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('channels_last', [False, True])
@pytest.mark.parametrize('ptype', [HALF, FLOAT], ids=['half', 'float'])
def test_three_images_in_one_launch(ptype, channels_last):
    """Images 0, 2 and 4 of six (an image stride of two images): one launch equals the three single launches and the restatement."""
    from rnr_amd import ops
    h, w = 17, 33
    six = np.stack([_pixels(h, w, 300 + i) for i in range(6)])
    dev = T(six.transpose(0, 2, 3, 1) if channels_last else six).to(DEV)
    for lines, coded in ((16, 1), (1, 1), (1, 0)):
        got = ops.exr_pack(dev[::2], ptype, lines, coded, channels_last=channels_last)
        assert got.shape[0] == 3
        for k in range(3):
            one = ops.exr_pack(dev[2 * k:2 * k + 1], ptype, lines, coded, channels_last=channels_last)
            assert torch.equal(got[k], one[0])
            assert got[k].cpu().numpy().tobytes() == expected_bytes(six[2 * k], ptype, lines, coded)


# ------------------------------------------------------------------------------------------------
# 5. guard bands and tracers
# ------------------------------------------------------------------------------------------------
def _tracer_source(rgb):
    """rgb [3,h,w] as rows 2.. and channels 0..2 of an [h + 4, w + 3, 4] buffer; a NaN in the unused channel, 1000.0 in the padding
    columns, both in the rows outside.  -> (CPU buffer, the addressing of the values in floats)."""
    _, h, w = rgb.shape
    buf = torch.empty(h + 4, w + 3, 4)
    buf[0::2], buf[1::2] = TRACERS
    buf[2:2 + h, :, 3] = float('nan')
    buf[2:2 + h, w:, :3] = 1000.0
    buf[2:2 + h, :w, :3] = T(rgb.transpose(1, 2, 0))
    rs = 4 * (w + 3)
    return buf, dict(image_stride=0, row_stride=rs, x_stride=4, r_offset=2 * rs, g_offset=2 * rs + 1, b_offset=2 * rs + 2)


@pytest.mark.parametrize('ptype, lines, coded', [(HALF, 16, 1), (HALF, 1, 1), (FLOAT, 16, 1), (HALF, 1, 0), (FLOAT, 1, 0)])
def test_guard_bands_and_tracers(ptype, lines, coded):
    """33 x 85 (a last chunk of one line; 255 values a line, so every chunk and half point at another residue of 4): dst guarded at
    an odd address, and inside a larger buffer at an odd offset between 64-byte margins of 0xA5; the source's unused channel,
    padding columns and the rows outside the crop hold NaN and 1000.0, and the bytes are those of the clean values."""
    from rnr_amd import ops
    from rnr_amd.testing import EntryCalls, In, Out
    h, w = 33, 85
    rgb = _pixels(h, w, 5)
    rgb[np.isnan(rgb) | (rgb == 1000.0)] = 0.5                  # the values themselves hold neither tracer
    want = expected_bytes(rgb, ptype, lines, coded)
    nbytes = len(want)
    buf, addr = _tracer_source(rgb)
    ec = EntryCalls(True)
    ec.call('rnr_exr_pack', src=In(buf), num_images=1, height=h, width=w, pixel_type=ptype, lines_per_chunk=lines, coded=coded,
            dst=Out((nbytes,), torch.uint8), **addr)
    assert ec.dev['dst'].data_ptr() % 2 == 1 and ec.dev['src'].data_ptr() % 8 == 4
    assert all(v is None for v in ec.report().values()), ec.report()
    assert ec.results()['dst'].numpy().tobytes() == want
    assert ec.dev['src'].cpu().view(-1).view(torch.int32).equal(buf.view(-1).view(torch.int32))      # the source is unchanged
    # the same through ops.exr_pack into a slice of a larger buffer
    for off in (65, 66, 67):
        big = torch.full((nbytes + 64 + off,), 0xA5, dtype=torch.uint8, device=DEV)
        view = buf.to(DEV)[2:2 + h, :w, :3]
        ops.exr_pack(view[None], ptype, lines, coded, channels_last=True, out=big[off:off + nbytes])
        got = big.cpu().numpy()
        assert got[off:off + nbytes].tobytes() == want, off
        assert (got[:off] == 0xA5).all() and (got[off + nbytes:] == 0xA5).all(), off
    if ptype == HALF and not coded:                             # the tracers' own half patterns are nowhere in the output
        halves = np.frombuffer(want, '<u2')
        assert not np.isin(halves, [0x7e00, 0x63d0]).any() and list(expected_half_bits(np.array([1000.0, np.nan], np.float32))) == [0x63d0, 0x7e00]


# ------------------------------------------------------------------------------------------------
# 6. refusals
# ------------------------------------------------------------------------------------------------
def _pack_args(over=None):
    """The valid call: a 20 x 31 crop (rows 2.., columns 3..) of a [3,25,40] image, HALF, ZIP chunks, coded."""
    from rnr_amd.testing import In, Out
    img = T(_pixels(25, 40, 9))
    args = dict(src=In(img), num_images=1, height=20, width=31, image_stride=0, row_stride=40, x_stride=1, r_offset=83,
                g_offset=1083, b_offset=2083, pixel_type=HALF, lines_per_chunk=16, coded=1, dst=Out((20 * 31 * 6,), torch.uint8))
    args.update(over or {})
    return args


PACK_REFUSALS = {
    'src NULL': dict(src=None), 'dst NULL': dict(dst=None),
    'num_images=0': dict(num_images=0), 'num_images<0': dict(num_images=-1), 'height=0': dict(height=0), 'height<0': dict(height=-20),
    'width=0': dict(width=0), 'width<0': dict(width=-31),
    'image_stride<0': dict(image_stride=-1), 'row_stride<0': dict(row_stride=-40), 'x_stride<0': dict(x_stride=-1),
    'r_offset<0': dict(r_offset=-1), 'g_offset<0': dict(g_offset=-1), 'b_offset<0': dict(b_offset=-1),
    'type=0 (UINT)': dict(pixel_type=0), 'type=3': dict(pixel_type=3), 'type=-1': dict(pixel_type=-1),
    'coded=2': dict(coded=2), 'coded=-1': dict(coded=-1),
    'lines_per_chunk=0': dict(lines_per_chunk=0), 'lines_per_chunk<0': dict(lines_per_chunk=-16),
    'src off by two bytes': 'align',
    'half image above 2^31 bytes': dict(height=1 << 20, width=1 << 10), 'float image above 2^31 bytes': dict(pixel_type=FLOAT, height=1 << 14, width=(1 << 14) + 1),
    'more than 2^31 - 1 workgroups': dict(num_images=(1 << 30) + 1),
}


@pytest.mark.parametrize('tag', sorted(PACK_REFUSALS))
def test_pack_refusals_launch_nothing(tag):
    """Refused with the function's name in rnr_last_error; dst still holds the sentinel and every guard is intact."""
    from rnr_amd import _lib
    from rnr_amd.testing import SENTINEL, EntryCalls, In
    over = PACK_REFUSALS[tag]
    if over == 'align':
        over = dict(src=In(T(_pixels(25, 40, 9)), align=(4, 2)))
    ec = EntryCalls(True)
    rc = ec.call('rnr_exr_pack', check=False, **_pack_args(over))
    err = _lib.load().rnr_last_error().decode()
    assert rc != 0, 'rnr_exr_pack accepted %s' % tag
    assert 'rnr_exr_pack' in err, err
    if tag.endswith('two bytes'):
        assert 'aligned' in err, err
    assert all(v is None for v in ec.report().values()), ec.report()
    if 'dst' in ec.dev:
        raw = ec.dev['dst'].cpu().view(-1).numpy()
        word = np.frombuffer(SENTINEL.to_bytes(4, 'little'), np.uint8)
        assert np.array_equal(raw, np.tile(word, raw.size // 4 + 1)[:raw.size]), 'dst was written'


def test_the_valid_pack_call_of_the_refusal_table_runs():
    from rnr_amd.testing import EntryCalls
    ec = EntryCalls(True)
    args = _pack_args()
    assert ec.call('rnr_exr_pack', **args) == 0
    assert all(v is None for v in ec.report().values())
    rgb = args['src'].tensor.numpy()[:, 2:22, 3:34]
    assert ec.results()['dst'].numpy().tobytes() == expected_bytes(rgb, HALF, 16, 1)


def test_wrapper_refusals():
    from rnr_amd import ops
    img = torch.zeros(3, 5, 3, device=DEV)
    with pytest.raises(ValueError, match='channels_last'):
        ops.write_exr('never.exr', img)                                             # [3,5,3] reads both ways
    with pytest.raises(ValueError):
        ops.write_exr('never.exr', torch.zeros(4, 5, 6, device=DEV))                # no axis of 3
    with pytest.raises(ValueError):
        ops.write_exr('never.exr', torch.zeros(3, 5, 6, device=DEV), channels_last=True)
    with pytest.raises(RuntimeError, match='float32'):
        ops.write_exr('never.exr', torch.zeros(3, 5, 6, device=DEV, dtype=torch.float64))
    with pytest.raises(ValueError, match='pixel_type'):
        ops.write_exr('never.exr', torch.zeros(3, 5, 6, device=DEV), pixel_type='uint')
    with pytest.raises(ValueError, match='compression'):
        ops.write_exr('never.exr', torch.zeros(3, 5, 6, device=DEV), compression='piz')
    with pytest.raises(ValueError, match='paths'):
        ops.write_exr_batch(['a.exr'], torch.zeros(2, 3, 5, 6, device=DEV))
    with pytest.raises(RuntimeError, match='CUDA'):
        ops.exr_pack(torch.zeros(1, 3, 5, 6), HALF, 1, 0)
    assert not os.path.exists('never.exr') and not os.path.exists('a.exr')


# ------------------------------------------------------------------------------------------------
# 7. files
# ------------------------------------------------------------------------------------------------
def _smooth_and_noise(h, w, seed):
    """float32 [3,h,w]: a smooth ramp above, below row h / 2 noise built from integer bit patterns (NaNs, -0 and infinities among
    them: the patterns 0x7fc00000, 0x80000000 and 0xff800000 are planted)."""
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    img = np.stack([((y * 0.25 + x * 0.125 + 0.5) * (k + 1)).astype(np.float32) for k in range(3)])
    noise = np.random.RandomState(seed).randint(0, 1 << 32, (3, h - h // 2, w), dtype=np.uint64).astype(np.uint32)
    noise[0, 0, :3] = (0x7fc00000, 0x80000000, 0xff800000)
    img[:, h // 2:] = noise.view(np.float32)
    return img


def _equal_values(a, b):
    """== plus matching NaN positions (so -0 == +0)."""
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and bool((a[~np.isnan(a)] == b[~np.isnan(b)]).all())


def test_write_exr_stores_both_kinds_of_chunk(tmp_path):
    from rnr_amd import ops
    img = _smooth_and_noise(40, 40, 1)
    fp = str(tmp_path / 'both.exr')
    how = ops.write_exr(fp, T(img).to(DEV), 'float', 'zip')
    assert how[0] == 'deflate' and how[2] == 'raw'               # rows 0..15 smooth, rows 32..39 noise (16..31: both)
    chans, info = er.decode(fp)
    assert info['stored'] == how and [c for c, _ in info['channels']] == ['B', 'G', 'R']
    for k, name in enumerate('RGB'):
        assert chans[name].dtype == np.float32 and np.array_equal(chans[name].view(np.uint32), _u32(img[k])), name
    back = ops.read_exr(fp, DEV).cpu().numpy()
    assert _equal_values(back, img) and np.isnan(img).sum() >= 1 and (_u32(img) == 0x80000000).sum() >= 1
    # the restatement's writer on the same pixels: the same file
    ref = str(tmp_path / 'ref.exr')
    assert er.write(ref, {name: img[k] for k, name in enumerate('RGB')}, compression=er.ZIP) == how
    assert open(ref, 'rb').read() == open(fp, 'rb').read()


@pytest.mark.parametrize('pixel_type, compression', [('half', 'zip'), ('half', 'zips'), ('float', 'none'), ('half', 'none')])
def test_write_exr_layouts_and_a_cpu_image(pixel_type, compression, tmp_path):
    """[3,H,W] on the device, [H,W,3] on the CPU and a crop by strides give the same file, which decodes to the expected bits."""
    from rnr_amd import ops
    h, w = 19, 23
    img = _pixels(h, w, 4)
    big = torch.full((3, h + 2, w + 2), float('nan'), device=DEV)
    big[:, 1:1 + h, 1:1 + w] = T(img).to(DEV)
    files = [str(tmp_path / n) for n in ('a.exr', 'b.exr', 'c.exr')]
    how = ops.write_exr(files[0], T(img).to(DEV), pixel_type, compression)
    assert ops.write_exr(files[1], T(img.transpose(1, 2, 0)), pixel_type, compression) == how
    assert ops.write_exr(files[2], big[:, 1:1 + h, 1:1 + w], pixel_type, compression, level=6, channels_last=False) == how
    data = open(files[0], 'rb').read()
    assert open(files[1], 'rb').read() == data and open(files[2], 'rb').read() == data
    chans, info = er.decode(files[0])
    assert info['stored'] == how and len(how) == (2 if compression == 'zip' else h)
    for k, name in enumerate('RGB'):
        if pixel_type == 'half':
            assert np.array_equal(chans[name].view(np.uint16), expected_half_bits(img[k])), name
        else:
            assert np.array_equal(chans[name].view(np.uint32), _u32(img[k])), name


@pytest.mark.parametrize('channels_last', [False, True])
def test_write_exr_batch_equals_three_files(channels_last, tmp_path):
    from rnr_amd import ops
    imgs = np.stack([_smooth_and_noise(40, 40, 10 + i) for i in range(3)])
    imgs[1, :, 20:] = imgs[1, :, :20]                            # the second image is smooth throughout: no raw chunk
    dev = T(imgs.transpose(0, 2, 3, 1) if channels_last else imgs).to(DEV)
    batch = [str(tmp_path / ('batch_%d.exr' % i)) for i in range(3)]
    single = [str(tmp_path / ('single_%d.exr' % i)) for i in range(3)]
    how = ops.write_exr_batch(batch, dev, 'float', 'zip')
    assert how[0][0] == 'deflate' and how[0][2] == 'raw' and how[1] == ['deflate'] * 3
    for i in range(3):
        assert ops.write_exr(single[i], dev[i], 'float', 'zip') == how[i]
        assert open(batch[i], 'rb').read() == open(single[i], 'rb').read()


# ------------------------------------------------------------------------------------------------
# 8. through the features
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def small():
    """The 64^2, nf0 = 4 scene of the frame tests, four poses: its probe, frames, coverage and cameras."""
    from rnr_amd import scene, testing
    from rnr_amd.pipeline import RNRPipeline
    sc = testing.tiny_scene(img_size=64, nf0=4, tex_size=32, tex_ch=16, nlat=16, nlon=32, seed=0)
    lp = torch.as_tensor(sc['lp'], dtype=torch.float32).reshape(sc['lp'].shape[-3], sc['lp'].shape[-2], 3).contiguous().to(DEV)

    def mk(probe):
        return RNRPipeline(sc['mesh'], 64, sc['textures'], sc['unet_sd'], sc['pivots_spec'], sc['pivots_diff'], probe, nf0=4, device=DEV,
                           max_views=4)
    v = {k: T(x).to(DEV) for k, x in scene.spiral_views(64, [5, 200, 400, 650]).items()}
    pipe = mk(lp)
    frames = pipe.render(v['proj'], v['pose'], v['proj_inv'], v['R_inv'], keep_intermediates=True).clone()
    alpha = pipe.last['gb']['alpha'].clone()
    return dict(sc=sc, lp=lp, mk=mk, v=v, frames=frames, alpha=alpha)


def test_stitched_probe_through_exr(small, tmp_path):
    """A probe stitched from the capture's backgrounds (the scene's probe seen along every background pixel's ray) is saved with
    exr=True; StitchedProbe.load(source='exr') and LightProbeDataset return lp bit for bit, and lighting_init_from_stitch from
    the loaded probe equals that from the one in memory bit for bit."""
    import dataio
    from rnr_amd import ops, scene
    from rnr_amd.lighting import LightProbeStitcher, StitchedProbe, lighting_init_from_stitch
    v = small['v']
    photos = ops.env_background(v['proj_inv'], v['R_inv'], small['lp'] * (3.0 / float(small['lp'].max())), (64, 64))          # [4,64,64,3], radiance above 1
    st = LightProbeStitcher(32, 64, device=DEV)
    st.add(photos, v['proj_inv'], v['R_inv'], alpha=small['alpha'], channels_last=True)
    res = st.result()
    assert 0.02 < float((res.mask != 0).float().mean()) < 1.0 and float(res.lp.max()) > 1.0
    d = str(tmp_path / 'stitch')
    before = res.lp.clone()
    res.save(d, exr=True)
    assert torch.equal(res.lp, before)
    assert sorted(os.listdir(d)) == ['0.exr', '0.npy', '0.png', 'count', 'mask']
    chans, info = er.decode(os.path.join(d, '0.exr'))
    assert set(info['stored']) <= {'deflate', 'raw'} and all(chans[k].dtype == np.float32 for k in 'RGB')
    want = res.lp.cpu().numpy()
    for k, name in enumerate('RGB'):
        assert np.array_equal(chans[name].view(np.uint32), _u32(want[..., k])), name
    # the default writes what it wrote before
    d0 = str(tmp_path / 'plain')
    res.save(d0)
    assert sorted(os.listdir(d0)) == ['0.npy', '0.png', 'count', 'mask']
    for device in (None, DEV):
        back = StitchedProbe.load(d, device=device, source='exr')
        assert back.lp.is_cuda == (device is not None) and back.lp.dtype == torch.float32
        assert np.array_equal(_u32(back.lp.cpu().numpy()), _u32(want))
        assert torch.equal(back.mask.cpu() != 0, res.mask.cpu() != 0) and torch.equal(back.count.cpu(), res.count.cpu()) and back.num_view == 4
    with pytest.raises(ValueError, match='source'):
        StitchedProbe.load(d, source='hdr')
    ds = dataio.LightProbeDataset(d)
    assert os.path.basename(ds.lp_fp_all[0]) == '0.exr'
    item = ds[0]['lp_img']
    assert not item.is_cuda and np.array_equal(_u32(item.numpy()), _u32(want.transpose(2, 0, 1)))
    l_dir = T(scene.sphere_samples(64)).t().contiguous().to(DEV)
    a = lighting_init_from_stitch(res, l_dir, 2, lp_recon_h=8, lp_recon_w=16)
    b = lighting_init_from_stitch(StitchedProbe.load(d, device=DEV, source='exr'), l_dir, 2, lp_recon_h=8, lp_recon_w=16)
    assert sorted(a) == sorted(b)
    for key in a:
        assert torch.equal(a[key], b[key]), key


def test_hdr_frame_keeps_what_eight_bits_lose(small, tmp_path):
    """A frame lit by the probe scaled until its maximum exceeds 1, written HALF / ZIP: it reads back equal to the frame rounded to
    half, and the maximum is still above 1."""
    from rnr_amd import ops
    v = small['v']
    peak = float(small['frames'].max())
    assert peak > 0
    pipe = small['mk'](small['lp'] * (4.0 / peak))
    frames = pipe.render(v['proj'], v['pose'], v['proj_inv'], v['R_inv']).clone()
    assert float(frames.max()) > 1.0 and bool(torch.isfinite(frames).all())
    files = [str(tmp_path / ('frame_%d.exr' % i)) for i in range(4)]
    how = ops.write_exr_batch(files, frames, 'half', 'zip')
    assert len(how) == 4 and all(len(h) == 4 for h in how)
    for i, fp in enumerate(files):
        back = ops.read_exr(fp, DEV).cpu().numpy()
        want = expected_half_bits(frames[i].cpu().numpy()).view(np.float16).astype(np.float32)
        assert _equal_values(back, want), i
    top = max(float(ops.read_exr(fp, DEV).max()) for fp in files)
    assert top > 1.0 and top == float(np.float32(np.float16(float(frames.max()))))
    u8 = ops.present_u8(frames.contiguous(), small['alpha'], v['proj_inv'], v['R_inv'], small['lp'], mode='frame')
    assert int(u8.max()) == 255                                  # the 8-bit route clamps at 1
