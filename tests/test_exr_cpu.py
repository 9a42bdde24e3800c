"""CPU: the OpenEXR scanline reader rnr_amd/exr.py without a GPU — the format document's literal example, one file spelled out byte
by byte, the restatement's writer -> decoder round trips (tests/exr_ref.py), read_header / ViewDataset.read_camera of an .exr
capture, every refusal by file name and field, which chunks deflate shrinks and which it does not, and the new symbols."""
import os
import struct
import zlib

import numpy as np
import pytest

import exr_ref as er


def _ramp(h, w, dtype, scale=1.0):
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    return ((y * 0.25 + x * 0.125 + 0.5) * scale).astype(dtype)


def _noise(h, w, dtype, seed):
    rng = np.random.RandomState(seed)
    if dtype == np.float16:
        bits = rng.randint(0, 0x7c00, (h, w)).astype(np.uint16)          # finite, positive: every mantissa and exponent byte random
        return bits.view(np.float16)
    return (rng.rand(h, w) * 50).astype(dtype)


# ------------------------------------------------------------------------------------------------
# 1. the literal example
# ------------------------------------------------------------------------------------------------
RAW, SPLIT, CODED = bytes.fromhex('010203040506'), bytes.fromhex('010305020406'), bytes.fromhex('0182827d8282')


def test_literal_example_both_directions():
    from rnr_amd import exr
    assert er.encode_chunk(RAW) == (SPLIT, CODED)
    assert er.decode_chunk(CODED) == RAW
    assert exr.unpack_chunk(CODED) == RAW
    # odd length: the lower half takes the extra byte
    for n in (1, 2, 5, 7, 255, 256, 257):
        raw = bytes(np.random.RandomState(n).randint(0, 256, n).astype(np.uint8))
        assert er.decode_chunk(er.encode_chunk(raw)[1]) == raw
        assert exr.unpack_chunk(er.encode_chunk(raw)[1]) == raw


# ------------------------------------------------------------------------------------------------
# 2. one file, byte by byte
# ------------------------------------------------------------------------------------------------
def _literal_file():
    """A 2 x 1 file (one scanline, two pixels), channels B G R, all HALF, uncompressed."""
    b = b''
    b += bytes([0x76, 0x2f, 0x31, 0x01])                # magic number 20000630, little endian
    b += bytes([0x02, 0x00, 0x00, 0x00])                # version 2, no flag bits: single-part scanline, names <= 31 bytes
    # --- header: attribute name \0, type name \0, int32 size, value ---
    b += b'channels\0' + b'chlist\0'
    b += struct.pack('<i', 3 * 18 + 1)                  # size: three entries of 2 + 16 bytes and the closing \0
    for name in (b'B', b'G', b'R'):                     # sorted by name
        b += name + b'\0'                               # channel name
        b += struct.pack('<i', 1)                       # pixel type: 0 UINT, 1 HALF, 2 FLOAT
        b += bytes([0])                                 # pLinear
        b += bytes(3)                                   # reserved
        b += struct.pack('<ii', 1, 1)                   # xSampling, ySampling
    b += b'\0'                                          # end of the channel list
    b += b'compression\0' + b'compression\0' + struct.pack('<i', 1) + bytes([0])            # NO_COMPRESSION
    b += b'dataWindow\0' + b'box2i\0' + struct.pack('<i', 16) + struct.pack('<4i', 0, 0, 1, 0)     # xMin yMin xMax yMax
    b += b'displayWindow\0' + b'box2i\0' + struct.pack('<i', 16) + struct.pack('<4i', 0, 0, 1, 0)
    b += b'lineOrder\0' + b'lineOrder\0' + struct.pack('<i', 1) + bytes([0])                # INCREASING_Y
    b += b'pixelAspectRatio\0' + b'float\0' + struct.pack('<i', 4) + struct.pack('<f', 1.0)
    b += b'screenWindowCenter\0' + b'v2f\0' + struct.pack('<i', 8) + struct.pack('<2f', 0.0, 0.0)
    b += b'screenWindowWidth\0' + b'float\0' + struct.pack('<i', 4) + struct.pack('<f', 1.0)
    b += b'\0'                                          # end of the header
    # --- offset table: one uint64 per chunk, from the start of the file ---
    table_at = len(b)
    b += struct.pack('<Q', table_at + 8)
    # --- the chunk: int32 y, int32 data size, then per channel in list order `width` values ---
    b += struct.pack('<ii', 0, 12)
    b += struct.pack('<2e', 0.5, 1.5)                   # B
    b += struct.pack('<2e', 2.0, 65504.0)               # G
    b += struct.pack('<2e', -1.0, 6e-8)                 # R (a subnormal half)
    return b


def test_literal_file(tmp_path):
    from rnr_amd import exr
    fp = str(tmp_path / 'literal.exr')
    with open(fp, 'wb') as f:
        f.write(_literal_file())
    h = exr.read_header(fp)
    assert (h.width, h.height, h.x_min, h.y_min) == (2, 1, 0, 0)
    assert h.compression == 'NONE' and h.lines_per_chunk == 1 and h.line_order == 0 and h.row_bytes == 12
    assert [tuple(c) for c in h.channels] == [('B', exr.HALF, 0, 2), ('G', exr.HALF, 4, 2), ('R', exr.HALF, 8, 2)]
    assert exr.rgb_layout(h) == ((8, 2, exr.HALF), (4, 2, exr.HALF), (0, 2, exr.HALF))
    assert len(h.chunks) == 1 and h.chunks[0].y == 0 and h.chunks[0].size == 12 and h.chunks[0].lines == 1
    assert h.chunks[0].offset == len(_literal_file()) - 12
    _, payload, table = exr.load(fp)
    assert bytes(payload) == _literal_file()[-12:] and table == [(0, 0, 12, 0)]
    # the restatement reads the same file
    chans, info = er.decode(fp)
    assert chans['G'].tolist() == [[2.0, 65504.0]] and chans['R'][0, 0] == -1.0 and info['stored'] == ['none']


# ------------------------------------------------------------------------------------------------
# 3. round trips, and which chunks deflate shrinks
# ------------------------------------------------------------------------------------------------
# name -> (channels, write kwargs, what every chunk must report)
def _cases():
    h16 = lambda a: a.astype(np.float16)
    return {
        'zip-noise-half-5x16': ({k: _noise(16, 5, np.float16, i) for i, k in enumerate('RGB')}, dict(compression=er.ZIP), {'raw'}),
        'zip-ramp-half-5x16': ({k: h16(_ramp(16, 5, np.float32)) for k in 'RGB'}, dict(compression=er.ZIP), {'deflate'}),
        'zip-ramp-float-7x3': ({k: _ramp(3, 7, np.float32, 1.2345 + 0.1 * i) for i, k in enumerate('RGB')}, dict(compression=er.ZIP), {'deflate'}),
        'zip-noise-float-7x3': ({k: _noise(3, 7, np.float32, 10 + i) for i, k in enumerate('RGB')}, dict(compression=er.ZIP), {'raw'}),
        'zips-ramp-half-40x9': ({k: h16(_ramp(9, 40, np.float32)) for k in 'RGB'}, dict(compression=er.ZIPS), {'deflate'}),
        'none-37x21-window': ({k: _noise(21, 37, np.float32, 3) for k in 'RGB'}, dict(compression=er.NONE, origin=(-3, 11)), {'none'}),
        'zip-mixed-31x37': ({'R': h16(_ramp(37, 31, np.float32)), 'G': _ramp(37, 31, np.float32), 'B': h16(_ramp(37, 31, np.float32)),
                             'A': h16(_ramp(37, 31, np.float32)), 'Z': np.arange(37 * 31, dtype=np.uint32).reshape(37, 31)},
                            dict(compression=er.ZIP, decreasing=True, origin=(5, 7), force_raw=(1,)), {'raw', 'deflate'}),
    }


CASES = sorted(_cases())


@pytest.mark.parametrize('case', CASES)
def test_round_trip_and_storage(case, tmp_path):
    """Writer -> numpy decoder gives the arrays back; the reader's table agrees with the decoder about every chunk; each
    compressed case asserts whether its chunks were deflated or stored raw, and the suite holds both kinds."""
    from rnr_amd import exr
    chans, kw, want_kinds = _cases()[case]
    fp = str(tmp_path / (case + '.exr'))
    how = er.write(fp, chans, **kw)
    print(case, how)
    assert set(how) == want_kinds, how
    got, info = er.decode(fp)
    assert sorted(got) == sorted(chans)
    for k in chans:
        assert got[k].dtype == chans[k].dtype and np.array_equal(got[k].view(np.uint8), chans[k].view(np.uint8)), k
    h, w = chans['R'].shape
    assert (info['height'], info['width'], info['origin']) == (h, w, kw.get('origin', (0, 0)))
    # the reader: same geometry, and its payload + table give the same raw scanlines by the host restatement of the kernel
    hd, payload, table = exr.load(fp)
    assert (hd.height, hd.width, hd.x_min, hd.y_min, hd.row_bytes) == (h, w) + kw.get('origin', (0, 0)) + (info['row_bytes'],)
    assert hd.line_order == int(kw.get('decreasing', False))
    assert [bool(r[3]) for r in table] == [s == 'deflate' for s in info['stored']]
    raw = bytearray(h * hd.row_bytes)
    for src, dst, n, coded in table:
        part = bytes(payload[src:src + n])
        raw[dst:dst + n] = exr.unpack_chunk(part) if coded else part
    assert bytes(raw) == er.raw_scanlines(fp)[0].tobytes()


def test_both_storage_kinds_are_covered():
    kinds = set()
    for _, _, k in _cases().values():
        kinds |= k
    assert kinds == {'none', 'raw', 'deflate'}


# ------------------------------------------------------------------------------------------------
# 4. an .exr capture without a GPU
# ------------------------------------------------------------------------------------------------
def test_read_camera_of_an_exr_capture(golden, tmp_path):
    """37 x 53 (odd shorter side): the window is 36 x 36 from column 8, scale = 64 / 36 and offset (0, -8), exactly as for a PNG of
    that size (test_capture_cpu.test_odd_side_uses_the_photographs_own_crop); a data window that does not start at 0 changes
    nothing.  read_view without a GPU raises RuntimeError."""
    import scipy.io
    import torch
    import dataio
    g = golden('dataio_views')
    calib_fp = str(tmp_path / 'calib.mat')
    scipy.io.savemat(calib_fp, {k[6:]: g[k] for k in g.files if k.startswith('calib:')})
    img_dir = str(tmp_path / 'rgb0')
    os.makedirs(img_dir)
    for i, origin in enumerate([(0, 0), (-7, 100)]):
        er.write(os.path.join(img_dir, 'view_%d.exr' % i), {k: _ramp(37, 53, np.float16) for k in 'RGB'}, origin=origin)
    ds = dataio.ViewDataset(str(tmp_path), calib_fp, 'convert', (64, 64), 'all', load_img=True, img_dir=img_dir)
    assert ds.img_idx2fn == ['view_0.exr', 'view_1.exr']
    for i in range(2):
        v = ds.read_camera(i)
        assert np.array_equal(v['scale'].numpy(), np.array([64 / 36, 64 / 36], np.float32))
        assert np.array_equal(v['offset'].numpy(), np.array([0, -8], np.float32))
        p0 = g['calib:projs'][i]
        assert np.allclose(v['proj'].numpy()[0, -1], (p0[0, -1] - 8) * np.float32(64 / 36), rtol=1e-6, atol=1e-6)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='GPU'):
            ds.read_view(0)
        lp = dataio.LightProbeDataset(img_dir)
        with pytest.raises(RuntimeError, match='GPU'):
            lp[0]
    # .mat probes keep raising, by name
    with open(os.path.join(img_dir, 'z_probe.mat'), 'wb') as f:
        f.write(b'\0')
    lp = dataio.LightProbeDataset(img_dir)
    assert [os.path.basename(f) for f in lp.lp_fp_all] == ['view_0.exr', 'view_1.exr', 'z_probe.mat']
    with pytest.raises(NotImplementedError, match='z_probe.mat'):
        lp[2]


# ------------------------------------------------------------------------------------------------
# 5. refusals
# ------------------------------------------------------------------------------------------------
def _good(tmp_path, name='good.exr', **kw):
    fp = str(tmp_path / name)
    chans = {k: _ramp(37, 20, np.float16) for k in 'RGB'}
    chans.update(kw.pop('channels', {}))
    for k in kw.pop('drop', ()):
        del chans[k]
    er.write(fp, chans, **kw)
    with open(fp, 'rb') as f:
        return fp, bytearray(f.read())


def _table_at(data):
    """Offset of the offset table: behind the header's closing \\0."""
    pos = 8
    while data[pos] != 0:
        pos = data.index(b'\0', pos) + 1
        pos = data.index(b'\0', pos) + 1
        pos += 4 + struct.unpack_from('<i', data, pos)[0]
    return pos + 1


def _rewrite(fp, data):
    with open(fp, 'wb') as f:
        f.write(data)
    return fp


def _both(fp, exc, match):
    from rnr_amd import exr
    for fn in (exr.read_header, exr.load):
        with pytest.raises(exc, match=match) as e:
            fn(fp)
        assert os.path.basename(fp) in str(e.value), str(e.value)


def test_refusals_of_the_header(tmp_path):
    fp, data = _good(tmp_path)
    # magic, version
    _both(_rewrite(fp, b'\x89PNG' + data[4:]), ValueError, 'magic')
    _both(_rewrite(fp, data[:4] + b'\x01' + data[5:]), ValueError, 'version')
    # tiled, deep, multi-part; an unknown flag bit
    for bit, what in ((0x200, 'tiled'), (0x800, 'deep'), (0x1000, 'multi-part')):
        _both(_rewrite(fp, data[:4] + struct.pack('<I', 2 | bit) + data[8:]), NotImplementedError, what)
    _both(_rewrite(fp, data[:4] + struct.pack('<I', 2 | 0x2000) + data[8:]), ValueError, 'flags')
    # long names alone are accepted
    from rnr_amd import exr
    assert exr.read_header(_rewrite(fp, data[:4] + struct.pack('<I', 2 | 0x400) + data[8:])).width == 20
    # compression methods that are not read, by name
    at = data.index(b'compression\0compression\0') + 24 + 4
    for code, name in ((1, 'RLE'), (4, 'PIZ'), (5, 'PXR24'), (6, 'B44'), (7, 'B44A'), (8, 'DWAA'), (9, 'DWAB')):
        _both(_rewrite(fp, data[:at] + bytes([code]) + data[at + 1:]), NotImplementedError, name)
    _both(_rewrite(fp, data[:at] + bytes([77]) + data[at + 1:]), ValueError, 'compression')
    # line order
    at = data.index(b'lineOrder\0lineOrder\0') + 20 + 4
    _both(_rewrite(fp, data[:at] + bytes([2]) + data[at + 1:]), ValueError, 'lineOrder')
    # data window: empty, and beyond the size limit
    at = data.index(b'dataWindow\0box2i\0') + 17 + 4
    _both(_rewrite(fp, data[:at] + struct.pack('<4i', 0, 0, -1, 36) + data[at + 16:]), ValueError, 'dataWindow')
    _both(_rewrite(fp, data[:at] + struct.pack('<4i', 0, 0, 99999, 99999) + data[at + 16:]), ValueError, 'dataWindow.*limit')
    # a missing attribute: rename it
    _both(_rewrite(fp, bytes(data).replace(b'dataWindow\0', b'dataWindoW\0')), ValueError, 'dataWindow')


def test_refusals_of_the_channel_list(tmp_path):
    u32 = np.zeros((37, 20), np.uint32)
    fp, _ = _good(tmp_path, 'uint_r.exr', channels={'R': u32})
    _both(fp, NotImplementedError, 'channels.*R is UINT')
    fp, _ = _good(tmp_path, 'no_g.exr', drop=('G',))
    _both(fp, ValueError, 'channels: no G channel')
    fp, _ = _good(tmp_path, 'yc.exr', drop=('R', 'G', 'B'), channels={'Y': _ramp(37, 20, np.float16)})
    _both(fp, ValueError, 'channels: no R channel')
    fp, _ = _good(tmp_path, 'sub.exr', channels={'BY': _ramp(37, 20, np.float16)}, sampling={'BY': (2, 2)})
    _both(fp, ValueError, "channels: channel 'BY' is subsampled")
    # a UINT channel that is not a colour is skipped by its size
    from rnr_amd import exr
    fp, _ = _good(tmp_path, 'with_z.exr', channels={'Z': u32})
    assert exr.read_header(fp).row_bytes == 20 * (2 + 2 + 2 + 4)
    # not sorted by name: swap the names of B and G in place
    fp, data = _good(tmp_path, 'unsorted.exr')
    at = data.index(b'chlist\0') + 7 + 4
    assert data[at:at + 2] == b'B\0' and data[at + 18:at + 20] == b'G\0'
    data[at], data[at + 18] = ord('G'), ord('B')
    _both(_rewrite(fp, data), ValueError, 'channels.*not sorted')


def test_refusals_of_the_chunks(tmp_path):
    fp, data = _good(tmp_path)                          # ZIP, 37 rows: chunks at y = 0, 16, 32
    t = _table_at(data)
    offs = list(struct.unpack_from('<3Q', data, t))
    # truncated: inside the last chunk, inside the offset table, inside the header
    _both(_rewrite(fp, data[:-1]), ValueError, 'chunk 2 size.*truncated')
    _both(_rewrite(fp, data[:t + 10]), ValueError, 'offset table.*truncated')
    _both(_rewrite(fp, data[:40]), ValueError, 'good.exr')
    # an offset past the end, and one that points into the header
    d = bytearray(data); struct.pack_into('<Q', d, t + 8, len(data) + 5)
    _both(_rewrite(fp, d), ValueError, 'chunk 1 header')
    d = bytearray(data); struct.pack_into('<Q', d, t + 8, 8)
    _both(_rewrite(fp, d), ValueError, 'chunk 1.*in front of the pixel data')
    # duplicate y (so y = 16 is missing), y outside the window, y off the chunk boundary
    d = bytearray(data); struct.pack_into('<i', d, offs[1], 0)
    _both(_rewrite(fp, d), ValueError, 'chunk 1 y.*second chunk')
    d = bytearray(data); struct.pack_into('<Q', d, t + 8, offs[0])          # two table entries -> the same chunk: one is missing
    _both(_rewrite(fp, d), ValueError, 'chunk 1 y.*second chunk')
    d = bytearray(data); struct.pack_into('<i', d, offs[2], 48)
    _both(_rewrite(fp, d), ValueError, 'chunk 2 y.*outside the data window')
    d = bytearray(data); struct.pack_into('<i', d, offs[1], 17)
    _both(_rewrite(fp, d), ValueError, 'chunk 1 y.*chunk boundary')
    # a size beyond the raw size, a size of zero
    d = bytearray(data); struct.pack_into('<i', d, offs[0] + 4, 16 * 120 + 1)
    _both(_rewrite(fp, d), ValueError, 'chunk 0 size')
    d = bytearray(data); struct.pack_into('<i', d, offs[0] + 4, 0)
    _both(_rewrite(fp, d), ValueError, 'chunk 0 size')


def _with_chunk0(tmp_path, name, raw_len):
    """The good file with chunk 0 replaced by a deflate stream of raw_len bytes (the other chunks moved along)."""
    fp, data = _good(tmp_path, name)
    t = _table_at(data)
    offs = list(struct.unpack_from('<3Q', data, t))
    size0 = struct.unpack_from('<i', data, offs[0] + 4)[0]
    new = zlib.compress(bytes(raw_len))
    d = bytearray(data[:offs[0] + 4] + struct.pack('<i', len(new)) + new + data[offs[0] + 8 + size0:])
    for i in (1, 2):
        struct.pack_into('<Q', d, t + 8 * i, offs[i] + len(new) - size0)
    return _rewrite(fp, d)


def test_refusals_of_the_inflated_length(tmp_path):
    """One byte short and one byte long: load refuses; read_header, which inflates nothing, reads both."""
    from rnr_amd import exr
    want = 16 * 20 * 6
    assert exr.load(_with_chunk0(tmp_path, 'exact.exr', want))[2][0] == (0, 0, want, 1)
    for name, n in (('short.exr', want - 1), ('long.exr', want + 1)):
        fp = _with_chunk0(tmp_path, name, n)
        assert exr.read_header(fp).height == 37
        with pytest.raises(ValueError, match=name + ': chunk 0 inflated length'):
            exr.load(fp)
    # not a deflate stream at all
    fp, data = _good(tmp_path, 'garbage.exr')
    off0 = struct.unpack_from('<Q', data, _table_at(data))[0]
    data[off0 + 8:off0 + 12] = b'\xff\xff\xff\xff'
    with pytest.raises(ValueError, match='garbage.exr: chunk 0 data: zlib'):
        exr.load(_rewrite(fp, data))


def test_inflate_pool_is_bounded():
    from rnr_amd import exr
    assert exr.MAX_INFLATE_WORKERS <= 16
    import inspect
    assert 'cpu_count' not in inspect.getsource(exr)


# ------------------------------------------------------------------------------------------------
# 6. the entry points exist
# ------------------------------------------------------------------------------------------------
def test_symbols_are_declared_and_bound():
    from rnr_amd import _lib
    lib = _lib.load()
    for name in ('rnr_exr_unpack', 'rnr_photo_prepare_hdr'):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert (_lib.EXR_HALF, _lib.EXR_FLOAT) == (1, 2) and _lib.EXR_PASS_BYTES % 512 == 0
    assert [(p.name, p.type, p.pointer) for p in _lib.PARAMS['rnr_exr_unpack'][:4]] == \
        [('payload', 'uint8_t', 1), ('table', 'int64_t', 1), ('num_chunks', 'int', 0), ('raw', 'uint8_t', 1)]
