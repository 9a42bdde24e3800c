"""CPU: the OpenEXR writer of rnr_amd/exr.py without a GPU.  It is fed the chunk bytes of the tests' restatement
(tests/exr_ref.py: encode_chunk) and its files are read back by that restatement's decoder AND by the product's reader, to the
exact bits: every compression x type x size; the header field by field; which chunks are deflated and which stored raw, against
exr_ref.write for the same pixels; the lazy raw callable; refusals that leave no file."""
import os
import struct

import numpy as np
import pytest

import exr_ref as er

COMPRESSIONS = {'none': er.NONE, 'zips': er.ZIPS, 'zip': er.ZIP}
DTYPES = {'half': np.float16, 'float': np.float32}
UINTS = {'half': np.uint16, 'float': np.uint32}
SHAPES = [(1, 1), (17, 5), (33, 40)]          # (H, W): one value; ragged, two ZIP chunks; three ZIP chunks, the last of one line


def _ramp(h, w, ptype, k=0):
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    return ((y * 0.25 + x * 0.125 + 0.5) * (k + 1)).astype(DTYPES[ptype])


def _random_bits(h, w, ptype, seed):
    """Every byte random: NaNs, infinities and subnormals included.  The writer moves bytes, so the comparison is on bits."""
    u = UINTS[ptype]
    return np.random.RandomState(seed).randint(0, 256, (h, w, u().itemsize)).astype(np.uint8).view(u).reshape(h, w).view(DTYPES[ptype])


def _pixels(h, w, ptype, kind, seed=0):
    """-> {'R' | 'G' | 'B': [h,w]}: a ramp (deflate shrinks it), random bits (it does not), or a ramp whose rows from 16 on are
    random."""
    out = {}
    for k, name in enumerate('RGB'):
        a = _ramp(h, w, ptype, k)
        if kind == 'random':
            a = _random_bits(h, w, ptype, seed + k)
        elif kind == 'mixed':
            a[16:] = _random_bits(h - 16, w, ptype, seed + k)
        out[name] = a
    return out


def _raw_chunks(chans, lines):
    """The raw bytes of every chunk, built here: per scanline the B, the G, the R run, little endian."""
    h = chans['R'].shape[0]
    u = UINTS['half' if chans['R'].dtype == np.float16 else 'float']
    return [b''.join(chans[n][y].view(u).astype(u().dtype.newbyteorder('<')).tobytes() for y in range(top, min(top + lines, h)) for n in 'BGR')
            for top in range(0, h, lines)]


def _chunks(chans, compression):
    raw = _raw_chunks(chans, er.LINES[COMPRESSIONS[compression]])
    return raw, (raw if compression == 'none' else [er.encode_chunk(r)[1] for r in raw])


def _same_bits(a, b):
    u = UINTS['half' if a.dtype == np.float16 else 'float']
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(u), b.view(u))


def _load_raw(fp):
    """The product reader's view of the file: rnr_amd.exr.load, the coding undone on the host -> (Header, raw scanline bytes)."""
    from rnr_amd import exr
    header, payload, table = exr.load(fp)
    raw = bytearray(header.height * header.row_bytes)
    for src, dst, n, coded in table:
        t = bytes(payload[src:src + n])
        raw[dst:dst + n] = exr.unpack_chunk(t) if coded else t
    return header, bytes(raw)


@pytest.mark.parametrize('shape', SHAPES, ids=['%dx%d' % s for s in SHAPES])
@pytest.mark.parametrize('ptype', ['half', 'float'])
@pytest.mark.parametrize('compression', ['none', 'zips', 'zip'])
@pytest.mark.parametrize('kind', ['ramp', 'random'])
def test_round_trip_through_both_readers(compression, ptype, shape, kind, tmp_path):
    from rnr_amd import exr
    h, w = shape
    chans = _pixels(h, w, ptype, kind, seed=h * w)
    raw, chunks = _chunks(chans, compression)
    fp = str(tmp_path / 'out.exr')
    how = exr.write(fp, w, h, ptype, compression, chunks, raw_chunk=lambda i: raw[i])
    assert len(how) == len(raw) and set(how) <= ({'none'} if compression == 'none' else {'raw', 'deflate'})
    got, info = er.decode(fp)
    assert sorted(got) == ['B', 'G', 'R'] and info['stored'] == how and info['origin'] == (0, 0)
    for n in 'RGB':
        assert _same_bits(got[n], chans[n]), n
    header, data = _load_raw(fp)
    assert (header.width, header.height) == (w, h) and data == b''.join(raw)
    # the same pixels through the restatement's writer: the same storage decisions, and the same file
    ref = str(tmp_path / 'ref.exr')
    assert er.write(ref, chans, compression=COMPRESSIONS[compression]) == how
    assert open(ref, 'rb').read() == open(fp, 'rb').read()


def _attributes(data):
    """The header's attributes in file order: [(name, type, value bytes)], and the offset behind the header."""
    assert data[:4] == bytes([0x76, 0x2f, 0x31, 0x01]) and data[4:8] == struct.pack('<I', 2)
    pos, out = 8, []
    while data[pos] != 0:
        end = data.index(b'\0', pos)
        name, pos = data[pos:end].decode(), end + 1
        end = data.index(b'\0', pos)
        kind, pos = data[pos:end].decode(), end + 1
        size = struct.unpack_from('<i', data, pos)[0]
        out.append((name, kind, data[pos + 4:pos + 4 + size]))
        pos += 4 + size
    return out, pos + 1


@pytest.mark.parametrize('ptype, compression', [('half', 'zip'), ('float', 'zips'), ('half', 'none')])
def test_header_field_by_field(ptype, compression, tmp_path):
    from rnr_amd import exr
    h, w = 33, 40
    chans = _pixels(h, w, ptype, 'ramp')
    raw, chunks = _chunks(chans, compression)
    fp = str(tmp_path / 'header.exr')
    exr.write(fp, w, h, ptype, compression, chunks)
    hd = exr.read_header(fp)
    size, code = (2, exr.HALF) if ptype == 'half' else (4, exr.FLOAT)
    lines = 16 if compression == 'zip' else 1
    assert (hd.width, hd.height, hd.x_min, hd.y_min) == (w, h, 0, 0)
    assert hd.channels == (exr.Channel('B', code, 0, size), exr.Channel('G', code, size * w, size), exr.Channel('R', code, 2 * size * w, size))
    assert hd.row_bytes == 3 * w * size and hd.compression == compression.upper() and hd.lines_per_chunk == lines and hd.line_order == 0
    assert [c.y for c in hd.chunks] == list(range(0, h, lines)) and [c.lines for c in hd.chunks] == [min(lines, h - y) for y in range(0, h, lines)]
    assert exr.rgb_layout(hd) == ((2 * size * w, size, code), (size * w, size, code), (0, size, code))
    data = open(fp, 'rb').read()
    attrs, table_at = _attributes(data)
    entry = struct.pack('<iB3xii', code, 0, 1, 1)
    window = struct.pack('<4i', 0, 0, w - 1, h - 1)
    assert attrs == [('channels', 'chlist', b'B\0' + entry + b'G\0' + entry + b'R\0' + entry + b'\0'),
                     ('compression', 'compression', bytes([COMPRESSIONS[compression]])),
                     ('dataWindow', 'box2i', window), ('displayWindow', 'box2i', window),
                     ('lineOrder', 'lineOrder', b'\0'),
                     ('pixelAspectRatio', 'float', struct.pack('<f', 1.0)),
                     ('screenWindowCenter', 'v2f', struct.pack('<2f', 0.0, 0.0)),
                     ('screenWindowWidth', 'float', struct.pack('<f', 1.0))]
    # the offset table, then the chunks as (y, size, data), back to back up to the file's end
    offsets = struct.unpack_from('<%dQ' % len(hd.chunks), data, table_at)
    pos = table_at + 8 * len(hd.chunks)
    for off, c in zip(offsets, hd.chunks):
        assert off == pos and struct.unpack_from('<ii', data, off) == (c.y, c.size) and c.offset == off + 8
        pos += 8 + c.size
    assert pos == len(data)


def test_what_deflate_shrinks_and_what_it_does_not(tmp_path):
    """A 16 x 40 FLOAT chunk of random bytes and a 1 x 5 HALF ZIPS chunk of random bytes are stored raw (7680 -> 7691 and 30 -> 39
    at level 6 with zlib 1.2.13); a smooth 16 x 40 HALF ramp is deflated (3840 -> 244)."""
    from rnr_amd import exr
    for (h, w), ptype, compression, kind, want, n in (((16, 40), 'float', 'zip', 'random', 'raw', 7680),
                                                      ((1, 5), 'half', 'zips', 'random', 'raw', 30),
                                                      ((16, 40), 'half', 'zip', 'ramp', 'deflate', 3840)):
        chans = _pixels(h, w, ptype, kind, seed=3)
        raw, chunks = _chunks(chans, compression)
        fp = str(tmp_path / ('%s_%s.exr' % (kind, ptype)))
        assert len(raw) == 1 and len(raw[0]) == n
        assert exr.write(fp, w, h, ptype, compression, chunks, raw_chunk=lambda i: raw[i]) == [want]
        stored = exr.read_header(fp).chunks[0].size
        print('%d x %d %s %s %s: %d -> %d bytes stored' % (h, w, ptype, compression, kind, n, stored))
        assert (stored == n) if want == 'raw' else (stored < n)
        got, info = er.decode(fp)
        assert info['stored'] == [want] and all(_same_bits(got[k], chans[k]) for k in 'RGB')


@pytest.mark.parametrize('ptype', ['half', 'float'])
@pytest.mark.parametrize('level', [1, 6, 9])
def test_both_kinds_in_one_file_and_the_lazy_raw_callable(ptype, level, tmp_path):
    """40 x 40, rows 16.. random: ZIP chunk 0 shrinks, chunks 1 and 2 do not.  The returned list is exr_ref.write's; raw_chunk is
    asked for exactly the chunks stored raw, once each; without it the writer undoes the coding on the host, to the same file."""
    from rnr_amd import exr
    h = w = 40
    chans = _pixels(h, w, ptype, 'mixed', seed=11)
    raw, chunks = _chunks(chans, 'zip')
    asked = []

    def raw_chunk(i):
        asked.append(i)
        return raw[i]

    fp, ref, fp2 = (str(tmp_path / n) for n in ('lazy.exr', 'ref.exr', 'host.exr'))
    how = exr.write(fp, w, h, ptype, 'zip', chunks, raw_chunk=raw_chunk, level=level)
    assert how == ['deflate', 'raw', 'raw'] and asked == [1, 2]
    assert how == er.write(ref, chans, compression=er.ZIP, level=level)
    assert open(fp, 'rb').read() == open(ref, 'rb').read()
    assert exr.write(fp2, w, h, ptype, 'zip', chunks, level=level) == how and open(fp2, 'rb').read() == open(fp, 'rb').read()
    got, info = er.decode(fp)
    assert info['stored'] == how and all(_same_bits(got[k], chans[k]) for k in 'RGB')
    assert _load_raw(fp)[1] == b''.join(raw)
    # a file of ramps alone never asks
    asked.clear()
    smooth = _pixels(h, w, ptype, 'ramp')
    assert exr.write(fp, w, h, ptype, 'zip', _chunks(smooth, 'zip')[1], raw_chunk=raw_chunk) == ['deflate'] * 3 and asked == []
    # zlib streams made by the caller (one pool for several files) give the same file
    streams = exr.deflate_chunks(chunks, level)
    assert exr.write(fp2, w, h, ptype, 'zip', chunks, raw_chunk=lambda i: raw[i], level=level, deflated=streams) == how
    assert open(fp2, 'rb').read() == open(ref, 'rb').read()


def test_pack_chunk_is_the_restatements_coding():
    from rnr_amd import exr
    assert exr.pack_chunk(bytes.fromhex('010203040506')) == bytes.fromhex('0182827d8282')
    for n in (2, 6, 30, 254, 256, 7680):
        raw = bytes(np.random.RandomState(n).randint(0, 256, n).astype(np.uint8))
        assert exr.pack_chunk(raw) == er.encode_chunk(raw)[1] and exr.unpack_chunk(exr.pack_chunk(raw)) == raw


def test_names_and_codes_are_the_same_arguments(tmp_path):
    from rnr_amd import exr
    chans = _pixels(5, 7, 'half', 'ramp')
    _, chunks = _chunks(chans, 'zips')
    a, b = str(tmp_path / 'a.exr'), str(tmp_path / 'b.exr')
    exr.write(a, 7, 5, 'half', 'zips', chunks)
    exr.write(b, 7, 5, exr.HALF, 2, [bytearray(c) for c in chunks], workers=1)
    assert open(a, 'rb').read() == open(b, 'rb').read()
    assert exr.chunk_sizes(7, 5, 'HALF', 'ZIP') == (42, 16, [210]) and exr.chunk_sizes(7, 33, 'float', 'zip') == (84, 16, [1344, 1344, 84])


BAD = {
    'pixel_type uint': dict(pixel_type=0), 'pixel_type name': dict(pixel_type='double'), 'pixel_type 3': dict(pixel_type=3),
    'compression piz': dict(compression='piz'), 'compression rle code': dict(compression=1), 'compression 10': dict(compression=10),
    'width 0': dict(width=0), 'height 0': dict(height=0), 'width < 0': dict(width=-7), 'width float': dict(width=7.0),
    'too large': dict(width=1 << 16, height=1 << 16),
    'one chunk short': dict(drop=1), 'one chunk more': dict(extra=1), 'a chunk one byte short': dict(trim=1),
    'a chunk that is not bytes': dict(chunk=17),
    'level 10': dict(level=10), 'level name': dict(level='best'),
    'raw_chunk not callable': dict(raw_chunk=b'raw'),
    'deflated of another length': dict(deflated=[b'x']),
}


@pytest.mark.parametrize('tag', sorted(BAD))
def test_bad_arguments_raise_before_a_byte_is_written(tag, tmp_path):
    from rnr_amd import exr
    over = dict(BAD[tag])
    chans = _pixels(5, 7, 'half', 'ramp')
    _, chunks = _chunks(chans, 'zips')
    if over.pop('drop', 0):
        chunks = chunks[:-1]
    if over.pop('extra', 0):
        chunks = chunks + chunks[:1]
    if over.pop('trim', 0):
        chunks = chunks[:2] + [chunks[2][:-1]] + chunks[3:]
    if 'chunk' in over:
        chunks = chunks[:1] + [over.pop('chunk')] + chunks[2:]
    args = dict(width=7, height=5, pixel_type='half', compression='zips', chunks=chunks)
    args.update(over)
    fp = str(tmp_path / 'never.exr')
    with pytest.raises(ValueError):
        exr.write(fp, **args)
    assert not os.path.exists(fp)


def test_a_raw_callable_of_the_wrong_size_leaves_no_file(tmp_path):
    from rnr_amd import exr
    chans = _pixels(1, 5, 'half', 'random', seed=3)
    _, chunks = _chunks(chans, 'zips')
    fp = str(tmp_path / 'never.exr')
    with pytest.raises(ValueError, match='raw_chunk'):
        exr.write(fp, 5, 1, 'half', 'zips', chunks, raw_chunk=lambda i: b'short')
    assert not os.path.exists(fp)


def test_the_writer_needs_neither_torch_nor_the_library():
    """rnr_amd/exr.py stays importable where nothing is built: it imports only the standard library."""
    import ast
    from rnr_amd import exr
    tree = ast.parse(open(exr.__file__).read())
    mods = {n.module if isinstance(n, ast.ImportFrom) else a.name for n in ast.walk(tree) if isinstance(n, (ast.Import, ast.ImportFrom))
            for a in (n.names if isinstance(n, ast.Import) else [None])}
    assert mods <= {'collections', 'struct', 'zlib', 'concurrent.futures', 'os'}, mods
