"""A strict reader and a writer of single-part OpenEXR scanline files, as the OpenEXR file-layout document defines them: pure Python
plus zlib, no GPU, no torch.

What is read: magic 76 2f 31 01, version 2 (of the flag bits only 0x400, long names), the header attributes `channels`,
`compression`, `dataWindow` and `lineOrder` (every other attribute is skipped by its size), the offset table and the chunks of
the compressions NONE, ZIPS and ZIP.  R, G and B must be HALF or FLOAT channels with sampling 1, 1; other channels are skipped.
Tiled, deep and multi-part files and the other compression methods raise NotImplementedError; a malformed file raises ValueError
naming the file and the field.

EVERYTHING is validated here, before a byte is uploaded: the file length against every offset and size, every chunk's y inside
the data window, on a chunk boundary and seen exactly once, every inflated length, the window's sizes against MAX_RAW_BYTES.  The
table `load` returns is what rnr_exr_unpack trusts (include/rnr_hip.h states that contract), so no input file can make a kernel
read or write outside its buffers.

    read_header(fp) -> Header    sizes, channel layout and chunk table: no pixel decode (what ViewDataset.read_camera needs)
    load(fp)        -> (Header, payload bytearray, table rows (src_offset, dst_offset, bytes, coded))

What is written (`write`): a version-2 file with the eight required attributes, B, G and R channels of ONE type (HALF or FLOAT),
compression NONE, ZIPS or ZIP, increasing line order, a data window from (0, 0).  The caller hands over each chunk's bytes as the
format gives them to deflate (rnr_exr_pack makes them on the device; `pack_chunk` restates the coding on the host); this module
deflates on the same bounded thread pool, stores a chunk that does not shrink raw, and lays out header, offset table and chunks.
Every file it writes is one `load` reads.

    write(fp, width, height, pixel_type, compression, chunks, ...) -> ['none' | 'raw' | 'deflate' per chunk]
"""
import collections
import struct
import zlib
from concurrent.futures import ThreadPoolExecutor

MAGIC = b'\x76\x2f\x31\x01'
FLAG_TILED, FLAG_LONG_NAMES, FLAG_DEEP, FLAG_MULTIPART = 0x200, 0x400, 0x800, 0x1000
UINT, HALF, FLOAT = 0, 1, 2
TYPE_BYTES = {UINT: 4, HALF: 2, FLOAT: 4}
# compression code -> (name, scanlines per chunk or None: not read here)
COMPRESSIONS = {0: ('NONE', 1), 1: ('RLE', None), 2: ('ZIPS', 1), 3: ('ZIP', 16), 4: ('PIZ', None), 5: ('PXR24', None),
                6: ('B44', None), 7: ('B44A', None), 8: ('DWAA', None), 9: ('DWAB', None)}
# the raw scanline buffer of one file: width x height x bytes per pixel
MAX_RAW_BYTES = 1 << 31
# zlib releases the GIL; a fixed bound, never the machine's processor count
MAX_INFLATE_WORKERS = 16

# name, type, offset of the channel's run inside a scanline (bytes), size of one value
Channel = collections.namedtuple('Channel', 'name type offset size')
# y: the chunk's first scanline (file coordinates); offset, size: its data (behind the 8-byte chunk header) in the file
Chunk = collections.namedtuple('Chunk', 'y offset size lines')
Header = collections.namedtuple('Header', 'width height x_min y_min channels row_bytes compression lines_per_chunk line_order chunks')


class _Cursor:
    """Reads of a file that name the file and the field when they run past its end."""

    def __init__(self, fh, fp, size):
        self.fh, self.fp, self.size = fh, fp, size

    def fail(self, field, why):
        raise ValueError('%s: %s: %s' % (self.fp, field, why))

    def at(self, pos, n, field):
        if pos < 0 or n < 0 or pos + n > self.size:
            self.fail(field, 'bytes [%d, %d) lie outside the file of %d bytes (truncated?)' % (pos, pos + n, self.size))
        self.fh.seek(pos)
        data = self.fh.read(n)
        if len(data) != n:
            self.fail(field, 'short read at %d' % pos)
        return data

    def take(self, n, field):
        return self.at(self.fh.tell(), n, field)

    def name(self, limit, field):
        """A NUL-terminated string of at most `limit` bytes; '' is the end of a list."""
        pos = self.fh.tell()
        data = self.fh.read(limit + 1)
        end = data.find(b'\0')
        if end < 0:
            self.fail(field, 'no NUL within %d bytes at offset %d (truncated or not a name)' % (limit + 1, pos))
        self.fh.seek(pos + end + 1)
        return data[:end].decode('latin-1')


def _channels(data, fp, limit):
    """The value of the `channels` attribute -> [(name, type, x sampling, y sampling)]."""
    out, pos = [], 0
    while True:
        end = data.find(b'\0', pos, pos + limit + 1)
        if end < 0:
            raise ValueError('%s: channels: unterminated channel name at byte %d of the list' % (fp, pos))
        if end == pos:
            if end + 1 != len(data):
                raise ValueError('%s: channels: %d bytes behind the end of the list' % (fp, len(data) - end - 1))
            return out
        if end + 17 > len(data):
            raise ValueError('%s: channels: the entry of channel %r is cut short' % (fp, data[pos:end]))
        ctype, _plinear, xs, ys = struct.unpack_from('<iB3xii', data, end + 1)
        out.append((data[pos:end].decode('latin-1'), ctype, xs, ys))
        pos = end + 17


def _parse(cur):
    fp = cur.fp
    head = cur.at(0, 8, 'magic and version')
    if head[:4] != MAGIC:
        cur.fail('magic', 'expected 76 2f 31 01, found %s' % head[:4].hex(' '))
    word = struct.unpack('<I', head[4:])[0]
    version, flags = word & 0xff, word & ~0xff
    if version != 2:
        cur.fail('version', 'expected 2, found %d' % version)
    for bit, what in ((FLAG_TILED, 'tiled'), (FLAG_DEEP, 'deep'), (FLAG_MULTIPART, 'multi-part')):
        if flags & bit:
            raise NotImplementedError('%s: version flags: %s files (flag 0x%x) are not read; single-part scanline files only'
                                      % (fp, what, bit))
    if flags & ~FLAG_LONG_NAMES:
        cur.fail('version flags', 'unknown bits 0x%x' % (flags & ~FLAG_LONG_NAMES))
    limit = 255 if flags & FLAG_LONG_NAMES else 31
    attrs = {}
    while True:
        name = cur.name(limit, 'header attribute name')
        if not name:
            break
        kind = cur.name(limit, 'type of attribute %r' % name)
        size = struct.unpack('<i', cur.take(4, 'size of attribute %r' % name))[0]
        if size < 0:
            cur.fail('size of attribute %r' % name, 'negative (%d)' % size)
        pos = cur.fh.tell()
        if name in ('channels', 'compression', 'dataWindow', 'lineOrder'):
            if name in attrs:
                cur.fail(name, 'the attribute appears twice')
            attrs[name] = (kind, cur.at(pos, size, name))
        elif pos + size > cur.size:
            cur.fail('attribute %r' % name, 'its %d bytes end behind the file (truncated?)' % size)
        cur.fh.seek(pos + size)
    for name, kind, size in (('channels', 'chlist', None), ('compression', 'compression', 1), ('dataWindow', 'box2i', 16),
                             ('lineOrder', 'lineOrder', 1)):
        if name not in attrs:
            cur.fail(name, 'the header has no such attribute')
        if attrs[name][0] != kind or (size is not None and len(attrs[name][1]) != size):
            cur.fail(name, 'expected type %s%s, found %r of %d bytes'
                     % (kind, '' if size is None else ' of %d bytes' % size, attrs[name][0], len(attrs[name][1])))
    # compression
    code = attrs['compression'][1][0]
    if code not in COMPRESSIONS:
        cur.fail('compression', 'unknown method %d' % code)
    method, lines = COMPRESSIONS[code]
    if lines is None:
        raise NotImplementedError('%s: compression: %s is not read here (NONE, ZIPS and ZIP are)' % (fp, method))
    # line order
    order = attrs['lineOrder'][1][0]
    if order not in (0, 1):
        cur.fail('lineOrder', 'expected 0 (increasing y) or 1 (decreasing y) in a scanline file, found %d' % order)
    # data window
    x_min, y_min, x_max, y_max = struct.unpack('<4i', attrs['dataWindow'][1])
    width, height = x_max - x_min + 1, y_max - y_min + 1
    if width <= 0 or height <= 0:
        cur.fail('dataWindow', 'width %d and height %d must be positive (%d, %d) - (%d, %d)' % (width, height, x_min, y_min, x_max, y_max))
    # channels
    entries = _channels(attrs['channels'][1], fp, limit)
    names = [e[0] for e in entries]
    if names != sorted(names) or len(set(names)) != len(names):
        cur.fail('channels', 'the list %r is not sorted by name without repeats' % names)
    channels, offset = [], 0
    for name, ctype, xs, ys in entries:
        if ctype not in TYPE_BYTES:
            cur.fail('channels', 'channel %r has unknown pixel type %d' % (name, ctype))
        if xs != 1 or ys != 1:
            cur.fail('channels', 'channel %r is subsampled (%d, %d); sampling 1, 1 only' % (name, xs, ys))
        if name in ('R', 'G', 'B') and ctype == UINT:
            raise NotImplementedError('%s: channels: channel %s is UINT; HALF and FLOAT colour channels only' % (fp, name))
        channels.append(Channel(name, ctype, offset * width, TYPE_BYTES[ctype]))
        offset += TYPE_BYTES[ctype]
    for want in 'RGB':
        if want not in names:
            cur.fail('channels', 'no %s channel among %r (luminance-chroma and grey files are not read)' % (want, names))
    row_bytes = offset * width
    if row_bytes * height > MAX_RAW_BYTES:
        cur.fail('dataWindow', '%d x %d pixels of %d bytes exceed the limit of %d bytes' % (width, height, offset, MAX_RAW_BYTES))
    # offset table and chunk headers
    count = (height + lines - 1) // lines
    table_at = cur.fh.tell()
    offsets = struct.unpack('<%dQ' % count, cur.at(table_at, 8 * count, 'offset table (%d entries)' % count))
    chunks, seen = [], set()
    for i, off in enumerate(offsets):
        field = 'chunk %d' % i
        if off < table_at + 8 * count:
            cur.fail(field, 'offset %d points in front of the pixel data' % off)
        y, size = struct.unpack('<ii', cur.at(off, 8, '%s header at offset %d' % (field, off)))
        if not (y_min <= y <= y_max):
            cur.fail(field + ' y', '%d is outside the data window rows [%d, %d]' % (y, y_min, y_max))
        if (y - y_min) % lines:
            cur.fail(field + ' y', '%d is not on a chunk boundary (%d + k * %d)' % (y, y_min, lines))
        if y in seen:
            cur.fail(field + ' y', 'a second chunk for scanline %d (and so one scanline block has none)' % y)
        seen.add(y)
        n_lines = min(lines, y_max - y + 1)
        raw = n_lines * row_bytes
        if size <= 0 or size > raw or (code == 0 and size != raw):
            cur.fail(field + ' size', '%d, for %d bytes of %s scanlines' % (size, raw, method))
        if off + 8 + size > cur.size:
            cur.fail(field + ' size', 'data [%d, %d) ends behind the file of %d bytes (truncated?)' % (off + 8, off + 8 + size, cur.size))
        chunks.append(Chunk(y, off + 8, size, n_lines))
    # count chunks with distinct y on distinct boundaries inside the window: every block is there exactly once
    return Header(width, height, x_min, y_min, tuple(channels), row_bytes, method, lines, order, tuple(chunks))


def read_header(fp):
    """Sizes, channel layout and chunk table of an OpenEXR file, fully validated against the file's length; no pixel is decoded."""
    import os
    with open(fp, 'rb') as fh:
        return _parse(_Cursor(fh, fp, os.fstat(fh.fileno()).st_size))


def rgb_layout(header):
    """-> ((offset, stride, type) of R, of G, of B) inside a scanline of the raw buffer: rnr_photo_prepare_hdr's addressing."""
    by_name = {c.name: c for c in header.channels}
    return tuple((by_name[k].offset, by_name[k].size, by_name[k].type) for k in 'RGB')


def _inflate(job):
    fp, index, data, want = job
    try:
        d = zlib.decompressobj()
        out = d.decompress(data, want + 1)
    except zlib.error as e:
        raise ValueError('%s: chunk %d data: zlib: %s' % (fp, index, e))
    if len(out) != want or not d.eof or d.unconsumed_tail:
        raise ValueError('%s: chunk %d inflated length: %s, expected exactly %d bytes'
                         % (fp, index, 'more than %d' % want if len(out) > want or d.unconsumed_tail else
                            ('%d' % len(out)) + ('' if d.eof else ' and the stream is cut short'), want))
    return out


def load(fp, workers=MAX_INFLATE_WORKERS):
    """-> (Header, payload, table): payload holds the chunks one behind the other, compressed ones inflated; table rows are
    (src_offset into payload, dst_offset into the raw scanline buffer of height * row_bytes bytes, bytes, coded), coded = 1 where
    the predictor and the interleave are still to be undone (rnr_exr_unpack; `unpack_chunk` restates them on the host)."""
    import os
    with open(fp, 'rb') as fh:
        cur = _Cursor(fh, fp, os.fstat(fh.fileno()).st_size)
        h = _parse(cur)
        data = [cur.at(c.offset, c.size, 'chunk %d data' % i) for i, c in enumerate(h.chunks)]
    raw_len = [c.lines * h.row_bytes for c in h.chunks]
    # the format's rule: a chunk that deflate did not shrink is stored raw, at its raw size
    coded = [h.compression != 'NONE' and len(d) < n for d, n in zip(data, raw_len)]
    jobs = [(fp, i, data[i], raw_len[i]) for i in range(len(data)) if coded[i]]
    if jobs:
        workers = max(1, min(int(workers), MAX_INFLATE_WORKERS, len(jobs)))
        if workers == 1:
            done = [_inflate(j) for j in jobs]
        else:
            with ThreadPoolExecutor(workers) as pool:
                done = list(pool.map(_inflate, jobs))
        for j, out in zip(jobs, done):
            data[j[1]] = out
    table, pos = [], 0
    for c, d, n, k in zip(h.chunks, data, raw_len, coded):
        assert len(d) == n
        table.append((pos, (c.y - h.y_min) * h.row_bytes, n, int(k)))
        pos += n
    return h, bytearray().join(data), table


def unpack_chunk(t):
    """The two reconstruction steps of a ZIP / ZIPS chunk on the host, as rnr_exr_unpack does them: bytes after inflate -> raw."""
    n = len(t)
    out, half, run = bytearray(n), (n + 1) // 2, 0
    acc = bytearray(n)
    for i, b in enumerate(t):
        run = b if i == 0 else (run + b - 128) & 0xff
        acc[i] = run
    out[0::2] = acc[:half]
    out[1::2] = acc[half:]
    return bytes(out)


def pack_chunk(raw):
    """The inverse of `unpack_chunk` on the host, as rnr_exr_pack(coded = 1) does it: raw scanline bytes -> the bytes for deflate."""
    raw = bytes(raw)
    split = raw[0::2] + raw[1::2]
    return split[:1] + bytes((b - a + 128) & 0xff for a, b in zip(split, split[1:]))


# ---------------------------------------------------------------------------------------------------
# the writer
# ---------------------------------------------------------------------------------------------------
_TYPE_NAMES = {'half': HALF, 'float': FLOAT}
_COMPRESSION_CODES = {name: code for code, (name, lines) in COMPRESSIONS.items() if lines is not None}


def pixel_type_code(pixel_type):
    """'half' | 'float' (any case) or HALF | FLOAT -> HALF | FLOAT; ValueError otherwise."""
    code = _TYPE_NAMES.get(pixel_type.lower()) if isinstance(pixel_type, str) else pixel_type
    if code not in (HALF, FLOAT) or isinstance(code, bool):
        raise ValueError("pixel_type must be 'half' or 'float' (exr.HALF or exr.FLOAT), got %r" % (pixel_type,))
    return code


def compression_code(compression):
    """'none' | 'zips' | 'zip' (any case) or the format's code 0 | 2 | 3 -> (code, name, scanlines per chunk); ValueError otherwise."""
    code = _COMPRESSION_CODES.get(compression.upper()) if isinstance(compression, str) else compression
    if code not in _COMPRESSION_CODES.values() or isinstance(code, bool):
        raise ValueError("compression must be 'none', 'zips' or 'zip' (0, 2 or 3), got %r: the other methods are not written"
                         % (compression,))
    return (code,) + COMPRESSIONS[code]


def chunk_sizes(width, height, pixel_type, compression):
    """-> (row_bytes, scanlines per chunk, [raw bytes of every chunk in increasing y]) of the file `write` lays out; validates
    the four arguments."""
    size = TYPE_BYTES[pixel_type_code(pixel_type)]
    _, _, lines = compression_code(compression)
    for v, name in ((width, 'width'), (height, 'height')):
        if isinstance(v, bool) or not isinstance(v, int) or v <= 0:
            raise ValueError('%s must be a positive integer, got %r' % (name, v))
    row_bytes = 3 * width * size
    if row_bytes * height > MAX_RAW_BYTES:
        raise ValueError('%d x %d pixels of %d bytes exceed the limit of %d bytes' % (width, height, 3 * size, MAX_RAW_BYTES))
    return row_bytes, lines, [min(lines, height - y) * row_bytes for y in range(0, height, lines)]


def check_level(level):
    if isinstance(level, bool) or not isinstance(level, int) or not (-1 <= level <= 9):
        raise ValueError('level must be an integer in -1..9 (zlib), got %r' % (level,))


def _deflate(job):
    data, level = job
    return zlib.compress(data, level)


def deflate_chunks(chunks, level=6, workers=MAX_INFLATE_WORKERS):
    """zlib streams of `chunks` (bytes-like) in their order, on a thread pool of at most MAX_INFLATE_WORKERS (zlib releases the
    GIL).  `write` calls it per file; a caller with several files deflates all their chunks in one call and passes the slices on."""
    check_level(level)
    jobs = [(c, level) for c in chunks]
    workers = max(1, min(int(workers), MAX_INFLATE_WORKERS, len(jobs)))
    if workers == 1:
        return [_deflate(j) for j in jobs]
    with ThreadPoolExecutor(workers) as pool:
        return list(pool.map(_deflate, jobs))


def _attribute(name, kind, value):
    return name.encode('latin-1') + b'\0' + kind.encode('latin-1') + b'\0' + struct.pack('<i', len(value)) + value


def write(fp, width, height, pixel_type, compression, chunks, raw_chunk=None, level=6, workers=MAX_INFLATE_WORKERS, deflated=None):
    """Write a version-2 single-part scanline file of B, G, R channels of `pixel_type` ('half' | 'float').

    chunks:    one bytes-like per chunk in increasing y (16 scanlines a chunk for 'zip', 1 for 'zips' and 'none'; sizes:
               `chunk_sizes`).  For 'none' the raw scanlines (per scanline the run of B, of G, of R values, little endian); for
               'zip' / 'zips' those bytes CODED for deflate (rnr_exr_pack(coded = 1), `pack_chunk`).
    raw_chunk: callable(i) -> the raw bytes of chunk i, asked only for a chunk whose deflated size is not below its raw size:
               the format stores such a chunk raw, and the reader tells the two apart by the size.  None: the coding is undone
               on the host (`unpack_chunk`: slow, but such chunks are rare).
    level:     zlib's, -1..9.  workers: the deflate pool, at most MAX_INFLATE_WORKERS.  deflated: the zlib streams of `chunks`
               when the caller has made them already (`deflate_chunks`).
    The header holds the eight required attributes: channels, compression, dataWindow = displayWindow = (0, 0, W-1, H-1),
    lineOrder increasing, pixelAspectRatio 1, screenWindowCenter (0, 0), screenWindowWidth 1; then the offset table; then the
    chunks as (y, size, data).  Everything is checked and deflated before the file is opened: a bad argument leaves no file.
    -> per chunk 'none' (no compression), 'raw' (did not shrink) or 'deflate'."""
    ptype = pixel_type_code(pixel_type)
    code, _, _ = compression_code(compression)
    row_bytes, lines, sizes = chunk_sizes(width, height, ptype, code)
    check_level(level)
    chunks = list(chunks)
    if len(chunks) != len(sizes):
        raise ValueError('%d x %d with %d scanlines per chunk has %d chunks, got %d' % (width, height, lines, len(sizes), len(chunks)))
    views = []
    for i, (c, n) in enumerate(zip(chunks, sizes)):
        try:
            v = memoryview(c).cast('B')
        except TypeError:
            raise ValueError('chunk %d is not bytes-like: %r' % (i, type(c)))
        if v.nbytes != n:
            raise ValueError('chunk %d (scanlines %d..%d) must hold %d bytes, got %d'
                             % (i, i * lines, min(height, (i + 1) * lines) - 1, n, v.nbytes))
        views.append(v)
    if raw_chunk is not None and not callable(raw_chunk):
        raise ValueError('raw_chunk must be callable(i) -> bytes or None, got %r' % (raw_chunk,))
    if deflated is not None and (code == 0 or len(deflated) != len(views)):
        raise ValueError("deflated: one zlib stream per chunk of a 'zip' / 'zips' file")
    data, how = views, ['none'] * len(views)
    if code != 0:
        streams = deflate_chunks(views, level, workers) if deflated is None else list(deflated)
        data, how = [], []
        for i, (v, z) in enumerate(zip(views, streams)):
            if len(z) < v.nbytes:
                data.append(z)
                how.append('deflate')
                continue
            raw = memoryview(raw_chunk(i) if raw_chunk is not None else unpack_chunk(v.tobytes())).cast('B')
            if raw.nbytes != v.nbytes:
                raise ValueError('raw_chunk(%d) returned %d bytes, the chunk has %d' % (i, raw.nbytes, v.nbytes))
            data.append(raw)
            how.append('raw')
    ctype = struct.pack('<iB3xii', ptype, 0, 1, 1)
    window = struct.pack('<4i', 0, 0, width - 1, height - 1)
    header = MAGIC + struct.pack('<I', 2)
    header += _attribute('channels', 'chlist', b''.join(k + b'\0' + ctype for k in (b'B', b'G', b'R')) + b'\0')
    header += _attribute('compression', 'compression', struct.pack('<B', code))
    header += _attribute('dataWindow', 'box2i', window)
    header += _attribute('displayWindow', 'box2i', window)
    header += _attribute('lineOrder', 'lineOrder', struct.pack('<B', 0))
    header += _attribute('pixelAspectRatio', 'float', struct.pack('<f', 1.0))
    header += _attribute('screenWindowCenter', 'v2f', struct.pack('<2f', 0.0, 0.0))
    header += _attribute('screenWindowWidth', 'float', struct.pack('<f', 1.0))
    header += b'\0'
    offsets, pos = [], len(header) + 8 * len(data)
    for d in data:
        offsets.append(pos)
        pos += 8 + len(d)
    with open(fp, 'wb') as fh:
        fh.write(header)
        fh.write(struct.pack('<%dQ' % len(offsets), *offsets))
        for i, d in enumerate(data):
            fh.write(struct.pack('<ii', i * lines, len(d)))
            fh.write(d)
    return how
