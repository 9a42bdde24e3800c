"""A restatement of the OpenEXR scanline file layout for the tests: a writer and a numpy decoder (numpy + struct + zlib).  It shares
no code with rnr_amd/exr.py; both restate the OpenEXR file-layout document.

    write(fp, channels, ...)   arbitrary channel sets and types, NONE / ZIPS / ZIP, both line orders, a data window with a
                               non-zero minimum; can force chunks to be stored raw; returns, per chunk, how it was stored
    decode(fp)                 -> ({name: array [H,W]}, info)
    raw_scanlines(fp)          -> the raw scanline buffer as uint8 [H * row_bytes] (what rnr_exr_unpack must produce)
"""
import struct
import zlib

import numpy as np

NONE, ZIPS, ZIP = 0, 2, 3
LINES = {NONE: 1, ZIPS: 1, ZIP: 16}
DTYPES = {0: np.dtype('<u4'), 1: np.dtype('<f2'), 2: np.dtype('<f4')}
CODES = {np.dtype('uint32'): 0, np.dtype('float16'): 1, np.dtype('float32'): 2}


def encode_chunk(raw):
    """raw scanline bytes -> the bytes handed to deflate: de-interleave (even bytes, then odd bytes), then differences + 128."""
    raw = np.frombuffer(bytes(raw), np.uint8)
    split = np.concatenate([raw[0::2], raw[1::2]])
    coded = split.copy()
    coded[1:] = (split[1:].astype(np.int32) - split[:-1].astype(np.int32) + 128 + 256) % 256
    return split.tobytes(), coded.tobytes()


def decode_chunk(coded):
    """The inverse: a running sum mod 256, then the two halves interleaved."""
    t = np.frombuffer(bytes(coded), np.uint8).astype(np.int64)
    d = t - 128
    d[0] = t[0]
    s = (np.cumsum(d) % 256).astype(np.uint8)
    half = (len(s) + 1) // 2
    raw = np.empty(len(s), np.uint8)
    raw[0::2] = s[:half]
    raw[1::2] = s[half:]
    return raw.tobytes()


def _attr(name, kind, value):
    return name.encode() + b'\0' + kind.encode() + b'\0' + struct.pack('<i', len(value)) + value


def write(fp, channels, compression=ZIP, decreasing=False, origin=(0, 0), force_raw=(), flags=0, sampling=None, extra_attrs=(),
          level=6):
    """channels: {name: array [H,W] of float16 / float32 / uint32}.  origin = (x_min, y_min) of the data window.  force_raw: chunk
    indices (in increasing y) stored raw although deflate would shrink them.  sampling: {name: (xs, ys)} written into the channel
    list only (for the refusal tests).  -> ['none' | 'raw' | 'deflate' per chunk, in increasing y]."""
    names = sorted(channels)
    h, w = channels[names[0]].shape
    assert all(channels[n].shape == (h, w) for n in names)
    x0, y0 = origin
    chlist = b''
    for n in names:
        xs, ys = (sampling or {}).get(n, (1, 1))
        chlist += n.encode() + b'\0' + struct.pack('<iB3xii', CODES[channels[n].dtype], 0, xs, ys)
    chlist += b'\0'
    header = struct.pack('<4sI', b'\x76\x2f\x31\x01', 2 | flags)
    header += _attr('channels', 'chlist', chlist)
    header += _attr('compression', 'compression', struct.pack('<B', compression))
    header += _attr('dataWindow', 'box2i', struct.pack('<4i', x0, y0, x0 + w - 1, y0 + h - 1))
    header += _attr('displayWindow', 'box2i', struct.pack('<4i', 0, 0, x0 + w - 1, y0 + h - 1))
    header += _attr('lineOrder', 'lineOrder', struct.pack('<B', 1 if decreasing else 0))
    header += _attr('pixelAspectRatio', 'float', struct.pack('<f', 1.0))
    header += _attr('screenWindowCenter', 'v2f', struct.pack('<2f', 0.0, 0.0))
    header += _attr('screenWindowWidth', 'float', struct.pack('<f', 1.0))
    for a in extra_attrs:
        header += _attr(*a)
    header += b'\0'
    lines = LINES[compression]
    blocks, how = [], []
    for i, top in enumerate(range(0, h, lines)):
        raw = b''.join(channels[n][y].astype(DTYPES[CODES[channels[n].dtype]]).tobytes()
                       for y in range(top, min(top + lines, h)) for n in names)
        if compression == NONE:
            data, kind = raw, 'none'
        else:
            data = zlib.compress(encode_chunk(raw)[1], level)
            kind = 'deflate'
            if len(data) >= len(raw) or i in force_raw:
                data, kind = raw, 'raw'
        blocks.append(struct.pack('<ii', y0 + top, len(data)) + data)
        how.append(kind)
    order = list(range(len(blocks)))[::-1] if decreasing else list(range(len(blocks)))
    pos = len(header) + 8 * len(blocks)
    offsets = [0] * len(blocks)
    body = b''
    for i in order:                     # the offset table is in increasing y; the chunks lie in the file in line order
        offsets[i] = pos + len(body)
        body += blocks[i]
    with open(fp, 'wb') as f:
        f.write(header + struct.pack('<%dQ' % len(blocks), *offsets) + body)
    return how


def _cstr(data, pos):
    end = data.index(b'\0', pos)
    return data[pos:end].decode(), end + 1


def raw_scanlines(fp):
    """-> (uint8 [H * row_bytes], info dict(width, height, origin, channels [(name, type code)], row_bytes, stored [per chunk in
    file-table order: 'none' | 'raw' | 'deflate']))."""
    with open(fp, 'rb') as f:
        data = f.read()
    assert data[:4] == b'\x76\x2f\x31\x01' and data[4] == 2
    pos, attrs = 8, {}
    while data[pos] != 0:
        name, pos = _cstr(data, pos)
        _, pos = _cstr(data, pos)
        size = struct.unpack_from('<i', data, pos)[0]
        attrs[name] = data[pos + 4:pos + 4 + size]
        pos += 4 + size
    pos += 1
    chans, p = [], 0
    while attrs['channels'][p] != 0:
        name, p = _cstr(attrs['channels'], p)
        chans.append((name, struct.unpack_from('<i', attrs['channels'], p)[0]))
        p += 16
    x0, y0, x1, y1 = struct.unpack('<4i', attrs['dataWindow'])
    w, h = x1 - x0 + 1, y1 - y0 + 1
    compression = attrs['compression'][0]
    lines = LINES[compression]
    row_bytes = w * sum(DTYPES[t].itemsize for _, t in chans)
    n = (h + lines - 1) // lines
    out = np.zeros(h * row_bytes, np.uint8)
    stored = []
    for off in struct.unpack_from('<%dQ' % n, data, pos):
        y, size = struct.unpack_from('<ii', data, off)
        chunk = data[off + 8:off + 8 + size]
        want = min(lines, y1 - y + 1) * row_bytes
        if compression == NONE:
            stored.append('none')
        elif size == want:
            stored.append('raw')
        else:
            chunk = decode_chunk(zlib.decompress(chunk))
            stored.append('deflate')
        assert len(chunk) == want
        out[(y - y0) * row_bytes:(y - y0) * row_bytes + want] = np.frombuffer(chunk, np.uint8)
    return out, dict(width=w, height=h, origin=(x0, y0), channels=chans, row_bytes=row_bytes, stored=stored)


def decode(fp):
    """-> ({channel name: array [H,W] in its own type}, info)."""
    raw, info = raw_scanlines(fp)
    rows = raw.reshape(info['height'], info['row_bytes'])
    out, off = {}, 0
    for name, t in info['channels']:
        nbytes = info['width'] * DTYPES[t].itemsize
        out[name] = np.ascontiguousarray(rows[:, off:off + nbytes]).view(DTYPES[t]).reshape(info['height'], info['width'])
        off += nbytes
    return out, info


def rgb(fp):
    """-> float32 [H,W,3] RGB, each channel converted from its own type as numpy converts it."""
    chans, _ = decode(fp)
    return np.stack([chans[k].astype(np.float32) for k in 'RGB'], -1)
