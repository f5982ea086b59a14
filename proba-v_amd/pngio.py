"""Minimal greyscale PNG I/O (scikit-image is not a dependency here).

imsave_uint16: the reference saves predictions with skimage.io.imsave as uint16 (test.py:96-100).
imread: the ESA PROBA-V frames and masks (LR / HR 16-bit, QM / SM 1-bit or 8-bit greyscale) as the dataset builder reads them
(utils/dataGenerator.py:905-938): bool for 1-bit, uint8 for 8-bit, uint16 for 16-bit.  PIL when it imports, else the pure reader
below (all five row filters, non-interlaced)."""
import struct
import zlib

import numpy as np


def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def imsave_uint16(path, img):
    a = np.ascontiguousarray(np.asarray(img).astype(np.uint16))
    if a.ndim != 2:
        raise ValueError("expected a 2-D image, got shape %r" % (a.shape,))
    h, w = a.shape
    rows = a.astype(">u2").tobytes()
    stride = 2 * w
    raw = b"".join(b"\x00" + rows[i * stride:(i + 1) * stride] for i in range(h))      # filter type 0 per scanline
    png = b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 16, 0, 0, 0, 0)) \
        + _chunk(b"IDAT", zlib.compress(raw, 6)) + _chunk(b"IEND", b"")
    with open(path, "wb") as fh:
        fh.write(png)


def imread_uint16(path):
    """Inverse of imsave_uint16 (filter 0, greyscale 16-bit only) -- used by the tests."""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, w, h = 8, b"", 0, 0
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        if tag == b"IHDR":
            w, h, depth, ctype = struct.unpack(">IIBB", body[:10])
            assert depth == 16 and ctype == 0
        elif tag == b"IDAT":
            idat += body
        pos += 12 + n
    raw = zlib.decompress(idat)
    out = np.empty((h, w), np.uint16)
    for i in range(h):
        line = raw[i * (2 * w + 1):(i + 1) * (2 * w + 1)]
        assert line[0] == 0
        out[i] = np.frombuffer(line[1:], dtype=">u2")
    return out


def _unfilter(raw, h, stride, bpp):
    """Undo the per-row filters (PNG spec 9.2: None, Sub, Up, Average, Paeth) -> [h][stride] uint8."""
    out = np.zeros((h, stride), np.uint8)
    prev = np.zeros(stride, np.int32)
    for i in range(h):
        line = raw[i * (stride + 1):(i + 1) * (stride + 1)]
        ft = line[0]
        cur = np.frombuffer(line[1:], np.uint8).astype(np.int32)
        if ft == 0:
            rec = cur
        elif ft == 2:
            rec = (cur + prev) & 0xFF
        elif ft == 1:                                      # Sub: a running sum along each of the bpp byte lanes
            rec = (np.cumsum(cur.reshape(-1, bpp), axis=0) & 0xFF).reshape(-1)
        elif ft in (3, 4):                                 # Average / Paeth depend on the reconstructed left byte: one byte at a time
            rec = cur.copy()
            for x in range(stride):
                a = int(rec[x - bpp]) if x >= bpp else 0
                if ft == 1:
                    pred = a
                elif ft == 3:
                    pred = (a + int(prev[x])) >> 1
                else:
                    b, c = int(prev[x]), int(prev[x - bpp]) if x >= bpp else 0
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
                rec[x] = (rec[x] + pred) & 0xFF
        else:
            raise ValueError("bad PNG filter type %d" % ft)
        out[i] = rec
        prev = rec
    return out


def _imread_pure(path):
    data = open(path, "rb").read()
    if data[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError("%s: not a PNG file" % path)
    pos, idat, w, h, depth = 8, b"", 0, 0, 0
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        if tag == b"IHDR":
            w, h, depth, ctype, _, _, interlace = struct.unpack(">IIBBBBB", body[:13])
            if ctype != 0 or depth not in (1, 8, 16) or interlace:
                raise ValueError("%s: only non-interlaced 1-, 8- and 16-bit greyscale PNGs are read (type %d, depth %d)" % (path, ctype, depth))
        elif tag == b"IDAT":
            idat += body
        elif tag == b"IEND":
            break
        pos += 12 + n
    stride = (w * depth + 7) // 8
    rows = _unfilter(zlib.decompress(idat), h, stride, max(1, depth // 8))
    if depth == 16:
        return rows.view(">u2").astype(np.uint16).reshape(h, w)
    if depth == 8:
        return rows
    return np.unpackbits(rows, axis=1)[:, :w].astype(bool)


def imread(path):
    """Greyscale PNG -> 2-D array: bool (1-bit), uint8 (8-bit) or uint16 (16-bit)."""
    try:
        from PIL import Image
    except ImportError:
        return _imread_pure(path)
    with Image.open(path) as im:
        a = np.array(im)
    if a.ndim != 2:
        raise ValueError("%s: greyscale PNG expected, got shape %r" % (path, a.shape))
    if a.dtype not in (np.bool_, np.uint8):
        a = a.astype(np.uint16)
    return a
