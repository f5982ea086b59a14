"""Shared pieces of the dataset builder's tests: a tiny greyscale PNG encoder (every row filter, 1/8/16-bit) and the exact
registration oracle (fp64 FFTs of 8-bit halves, rounded to integers)."""
import struct
import zlib

import numpy as np


def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else (b if pb <= pc else c)


def encode_png(img, depth, filters=(0,)):
    """2-D array -> greyscale PNG bytes; row i uses filter filters[i % len(filters)] (0 None, 1 Sub, 2 Up, 3 Average, 4 Paeth)."""
    a = np.asarray(img)
    h, w = a.shape
    if depth == 16:
        rows = a.astype(">u2").view(np.uint8).reshape(h, 2 * w)
    elif depth == 8:
        rows = a.astype(np.uint8)
    else:
        rows = np.packbits(a.astype(bool), axis=1)
    bpp = max(1, depth // 8)
    out, prev = [], np.zeros(rows.shape[1], np.int64)
    for i in range(h):
        cur, ft = rows[i].astype(np.int64), filters[i % len(filters)]
        f = np.empty_like(cur)
        for x in range(len(cur)):
            a_ = cur[x - bpp] if x >= bpp else 0
            c_ = prev[x - bpp] if x >= bpp else 0
            pred = [0, a_, prev[x], (a_ + prev[x]) >> 1, _paeth(a_, prev[x], c_)][ft]
            f[x] = (cur[x] - pred) & 0xFF
        out.append(bytes([ft]) + f.astype(np.uint8).tobytes())
        prev = cur
    return (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, 0, 0, 0, 0))
            + _chunk(b"IDAT", zlib.compress(b"".join(out))) + _chunk(b"IEND", b""))


def exact_xcorr(ref, img):
    """cc[s] = sum_p ref[p] * img[p - s] (circular) as int64, exact for uint16: each 8-bit-half correlation is below 2^30 and the
    fp64 FFT's error far below 0.5, so rint recovers it."""
    r, g = np.asarray(ref, np.int64), np.asarray(img, np.int64)
    parts = lambda a: (a >> 8, a & 255)
    F = lambda a: np.fft.fft2(a.astype(np.float64))
    out = np.zeros(r.shape, np.int64)
    for i, rp in enumerate(parts(r)):
        for j, gp in enumerate(parts(g)):
            c = np.rint(np.fft.ifft2(F(rp) * np.conj(F(gp))).real).astype(np.int64)
            out += c << (8 * ((1 - i) + (1 - j)))
    return out


def exact_shift(ref, img):
    """skimage register_translation(ref, img) on the exact surface: argmax, first index in C order, indices > 64 wrapped."""
    cc = exact_xcorr(ref, img)
    y, x = np.unravel_index(int(np.argmax(cc)), cc.shape)
    n = cc.shape[0]
    return (y - n if y > n // 2 else y, x - n if x > n // 2 else x), (y, x)
