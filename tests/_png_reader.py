"""A small PNG reader for the encoder's tests, independent of the code under test: zlib.decompress + a NumPy unfilter.  read() checks the
signature, the chunk order (IHDR, one IDAT, IEND), every chunk CRC against zlib.crc32, the IHDR fields and the inflated length, and
returns the pixels together with the filter byte of every row.  expected_filters() restates libpng's default heuristic in NumPy."""
import struct
import zlib

import numpy as np

COLOUR_TYPE = {1: 0, 3: 2, 4: 6}


def read(data):
    """bytes -> (pixels (H, W, C) uint8, filters (H,) uint8, filtered stream bytes)."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n", "signature"
    at, chunks = 8, []
    while at < len(data):
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        assert struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + body), f"CRC of {kind}"
        chunks.append((kind, body))
        at += 12 + n
    assert at == len(data) and [k for k, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"], [k for k, _ in chunks]
    w, h, depth, ctype, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, comp, filt, lace) == (8, 0, 0, 0) and ctype in COLOUR_TYPE.values() and len(chunks[2][1]) == 0
    c = {v: k for k, v in COLOUR_TYPE.items()}[ctype]
    assert chunks[1][1][:2] == b"\x78\x01", "zlib header"
    stream = zlib.decompress(chunks[1][1])
    assert len(stream) == h * (1 + w * c), "inflated length"
    rows = np.frombuffer(stream, np.uint8).reshape(h, 1 + w * c)
    filters, res = rows[:, 0].copy(), rows[:, 1:].astype(np.int64)
    assert filters.max() <= 4
    out = np.zeros((h, w * c), np.int64)
    prev = np.zeros(w * c, np.int64)
    for y in range(h):
        f, r, cur = filters[y], res[y], out[y]
        if f == 0:
            cur[:] = r
        elif f == 2:
            cur[:] = (r + prev) & 255
        else:                                   # the filters that look left go pixel by pixel (all c bytes of a pixel at once)
            for x in range(0, w * c, c):
                a = cur[x - c:x] if x else np.zeros(c, np.int64)
                b = prev[x:x + c]
                cc = prev[x - c:x] if x else np.zeros(c, np.int64)
                if f == 1:
                    pred = a
                elif f == 3:
                    pred = (a + b) >> 1
                else:
                    p = a + b - cc
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - cc)
                    pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, cc))
                cur[x:x + c] = (r[x:x + c] + pred) & 255
        prev = cur
    return out.astype(np.uint8).reshape(h, w, c), filters, stream


def filter_costs(pixels):
    """(H, 5) sums of |residual as a signed byte| of every filter on every row of (H, W, C) uint8 pixels."""
    h, w, c = pixels.shape
    x = pixels.reshape(h, w * c).astype(np.int64)
    b = np.vstack([np.zeros((1, w * c), np.int64), x[:-1]])
    a = np.hstack([np.zeros((h, c), np.int64), x[:, :-c]])
    cc = np.hstack([np.zeros((h, c), np.int64), b[:, :-c]])
    p = a + b - cc
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - cc)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, cc))
    costs = []
    for pred in (0, a, b, (a + b) >> 1, paeth):
        r = (x - pred) & 255
        costs.append(np.where(r < 128, r, 256 - r).sum(axis=1))
    return np.stack(costs, axis=1)


def expected_filters(pixels):
    """The smallest cost, ties to the lowest filter number (np.argmin returns the first minimum)."""
    return np.argmin(filter_costs(pixels), axis=1).astype(np.uint8)
