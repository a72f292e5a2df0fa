"""The files of the PNG decoder's tests (tests/test_png_dec_host.py, tests/test_gpu_png_dec.py), written by hand at test time: given
samples, a given filter byte per row (the residuals computed with NumPy: the predictors are those tests/_png_reader.py restates),
zlib.compress at a chosen level, the stream split over chosen IDAT chunks, optional PLTE, tRNS and ancillary chunks.  Pillow decodes
the same bytes as the independent reference; expected_rgb() is the contract of include/tokenhmr_hip.h computed from the samples.
Also a small deflate bit writer for the streams zlib never writes (a distance of 32768, malformed codes)."""
import io
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
KINDS = [(0, 8), (2, 8), (3, 8), (4, 8), (6, 8), (0, 16), (2, 16), (4, 16), (6, 16)]          # every supported (colour type, bit depth)
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}


def bpp_of(ctype, depth):
    return CHANNELS[ctype] * depth // 8


def chunk(kind, body, crc=None):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) if crc is None else crc)


def ihdr(w, h, depth, ctype, compression=0, filt=0, interlace=0):
    return chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, compression, filt, interlace))


def residuals(raw, filters, bpp):
    """raw (H, row bytes) uint8 unfiltered bytes, filters (H,) -> the filtered stream as (H, 1 + row bytes) uint8."""
    x = raw.astype(np.int64)
    h, n = x.shape
    b = np.vstack([np.zeros((1, n), np.int64), x[:-1]])
    a = np.hstack([np.zeros((h, bpp), np.int64), x[:, :-bpp]]) if n > bpp else np.zeros((h, n), np.int64)
    c = np.hstack([np.zeros((h, bpp), np.int64), b[:, :-bpp]]) if n > bpp else np.zeros((h, n), np.int64)
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    preds = [np.zeros_like(x), a, b, (a + b) >> 1, paeth]
    out = np.empty((h, 1 + n), np.uint8)
    for y in range(h):
        out[y, 0] = filters[y]
        out[y, 1:] = (x[y] - preds[int(filters[y])][y]) & 255
    return out


def split(data, pieces):
    """data cut into IDAT bodies: pieces an int (that many near-equal parts) or a list of byte counts (the rest goes last)."""
    if isinstance(pieces, int):
        cuts = [len(data) * k // pieces for k in range(pieces + 1)]
        return [data[cuts[k]:cuts[k + 1]] for k in range(pieces)]
    out, at = [], 0
    for n in pieces:
        out.append(data[at:at + n])
        at += n
    return out + [data[at:]]


def write_png(raw, filters, ctype, depth, level=6, idat=1, plte=None, trns=None, ancillary=False, zstream=None, interlace=0):
    """raw (H, W * bpp) uint8 -> the file.  plte: (n, 3) uint8; trns: bytes; ancillary: gAMA, sRGB, pHYs and tEXt before IDAT and a
    tEXt behind it; zstream: these bytes instead of the compressed residuals."""
    raw = np.asarray(raw, np.uint8)
    h, w = raw.shape[0], raw.shape[1] // bpp_of(ctype, depth)
    z = zlib.compress(residuals(raw, filters, bpp_of(ctype, depth)).tobytes(), level) if zstream is None else zstream
    out = [SIGNATURE, ihdr(w, h, depth, ctype, interlace=interlace)]
    if ancillary:
        out += [chunk(b"gAMA", struct.pack(">I", 45455)), chunk(b"sRGB", b"\x00"), chunk(b"pHYs", struct.pack(">IIB", 2835, 2835, 1)),
                chunk(b"tEXt", b"Comment\x00by hand")]
    if plte is not None:
        out.append(chunk(b"PLTE", np.asarray(plte, np.uint8).tobytes()))
    if trns is not None:
        out.append(chunk(b"tRNS", bytes(trns)))
    out += [chunk(b"IDAT", part) for part in split(z, idat)]
    if ancillary:
        out.append(chunk(b"tEXt", b"Software\x00tests"))
    return b"".join(out + [chunk(b"IEND", b"")])


def write_interlaced(rgb):
    """(H, W, 3) uint8 R, G, B -> an Adam7-interlaced 8-bit RGB file (every pass row with filter None), for the fallback tests."""
    rgb = np.asarray(rgb, np.uint8)
    h, w = rgb.shape[:2]
    stream = b""
    for xs, ys, dx, dy in ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2)):
        sub = rgb[ys::dy, xs::dx]
        if sub.size:
            stream += b"".join(b"\x00" + row.tobytes() for row in sub)
    return b"".join([SIGNATURE, ihdr(w, h, 8, 2, interlace=1), chunk(b"IDAT", zlib.compress(stream)), chunk(b"IEND", b"")])


def expected_rgb(raw, ctype, depth, plte=None):
    """The contract: (H, W, 3) uint8 R, G, B from the unfiltered bytes."""
    raw = np.asarray(raw, np.uint8)
    s, ch = depth // 8, CHANNELS[ctype]
    px = raw.reshape(raw.shape[0], -1, ch, s)[:, :, :, 0]          # the high byte of every sample
    if ctype == 3:
        return np.asarray(plte, np.uint8)[px[:, :, 0]]
    if ctype in (0, 4):
        return np.repeat(px[:, :, :1], 3, axis=2)
    return px[:, :, :3].copy()


def pillow_rgb(data, ctype, depth):
    """Pillow's decode of the file as the contract holds it to Pillow; None for 16-bit grey + alpha, where the contract stands alone."""
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        if depth == 8:
            return np.asarray(im.convert("RGB"))
        if ctype in (2, 6):
            return np.asarray(im)[:, :, :3].copy()
        if ctype == 0:
            a = np.asarray(im)
            return np.repeat((a >> 8).astype(np.uint8)[:, :, None], 3, axis=2)
    return None


def samples(h, w, ctype, depth, seed, smooth=False):
    """(H, W * bpp) uint8: noise, or (smooth) a gradient with a little noise, which gives every filter something to do."""
    rng = np.random.default_rng(seed)
    n = w * bpp_of(ctype, depth)
    if not smooth:
        return rng.integers(0, 256, (h, n), dtype=np.uint8)
    y, x = np.mgrid[0:h, 0:n]
    return ((3 * y + 2 * (x // bpp_of(ctype, depth)) + 40 * (x % bpp_of(ctype, depth)) + rng.integers(0, 3, (h, n))) & 255).astype(np.uint8)


def palette(n, seed=5):
    return np.random.default_rng(seed).integers(0, 256, (n, 3), dtype=np.uint8)


def all_pairs():
    """26 filter bytes in which every ordered pair of filters follows one another: a de Bruijn sequence B(5, 2), closed."""
    k, n = 5, 2
    a, seq = [0] * (k * n), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)

    db(1, 1)
    return np.array(seq + seq[:1], np.uint8)


def case(h, w, ctype, depth, filters, seed=0, smooth=True, **kw):
    """(file bytes, expected (H, W, 3) RGB, raw) of one hand-written file; filters: an int (every row) or a sequence cycled over rows."""
    raw = samples(h, w, ctype, depth, seed, smooth)
    f = np.resize(np.atleast_1d(np.asarray(filters, np.uint8)), h)
    plte = None
    if ctype == 3:
        plte = kw.pop("plte", None)
        plte = palette(256) if plte is None else plte
        raw = (raw.astype(np.int64) % len(plte)).astype(np.uint8)
    return write_png(raw, f, ctype, depth, plte=plte, **kw), expected_rgb(raw, ctype, depth, plte), raw


# ---- deflate by hand ----
class Bits:
    """A deflate bit writer: bits() appends a value least significant bit first, code() a Huffman code most significant bit first."""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, v, n):
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, v, n):
        self.bits(int(format(v, f"0{n}b")[::-1], 2), n)

    def done(self):
        if self.n:
            self.bits(0, 8 - self.n)
        return bytes(self.out)


_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
              16385, 24577]
_DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


def _fixed_symbol(w, s):
    if s < 144:
        w.code(0x30 + s, 8)
    elif s < 256:
        w.code(0x190 + s - 144, 9)
    elif s < 280:
        w.code(s - 256, 7)
    else:
        w.code(0xC0 + s - 280, 8)


def fixed_block(w, tokens, last=True):
    """One fixed-Huffman block: tokens are literals (int) or (length, distance) pairs."""
    w.bits(1 if last else 0, 1)
    w.bits(1, 2)
    for t in tokens:
        if isinstance(t, tuple):
            length, dist = t
            k = max(i for i in range(29) if _LEN_BASE[i] <= length)
            _fixed_symbol(w, 257 + k)
            w.bits(length - _LEN_BASE[k], _LEN_EXTRA[k])
            k = max(i for i in range(30) if _DIST_BASE[i] <= dist)
            w.code(k, 5)
            w.bits(dist - _DIST_BASE[k], _DIST_EXTRA[k])
        else:
            _fixed_symbol(w, t)
    _fixed_symbol(w, 256)


def zwrap(deflate, plain=None, header=b"\x78\x9c"):
    """header + deflate + the Adler-32 of `plain` (zero when not given: for streams that must fail before it is read)."""
    return header + deflate + struct.pack(">I", zlib.adler32(plain) if plain is not None else 0)


def dynamic_header(w, cl_lens, lengths, hlit, hdist, last=True):
    """A dynamic block's header: cl_lens {code-length symbol: length}, `lengths` the hlit + hdist code lengths, each sent as itself
    with the canonical code-length code (no repeats)."""
    order = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
    hclen = max(k + 1 for k in range(19) if cl_lens.get(order[k], 0)) if any(cl_lens.values()) else 4
    hclen = max(hclen, 4)
    w.bits(1 if last else 0, 1)
    w.bits(2, 2)
    w.bits(hlit - 257, 5)
    w.bits(hdist - 1, 5)
    w.bits(hclen - 4, 4)
    for k in range(hclen):
        w.bits(cl_lens.get(order[k], 0), 3)
    codes, code = {}, 0
    for n in range(1, 8):
        for s in sorted(cl_lens):
            if cl_lens[s] == n:
                codes[s] = (code, n)
                code += 1
        code <<= 1
    for v in lengths:
        w.code(*codes[v])


def single_distance_code_stream():
    """A dynamic block whose distance code is ONE code of one bit (incomplete, and legal): 'a', then a match of 3 at distance 1."""
    w = Bits()
    lengths = [0] * 258 + [1]
    lengths[97], lengths[256], lengths[257] = 1, 2, 2
    dynamic_header(w, {0: 1, 1: 2, 2: 2}, lengths, 258, 1)
    w.code(0, 1)            # 'a'
    w.code(3, 2)            # 257: length 3
    w.code(0, 1)            # distance 1
    w.code(2, 2)            # end of block
    return zwrap(w.done(), b"aaaa"), b"aaaa"
