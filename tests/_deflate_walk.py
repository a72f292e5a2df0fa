"""A small pure-Python walker of deflate blocks (RFC 1951) for the PNG encoder's tests, independent of the code under test: blocks() reads a
zlib stream block by block and reports each block's BFINAL and BTYPE, the code lengths a dynamic block declares, whether each of its
codes is complete (Kraft sum exactly 1), and how many bytes the block inflates to."""
from fractions import Fraction

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 30


class Bits:
    def __init__(self, data):
        self.data, self.at = data, 0

    def take(self, n):
        v = 0
        for i in range(n):
            v |= ((self.data[self.at >> 3] >> (self.at & 7)) & 1) << i
            self.at += 1
        return v


def kraft(lens):
    return sum((Fraction(1, 1 << n) for n in lens if n), Fraction(0))


def canonical(lens):
    """{(length, code): symbol} of the canonical code of RFC 1951 3.2.2."""
    count = [0] * 17
    for n in lens:
        count[n] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    table = {}
    for s, n in enumerate(lens):
        if n:
            table[(n, nxt[n])] = s
            nxt[n] += 1
    return table


def symbol(bits, table):
    code = 0
    for n in range(1, 16):
        code = (code << 1) | bits.take(1)           # Huffman codes go out most significant bit first
        if (n, code) in table:
            return table[(n, code)]
    raise AssertionError("no code of up to 15 bits matches")


def blocks(zstream):
    """zlib stream -> [dict(final, btype, bytes, ll, d, cl, complete, long_tokens)]: ll / d / cl the declared code lengths of a dynamic
    block (else None), complete = (ll, d, cl) whether each code's Kraft sum is exactly 1, long_tokens = [(bit offset from the block's
    first bit, bits)] of every length + distance token of more than 33 bits."""
    bits = Bits(zstream[2:-4])
    out = []
    while True:
        first = bits.at
        final, btype = bits.take(1), bits.take(2)
        b = dict(final=bool(final), btype=btype, bytes=0, ll=None, d=None, cl=None, complete=None, long_tokens=[])
        assert btype != 3, "reserved block type"
        if btype == 0:
            bits.at = (bits.at + 7) & ~7
            n, inv = bits.take(16), bits.take(16)
            assert n ^ inv == 0xFFFF
            bits.at += 8 * n
            b["bytes"] = n
        else:
            if btype == 1:
                ll, d = FIXED_LL, FIXED_D
            else:
                hlit, hdist, hclen = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
                assert hlit <= 286 and hdist <= 30
                cl = [0] * 19
                for k in range(hclen):
                    cl[CL_ORDER[k]] = bits.take(3)
                table, lens = canonical(cl), []
                while len(lens) < hlit + hdist:
                    s = symbol(bits, table)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        assert lens, "repeat without a previous length"
                        lens += [lens[-1]] * (3 + bits.take(2))
                    else:
                        lens += [0] * (3 + bits.take(3) if s == 17 else 11 + bits.take(7))
                assert len(lens) == hlit + hdist, "a run crosses the end of the lengths"
                ll, d = lens[:hlit], lens[hlit:]
                assert ll[256], "no end-of-block code"
                b.update(ll=ll, d=d, cl=cl, complete=(kraft(ll) == 1, kraft(d) == 1, kraft(cl) == 1))
            tl, td = canonical(ll), canonical(d)
            while True:
                at = bits.at
                s = symbol(bits, tl)
                if s < 256:
                    b["bytes"] += 1
                elif s == 256:
                    break
                else:
                    assert s <= 285
                    b["bytes"] += LEN_BASE[s - 257] + bits.take(LEN_EXTRA[s - 257])
                    ds = symbol(bits, td)
                    assert ds < 30
                    bits.take(DIST_EXTRA[ds])
                    if bits.at - at > 33:
                        b["long_tokens"].append((at - first, bits.at - at))
        out.append(b)
        if final:
            break
    assert (bits.at + 7) >> 3 == len(bits.data), "bytes behind the final block"
    return out
