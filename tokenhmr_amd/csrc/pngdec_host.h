// The host half of the PNG decoder (include/tokenhmr_hip.h): the chunk walk, an inflate written here (the library links no zlib), the
// rows a window needs kept as they come out of the inflate, and the whole decode on the CPU with the arithmetic of pngdec_math.h — the
// oracle of the kernels, and what a caller without a device gets.  Host only, no HIP call; it can be included from a stand-alone CPU
// program (scripts/pngdec_sanitize.cpp).
//
// The format contract stands in include/tokenhmr_hip.h.  What this file guarantees on top of it: every read of the input is bounds
// checked (the chunk walk never trusts a length, the bit reader never leaves an IDAT's data), every Huffman symbol costs at most
// 15 + 13 bits and every loop advances either the input or the output, so a malformed file ends in THMR_ERR_INVALID.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <new>
#include <string>
#include <vector>

#include "png_host.h"
#include "pngdec_math.h"

namespace pngdh {

// The plan words of include/tokenhmr_hip.h (THMR_PNG_PLAN_*) as this file and pngdec.hip name them: the same 206 words.
struct Plan {
    int32_t height, width, bit_depth, colour_type, bpp;
    int32_t win_x0, win_y0, win_w, win_h;
    int32_t row0, rows_kept, kept_row_bytes, rows_inflated;
    int32_t palette_entries;
    uint8_t palette[256][3];
};
static_assert(sizeof(Plan) == 4 * THMR_PNG_PLAN_WORDS && offsetof(Plan, palette) == 4 * THMR_PNG_PLAN_PALETTE &&
              offsetof(Plan, bpp) == 4 * THMR_PNG_PLAN_BPP && offsetof(Plan, win_x0) == 4 * THMR_PNG_PLAN_WIN_X0 &&
              offsetof(Plan, win_h) == 4 * THMR_PNG_PLAN_WIN_H && offsetof(Plan, row0) == 4 * THMR_PNG_PLAN_ROW0 &&
              offsetof(Plan, rows_kept) == 4 * THMR_PNG_PLAN_ROWS_KEPT && offsetof(Plan, kept_row_bytes) == 4 * THMR_PNG_PLAN_KEPT_ROW_BYTES &&
              offsetof(Plan, rows_inflated) == 4 * THMR_PNG_PLAN_ROWS_INFLATED && offsetof(Plan, palette_entries) == 4 * THMR_PNG_PLAN_PALETTE_ENTRIES,
              "Plan is the word layout of the header");

// ---- the container ----
struct Segment {            // one IDAT chunk: its data, and the CRC stored behind it (over the type and the data)
    const uint8_t* p;
    size_t n;
    uint32_t crc;
};

struct Header {
    int32_t H = 0, W = 0, depth = 0, ctype = 0, interlace = 0, bpp = 0;
    bool unsupported = false;
    std::string why;
    int32_t palette_entries = 0;
    uint8_t palette[256][3];
    std::vector<Segment> idat;
};

inline uint32_t be32(const uint8_t* p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }

// Signature, IHDR (and, unless ihdr_only, every chunk up to IEND or the end of the data): 0 with h filled, or THMR_ERR_INVALID.  A file
// of a kind the decoder does not handle parses (h.unsupported, h.why); the caller turns that into THMR_ERR_UNSUPPORTED.
inline int parse(const uint8_t* data, size_t len, bool ihdr_only, Header& h, std::string& err) {
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    if (len < 8 || memcmp(data, sig, 8) != 0) { err = "not a PNG: bad signature"; return THMR_ERR_INVALID; }
    memset(h.palette, 0, sizeof(h.palette));
    size_t pos = 8;
    bool first = true, idat_over = false;
    while (pos < len) {
        if (len - pos < 12) { err = "truncated chunk at byte " + std::to_string(pos); return THMR_ERR_INVALID; }
        const uint32_t n = be32(data + pos);
        if (n > 0x7FFFFFFFu || (size_t)n > len - pos - 12) { err = "truncated chunk at byte " + std::to_string(pos); return THMR_ERR_INVALID; }
        const uint8_t* type = data + pos + 4;
        const uint8_t* body = type + 4;
        const uint32_t crc = be32(body + n);
        pos += 12 + (size_t)n;
        if (first) {
            if (memcmp(type, "IHDR", 4) != 0 || n != 13) { err = "the first chunk is not a 13-byte IHDR"; return THMR_ERR_INVALID; }
            if (pngh::crc32(type, 17) != crc) { err = "wrong CRC on IHDR"; return THMR_ERR_INVALID; }
            first = false;
            const uint32_t W = be32(body), H = be32(body + 4);
            h.depth = body[8]; h.ctype = body[9]; h.interlace = body[12];
            if (W == 0 || H == 0 || W > 0x7FFFFFFFu || H > 0x7FFFFFFFu) { err = "IHDR: a side is 0 or above 2^31 - 1"; return THMR_ERR_INVALID; }
            h.W = (int32_t)W; h.H = (int32_t)H;
            const int d = h.depth, t = h.ctype;
            const bool pair_ok = t == 0 ? (d == 1 || d == 2 || d == 4 || d == 8 || d == 16)
                               : t == 3 ? (d == 1 || d == 2 || d == 4 || d == 8)
                               : (t == 2 || t == 4 || t == 6) ? (d == 8 || d == 16) : false;
            if (!pair_ok) { err = "IHDR: colour type " + std::to_string(t) + " with bit depth " + std::to_string(d) + " is no PNG"; return THMR_ERR_INVALID; }
            if (h.interlace > 1) { err = "IHDR: interlace method " + std::to_string(h.interlace) + " is no PNG"; return THMR_ERR_INVALID; }
            if (h.interlace == 1) { h.unsupported = true; h.why = "Adam7 interlace"; }
            else if (d < 8) { h.unsupported = true; h.why = "bit depth " + std::to_string(d); }
            else if (W > 32767 || H > 32767) { h.unsupported = true; h.why = "a side above 32767 (" + std::to_string(W) + " x " + std::to_string(H) + ")"; }
            else if (body[10] != 0) { h.unsupported = true; h.why = "compression method " + std::to_string(body[10]); }
            else if (body[11] != 0) { h.unsupported = true; h.why = "filter method " + std::to_string(body[11]); }
            h.bpp = pngdm::bytes_per_pixel(t, d);
            if (ihdr_only || h.unsupported) return 0;
            continue;
        }
        if (memcmp(type, "IDAT", 4) == 0) {
            if (idat_over) { err = "IDAT chunks are not consecutive"; return THMR_ERR_INVALID; }
            h.idat.push_back(Segment{body, (size_t)n, crc});
            continue;
        }
        if (!h.idat.empty()) idat_over = true;
        if (memcmp(type, "IEND", 4) == 0) break;
        if (memcmp(type, "PLTE", 4) == 0) {
            if (idat_over || h.palette_entries) { err = "PLTE after IDAT, or twice"; return THMR_ERR_INVALID; }
            if (n == 0 || n > 768 || n % 3 != 0) { err = "PLTE of " + std::to_string(n) + " bytes"; return THMR_ERR_INVALID; }
            if (pngh::crc32(type, 4 + (size_t)n) != crc) { err = "wrong CRC on PLTE"; return THMR_ERR_INVALID; }
            h.palette_entries = (int32_t)(n / 3);
            memcpy(h.palette, body, n);
        }
        // every other chunk (tRNS, gAMA, sRGB, iCCP, pHYs, tEXt, acTL, ...) is skipped and has no effect
    }
    if (first) { err = "not a PNG: no IHDR"; return THMR_ERR_INVALID; }
    if (h.idat.empty()) { err = "no IDAT chunk"; return THMR_ERR_INVALID; }
    if (h.ctype == 3 && h.palette_entries == 0) { err = "colour type 3 without PLTE before IDAT"; return THMR_ERR_INVALID; }
    return 0;
}

inline int parse_supported(const uint8_t* data, size_t len, Header& h, std::string& err) {
    const int rc = parse(data, len, false, h, err);
    if (rc) return rc;
    if (h.unsupported) { err = "unsupported PNG: " + h.why; return THMR_ERR_UNSUPPORTED; }
    return 0;
}

// ---- the inflate ----
// The input: the data of the IDAT chunks one after the other, as one bit stream, least significant bit first.  An IDAT's CRC is
// checked when the reader enters it, so only chunks that are read are checked.
struct Input {
    const Segment* seg;
    size_t nseg, next = 0;
    bool check_crc;
    bool bad_crc = false;
    const uint8_t* cur = nullptr;
    const uint8_t* end = nullptr;
    uint64_t bits = 0;
    int nbits = 0;

    Input(const Segment* s, size_t n, bool crc) : seg(s), nseg(n), check_crc(crc) {}

    bool enter() {          // the next segment that has data; false at the end of the input (or at a wrong CRC)
        while (cur == end) {
            if (next >= nseg || bad_crc) return false;
            const Segment& s = seg[next++];
            if (check_crc && pngh::crc32(s.p - 4, s.n + 4) != s.crc) { bad_crc = true; return false; }
            cur = s.p; end = s.p + s.n;
        }
        return true;
    }
    void refill() {         // at least 57 bits where the input has them
        if (end - cur >= 8) {
            uint64_t w;
            memcpy(&w, cur, 8);         // little-endian hosts (the library's only targets)
            bits |= w << nbits;
            cur += (63 - nbits) >> 3;
            nbits |= 56;
            return;
        }
        while (nbits <= 56) {
            if (cur == end && !enter()) return;
            bits |= (uint64_t)*cur++ << nbits;
            nbits += 8;
        }
    }
    bool get(int n, uint32_t& v) {          // n <= 32
        if (nbits < n) { refill(); if (nbits < n) return false; }
        v = (uint32_t)(bits & (((uint64_t)1 << n) - 1));
        bits >>= n; nbits -= n;
        return true;
    }
};

constexpr int FAST_BITS = 10;

// One canonical Huffman code: a first-level table over FAST_BITS bits (length << 9 | symbol, 0 = no code this short), and the counts
// per length with the symbols in code order for the walk over longer codes.
struct Huff {
    uint16_t fast[1 << FAST_BITS];
    uint16_t count[16];
    uint16_t symbol[288];
};

// lens[0 .. n) -> h.  Returns what is left of the code space in units of 2^-15: 0 complete, > 0 incomplete, < 0 over-subscribed.
inline int build(Huff& h, const uint8_t* lens, int n) {
    memset(h.fast, 0, sizeof(h.fast));
    memset(h.count, 0, sizeof(h.count));
    for (int s = 0; s < n; ++s) ++h.count[lens[s]];
    h.count[0] = 0;
    int left = 1;
    for (int l = 1; l <= 15; ++l) {
        left <<= 1;
        left -= h.count[l];
        if (left < 0) return left;
    }
    uint16_t offs[16], code[16];
    offs[1] = 0; code[1] = 0;
    for (int l = 1; l < 15; ++l) {
        offs[l + 1] = (uint16_t)(offs[l] + h.count[l]);
        code[l + 1] = (uint16_t)((code[l] + h.count[l]) << 1);
    }
    for (int s = 0; s < n; ++s) {
        const int l = lens[s];
        if (!l) continue;
        h.symbol[offs[l]++] = (uint16_t)s;
        const uint32_t c = code[l]++;
        if (l <= FAST_BITS) {
            const uint32_t r = pngm::reverse_bits(c, l);
            for (uint32_t k = r; k < (1u << FAST_BITS); k += 1u << l) h.fast[k] = (uint16_t)(l << 9 | s);
        }
    }
    return left;
}

// The next symbol, or -1: the input ended inside the code, or the bits are no code of an incomplete set.
inline int decode(Input& in, const Huff& h) {
    const uint32_t e = h.fast[in.bits & ((1u << FAST_BITS) - 1)];
    if (e) {
        const int l = (int)(e >> 9);
        if (l > in.nbits) return -1;
        in.bits >>= l; in.nbits -= l;
        return (int)(e & 511);
    }
    int code = 0, first = 0, index = 0;
    for (int l = 1; l <= 15; ++l) {
        if (l > in.nbits) return -1;
        code |= (int)((in.bits >> (l - 1)) & 1);
        const int count = h.count[l];
        if (code - count < first) {
            in.bits >>= l; in.nbits -= l;
            return h.symbol[index + (code - first)];
        }
        index += count; first += count;
        first <<= 1; code <<= 1;
    }
    return -1;
}

struct FixedCodes {
    Huff ll, d;
    FixedCodes() {
        uint8_t lens[288];
        for (int s = 0; s < 288; ++s) lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8;
        build(ll, lens, 288);
        for (int s = 0; s < 30; ++s) lens[s] = 5;
        build(d, lens, 30);            // 30 of the 32 five-bit codes: the other two decode as "no code"
    }
};

constexpr int HISTORY = 32768;          // the furthest a distance reaches
constexpr int CHUNK = 32768;            // bytes handed to the sink at a time

inline void adler_update(uint32_t& a, uint32_t& b, const uint8_t* p, size_t n) {
    while (n) {
        size_t k = n < 5552 ? n : 5552;         // the longest run whose sums stay below 2^32
        n -= k;
        while (k--) { a += *p++; b += a; }
        a %= pngm::ADLER_MOD; b %= pngm::ADLER_MOD;
    }
}

// Inflates the zlib stream of `in` into `sink`, in order: sink.put(p, n) returns 0 (go on), 1 (it has all it wants: stop) or a
// negative status with `err` set; sink.want() is the number of bytes after which it will say 1 (INT64_MAX: never), so that the inflate
// hands over exactly then and reads no input beyond what those bytes took.  0 with ended = true: the final block was read to its end and the Adler-32 behind it equals that
// of the bytes put (checked only then).  0 with ended = false: the sink stopped it.
template <typename Sink>
int inflate(Input& in, Sink& sink, bool& ended, std::string& err) {
    static const uint16_t len_base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    static const uint8_t len_extra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    static const uint16_t dist_base[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
    static const uint8_t dist_extra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
    static const FixedCodes fixed;
    ended = false;
    const auto early = [&]() {
        err = in.bad_crc ? "wrong CRC on IDAT" : "the deflate stream ends early";
        return THMR_ERR_INVALID;
    };
    uint32_t v;
    if (!in.get(16, v)) return early();
    const uint32_t cmf = v & 255, flg = v >> 8;
    if ((cmf & 15) != 8 || (cmf >> 4) > 7 || ((cmf << 8) | flg) % 31 != 0 || (flg & 32)) {
        err = "the zlib header is not deflate with a window of 32K or less and no preset dictionary";
        return THMR_ERR_INVALID;
    }
    std::vector<uint8_t> hist;
    try { hist.resize(HISTORY + CHUNK + 258 + 8); } catch (const std::bad_alloc&) { err = "out of host memory for the inflate window"; return THMR_ERR_NOMEM; }
    uint8_t* buf = hist.data();
    size_t pos = 0, flushed = 0;            // buf[flushed, pos) is not yet with the sink
    int64_t before = 0;                     // bytes that have left buf: the output so far is before + pos
    uint32_t ad_a = 1, ad_b = 0;
    size_t stop = 0;                        // flush when pos reaches it
    const auto set_stop = [&]() {
        const int64_t want = sink.want();
        stop = (size_t)(HISTORY + CHUNK);
        if (want < (int64_t)(stop - flushed)) stop = flushed + (size_t)want;
    };
    set_stop();
    const auto flush = [&](bool slide) -> int {
        if (pos > flushed) {
            adler_update(ad_a, ad_b, buf + flushed, pos - flushed);
            const int rc = sink.put(buf + flushed, pos - flushed);
            if (rc) return rc;
            flushed = pos;
        }
        if (slide && pos > (size_t)HISTORY) {
            memmove(buf, buf + pos - HISTORY, HISTORY);
            before += (int64_t)(pos - HISTORY);
            pos = flushed = HISTORY;
        }
        set_stop();
        return 0;
    };
    Huff dyn_ll, dyn_d;
    for (bool last = false; !last;) {
        if (!in.get(3, v)) return early();
        last = v & 1;
        const uint32_t type = v >> 1;
        if (type == 3) { err = "deflate block type 3"; return THMR_ERR_INVALID; }
        if (type == 0) {
            in.bits >>= in.nbits & 7; in.nbits -= in.nbits & 7;
            if (!in.get(32, v)) return early();
            uint32_t n = v & 0xFFFF;
            if ((n ^ 0xFFFF) != (v >> 16)) { err = "a stored block's length check fails"; return THMR_ERR_INVALID; }
            while (n) {
                if (pos >= stop) { if (const int rc = flush(true)) return rc < 0 ? rc : 0; }
                if (in.nbits) {                 // whole bytes still in the bit buffer
                    buf[pos++] = (uint8_t)in.bits; in.bits >>= 8; in.nbits -= 8; --n;
                    continue;
                }
                in.bits = 0;                    // refill() may have left bits of the bytes at cur above nbits: they are copied below
                if (in.cur == in.end && !in.enter()) return early();
                size_t k = (size_t)(in.end - in.cur);
                if (k > n) k = n;
                if (k > stop - pos) k = stop - pos;
                memcpy(buf + pos, in.cur, k);
                in.cur += k; pos += k; n -= (uint32_t)k;
            }
            continue;
        }
        const Huff* ll = &fixed.ll;
        const Huff* dd = &fixed.d;
        if (type == 2) {
            if (!in.get(14, v)) return early();
            const int hlit = (int)(v & 31) + 257, hdist = (int)((v >> 5) & 31) + 1, hclen = (int)(v >> 10) + 4;
            if (hlit > 286 || hdist > 30) { err = "a dynamic block with more than 286 length or 30 distance codes"; return THMR_ERR_INVALID; }
            uint8_t lens[320];
            memset(lens, 0, 19);
            for (int k = 0; k < hclen; ++k) {
                if (!in.get(3, v)) return early();
                lens[pngm::cl_order(k)] = (uint8_t)v;
            }
            Huff& cl = dyn_d;           // built and used before the distance code is
            if (build(cl, lens, 19) != 0) { err = "the code-length code is over-subscribed or incomplete"; return THMR_ERR_INVALID; }
            int i = 0;
            while (i < hlit + hdist) {
                if (in.nbits < 15 + 7) in.refill();
                const int s = decode(in, cl);
                if (s < 0) return in.nbits < 15 ? early() : (err = "invalid code-length code", THMR_ERR_INVALID);
                if (s < 16) { lens[i++] = (uint8_t)s; continue; }
                int rep, val = 0;
                if (s == 16) {
                    if (i == 0) { err = "a length repeat with nothing before it"; return THMR_ERR_INVALID; }
                    val = lens[i - 1];
                    if (!in.get(2, v)) return early();
                    rep = 3 + (int)v;
                } else if (s == 17) {
                    if (!in.get(3, v)) return early();
                    rep = 3 + (int)v;
                } else {
                    if (!in.get(7, v)) return early();
                    rep = 11 + (int)v;
                }
                if (i + rep > hlit + hdist) { err = "a length repeat runs past the last code"; return THMR_ERR_INVALID; }
                while (rep--) lens[i++] = (uint8_t)val;
            }
            if (lens[256] == 0) { err = "a dynamic block without an end-of-block code"; return THMR_ERR_INVALID; }
            uint8_t dl[32];
            memcpy(dl, lens + hlit, (size_t)hdist);
            if (build(dyn_ll, lens, hlit) != 0) { err = "the literal/length code is over-subscribed or incomplete"; return THMR_ERR_INVALID; }
            const int left = build(dyn_d, dl, hdist);
            int used = 0;
            for (int s = 0; s < hdist; ++s) used += dl[s] != 0;
            // as zlib: an incomplete distance code is legal only as a single code of one bit (or none at all, in a block of literals)
            if (left < 0 || (left > 0 && !(used == 0 || (used == 1 && dyn_d.count[1] == 1)))) {
                err = "the distance code is over-subscribed or incomplete";
                return THMR_ERR_INVALID;
            }
            ll = &dyn_ll; dd = &dyn_d;
        }
        for (;;) {
            if (pos >= stop) { if (const int rc = flush(true)) return rc < 0 ? rc : 0; }
            if (in.nbits < 48) in.refill();            // a length and a distance with their extra bits: at most 15 + 5 + 15 + 13
            int s = decode(in, *ll);
            if (s < 0) return in.nbits < 15 ? early() : (err = "invalid literal/length code", THMR_ERR_INVALID);
            if (s < 256) { buf[pos++] = (uint8_t)s; continue; }
            if (s == 256) break;
            s -= 257;
            if (s >= 29) { err = "length symbol " + std::to_string(s + 257); return THMR_ERR_INVALID; }
            if (in.nbits < len_extra[s]) return early();
            const int length = len_base[s] + (int)(in.bits & ((1u << len_extra[s]) - 1));
            in.bits >>= len_extra[s]; in.nbits -= len_extra[s];
            const int ds = decode(in, *dd);
            if (ds < 0) return in.nbits < 15 ? early() : (err = "invalid distance code", THMR_ERR_INVALID);
            if (ds >= 30) { err = "distance symbol " + std::to_string(ds); return THMR_ERR_INVALID; }
            if (in.nbits < dist_extra[ds]) return early();
            const size_t dist = dist_base[ds] + (size_t)(in.bits & ((1u << dist_extra[ds]) - 1));
            in.bits >>= dist_extra[ds]; in.nbits -= dist_extra[ds];
            if (dist > pos) { err = "a distance of " + std::to_string(dist) + " reaches before the first output byte"; return THMR_ERR_INVALID; }
            uint8_t* o = buf + pos;
            const uint8_t* f = o - dist;
            if (dist >= (size_t)length) memcpy(o, f, (size_t)length);
            else for (int k = 0; k < length; ++k) o[k] = f[k];
            pos += (size_t)length;
        }
    }
    if (const int rc = flush(false)) return rc < 0 ? rc : 0;
    in.bits >>= in.nbits & 7; in.nbits -= in.nbits & 7;
    if (!in.get(32, v)) return early();
    const uint32_t stored = (v & 255) << 24 | ((v >> 8) & 255) << 16 | ((v >> 16) & 255) << 8 | v >> 24;
    if (stored != (ad_b << 16 | ad_a)) { err = "wrong Adler-32 behind the deflate stream"; return THMR_ERR_INVALID; }
    (void)before;
    ended = true;
    return 0;
}

// A sink into one buffer of a given capacity (thmr_png_inflate).
struct BufferSink {
    uint8_t* out;
    int64_t capacity, n = 0;
    std::string* err;
    int64_t want() const { return INT64_MAX; }
    int put(const uint8_t* p, size_t k) {
        if ((int64_t)k > capacity - n) { *err = "the output exceeds the capacity of " + std::to_string(capacity) + " bytes"; return THMR_ERR_INVALID; }
        memcpy(out + n, p, k);
        n += (int64_t)k;
        return 0;
    }
};

inline int inflate_buffer(const uint8_t* z, size_t len, uint8_t* out, int64_t capacity, int64_t& written, std::string& err) {
    const Segment seg{z, len, 0};
    Input in(&seg, 1, false);
    BufferSink sink{out, capacity, 0, &err};
    bool ended;
    const int rc = inflate(in, sink, ended, err);
    written = sink.n;
    return rc;
}

// ---- the rows a window needs ----
inline int make_plan(const Header& h, const int32_t* window, Plan& p, std::string& err) {
    memset(&p, 0, sizeof(p));
    p.height = h.H; p.width = h.W; p.bit_depth = h.depth; p.colour_type = h.ctype; p.bpp = h.bpp;
    p.palette_entries = h.palette_entries;
    memcpy(p.palette, h.palette, sizeof(p.palette));
    if (window) { p.win_x0 = window[0]; p.win_y0 = window[1]; p.win_w = window[2]; p.win_h = window[3]; }
    else { p.win_w = h.W; p.win_h = h.H; }
    if (p.win_x0 < 0 || p.win_y0 < 0 || p.win_w < 0 || p.win_h < 0 || (int64_t)p.win_x0 + p.win_w > h.W || (int64_t)p.win_y0 + p.win_h > h.H) {
        err = "the window does not lie inside the " + std::to_string(h.W) + " x " + std::to_string(h.H) + " frame";
        return THMR_ERR_INVALID;
    }
    if (p.win_w && p.win_h) p.kept_row_bytes = (p.win_x0 + p.win_w) * h.bpp;        // at most 32767 * 8
    return 0;
}

inline int64_t rows_bound(const Plan& p) {
    return (p.win_w && p.win_h) ? (int64_t)(p.win_y0 + p.win_h) * (1 + (int64_t)p.kept_row_bytes) : 0;
}

// The inflate's sink for a window: cuts the stream into rows, keeps bytes [0, 1 + kept) of each row from the restart row on, and moves
// the write position back to the start whenever it meets a row at or above y0 whose filter (None, Sub) ignores the row above.
struct RowSink {
    uint8_t* out;
    int64_t full, keep;             // bytes of a row in the stream / kept of it, the filter byte included
    int32_t y0, yend, H;
    int32_t row = 0, row0 = 0;
    int64_t col = 0;
    std::string* err;
    int64_t want() const { return yend < H ? (int64_t)(yend - row) * full - col : INT64_MAX; }
    int put(const uint8_t* p, size_t n) {
        while (n) {
            if (row >= yend) {
                if (yend < H) return 1;
                *err = "the stream holds more than the frame's rows";
                return THMR_ERR_INVALID;
            }
            if (col == 0) {
                if (*p > 4) { *err = "row " + std::to_string(row) + " has filter byte " + std::to_string(*p); return THMR_ERR_INVALID; }
                if (*p <= 1 && row <= y0) row0 = row;
            }
            size_t k = (size_t)(full - col);
            if (k > n) k = n;
            if (col < keep) {
                const size_t c = (size_t)(keep - col) < k ? (size_t)(keep - col) : k;
                memcpy(out + (int64_t)(row - row0) * keep + col, p, c);
            }
            col += (int64_t)k; p += k; n -= k;
            if (col == full) { col = 0; ++row; }
        }
        return (row >= yend && yend < H) ? 1 : 0;
    }
};

// Rows of 1 + kept_row_bytes (filter byte first) -> the unfiltered bytes, rows of kept_row_bytes.  The first row's filter ignores the
// row above, or the row is row 0 of the frame, whose row above is zeros.
inline void unfilter(const uint8_t* rows, int32_t nrows, int32_t krb, int32_t bpp, uint8_t* plane) {
    for (int32_t r = 0; r < nrows; ++r) {
        const uint8_t* src = rows + (int64_t)r * (1 + krb);
        const int f = src[0];
        ++src;
        uint8_t* cur = plane + (int64_t)r * krb;
        const uint8_t* up = r ? cur - krb : nullptr;
        for (int32_t i = 0; i < krb; ++i) {
            const int a = i >= bpp ? cur[i - bpp] : 0, b = up ? up[i] : 0, c = (up && i >= bpp) ? up[i - bpp] : 0;
            cur[i] = pngdm::reconstruct(f, src[i], a, b, c);
        }
    }
}

// thmr_png_inflate_window behind its argument checks: the plan, and (rows != null) the kept rows.
inline int inflate_window(const uint8_t* data, size_t len, const int32_t* window, uint8_t* rows, int64_t capacity, Plan& plan,
                          int64_t* bytes_needed, std::string& err) {
    Header h;
    int rc = parse_supported(data, len, h, err);
    if (rc) return rc;
    if ((rc = make_plan(h, window, plan, err)) != 0) return rc;
    const int64_t bound = rows_bound(plan);
    if (bytes_needed) *bytes_needed = bound;
    if (!rows || bound == 0) return 0;
    if (capacity < bound) { err = "the row buffer holds " + std::to_string(capacity) + " bytes, the window needs " + std::to_string(bound); return THMR_ERR_INVALID; }
    Input in(h.idat.data(), h.idat.size(), true);
    RowSink sink{rows, 1 + (int64_t)h.W * h.bpp, 1 + (int64_t)plan.kept_row_bytes, plan.win_y0, plan.win_y0 + plan.win_h, h.H, 0, 0, 0, &err};
    bool ended;
    if ((rc = inflate(in, sink, ended, err)) != 0) return rc;
    if (sink.row < sink.yend) { err = "the stream ends after " + std::to_string(sink.row) + " rows, the window needs " + std::to_string(sink.yend); return THMR_ERR_INVALID; }
    plan.row0 = sink.row0;
    plan.rows_kept = sink.yend - sink.row0;
    plan.rows_inflated = sink.row;
    if (bytes_needed) *bytes_needed = (int64_t)plan.rows_kept * (1 + (int64_t)plan.kept_row_bytes);
    if (h.ctype == 3 && h.palette_entries < 256) {
        // an index beyond the palette is refused here, on the host, so that the device never meets one: bpp is 1, the pass is cheap
        std::vector<uint8_t> plane;
        try { plane.resize((size_t)plan.rows_kept * (size_t)plan.kept_row_bytes); } catch (const std::bad_alloc&) { err = "out of host memory for the palette check"; return THMR_ERR_NOMEM; }
        unfilter(rows, plan.rows_kept, plan.kept_row_bytes, 1, plane.data());
        for (int32_t y = plan.win_y0; y < plan.win_y0 + plan.win_h; ++y) {
            const uint8_t* r = plane.data() + (int64_t)(y - plan.row0) * plan.kept_row_bytes;
            for (int32_t x = plan.win_x0; x < plan.win_x0 + plan.win_w; ++x)
                if (r[x] >= h.palette_entries) {
                    err = "palette index " + std::to_string(r[x]) + " at (" + std::to_string(x) + ", " + std::to_string(y) + ") is beyond the " + std::to_string(h.palette_entries) + " entries of PLTE";
                    return THMR_ERR_INVALID;
                }
        }
    }
    return 0;
}

// What thmr_png_decode_batch checks of one item's plan and rows before the device sees them (decode_host's rows pass by construction).
inline int check_rows(const Plan& p, const uint8_t* rows, std::string& err) {
    for (int32_t r = 0; r < p.rows_kept; ++r) {
        const int f = rows[(int64_t)r * (1 + (int64_t)p.kept_row_bytes)];
        if (f > 4) { err = "kept row " + std::to_string(r) + " has filter byte " + std::to_string(f); return THMR_ERR_INVALID; }
        if (r == 0 && f > 1 && p.row0 != 0) { err = "the first kept row is filtered against a row that was not kept"; return THMR_ERR_INVALID; }
    }
    return 0;
}

// Unfiltered rows -> the window's pixels.
inline void convert(const Plan& p, const uint8_t* plane, int32_t bgr, uint8_t* out, int64_t row_stride) {
    for (int32_t yy = 0; yy < p.win_h; ++yy) {
        const uint8_t* src = plane + (int64_t)(p.win_y0 - p.row0 + yy) * p.kept_row_bytes + (int64_t)p.win_x0 * p.bpp;
        uint8_t* o = out + (int64_t)yy * row_stride;
        for (int32_t xx = 0; xx < p.win_w; ++xx) pngdm::to_bgr(p.colour_type, p.bit_depth, src + (int64_t)xx * p.bpp, &p.palette[0][0], bgr, o + 3 * xx);
    }
}

inline int decode(const uint8_t* data, size_t len, const int32_t* window, int32_t bgr, uint8_t* out, int64_t row_stride, std::string& err) {
    Plan plan;
    int64_t need = 0;
    int rc = inflate_window(data, len, window, nullptr, 0, plan, &need, err);
    if (rc) return rc;
    if (need == 0) return 0;
    if (!out) { err = "null out"; return THMR_ERR_INVALID; }
    if (row_stride < (int64_t)plan.win_w * 3) { err = "row_stride is less than win_w * 3"; return THMR_ERR_INVALID; }
    std::vector<uint8_t> rows, plane;
    try { rows.resize((size_t)need); } catch (const std::bad_alloc&) { err = "out of host memory for the rows"; return THMR_ERR_NOMEM; }
    if ((rc = inflate_window(data, len, window, rows.data(), need, plan, &need, err)) != 0) return rc;
    try { plane.resize((size_t)plan.rows_kept * (size_t)plan.kept_row_bytes); } catch (const std::bad_alloc&) { err = "out of host memory for the rows"; return THMR_ERR_NOMEM; }
    unfilter(rows.data(), plan.rows_kept, plan.kept_row_bytes, plan.bpp, plane.data());
    convert(plan, plane.data(), bgr, out, row_stride);
    return 0;
}

}  // namespace pngdh
