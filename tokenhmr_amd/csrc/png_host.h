// The host half of the PNG encoder (include/tokenhmr_hip.h): argument checks, the container (signature, IHDR, IDAT, IEND, CRC-32,
// Adler-32 from the segment partials), and the whole encode on the CPU with the arithmetic of png_math.h — the oracle of the kernels,
// and what a caller without a device gets.  Host only, no HIP call.
#pragma once
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "image_item_host.h"
#include "png_math.h"

namespace pngh {

constexpr int64_t CONTAINER_BYTES = 57;     // 8 signature + 25 IHDR + 12 IDAT framing + 12 IEND
constexpr int64_t IDAT_DATA_AT = 41;        // the zlib stream's offset in the file

inline int64_t stream_bytes(int32_t w, int32_t h, int32_t c) { return (int64_t)h * (1 + (int64_t)w * c); }
inline int64_t segments(int64_t stream) { return (stream + pngm::SEGMENT - 1) / pngm::SEGMENT; }

inline int64_t bound(int32_t w, int32_t h, int32_t c) {
    if (w < 1 || h < 1 || (c != 1 && c != 3 && c != 4)) return 0;
    const int64_t raw = stream_bytes(w, h, c);
    if (raw >= ((int64_t)1 << 31)) return 0;
    return raw + 5 * segments(raw) + 6 + CONTAINER_BYTES;
}

using imgitem::image_of;

// 0, or the status with the reason in err.  Pointers and capacity included.
inline int check_item(const thmr_png_item& it, std::string& err) {
    if (const int rc = imgitem::check_source(it, "writes", err)) return rc;
    if (it.width < 1 || it.height < 1) {
        err = "width and height must be at least 1, got " + std::to_string(it.width) + " x " + std::to_string(it.height);
        return THMR_ERR_INVALID;
    }
    if (stream_bytes(it.width, it.height, it.channels) >= ((int64_t)1 << 31)) { err = "the filtered stream would reach 2^31 bytes"; return THMR_ERR_INVALID; }
    if (it.rounding != THMR_PNG_ROUND_NEAREST && it.rounding != THMR_PNG_ROUND_TRUNC) { err = "rounding must be THMR_PNG_ROUND_NEAREST or _TRUNC"; return THMR_ERR_INVALID; }
    if (it.compression != THMR_PNG_FIXED && it.compression != THMR_PNG_DYNAMIC) {
        err = "compression must be THMR_PNG_FIXED or THMR_PNG_DYNAMIC, got " + std::to_string(it.compression);
        return THMR_ERR_INVALID;
    }
    return imgitem::check_buffers(it, bound(it.width, it.height, it.channels), "thmr_png_bound", err);
}

// thmr_png_code_lengths: the arguments checked, then pngm::code_lengths.
inline int code_lengths(const int32_t* freq, int32_t n, int32_t max_bits, int32_t* lens, std::string& err) {
    if (!freq || !lens) { err = "null freq or lens"; return THMR_ERR_INVALID; }
    if (n < 1 || n > pngm::N_LL || max_bits < 1 || max_bits > pngm::MAX_BITS) { err = "n must be 1 ... 286 and max_bits 1 ... 15"; return THMR_ERR_INVALID; }
    int used = 0;
    for (int s = 0; s < n; ++s) {
        if (freq[s] < 0 || freq[s] >= (1 << 22)) { err = "a frequency must be 0 ... 2^22 - 1, got " + std::to_string(freq[s]); return THMR_ERR_INVALID; }
        used += freq[s] > 0;
    }
    if (used > (1 << max_bits)) { err = std::to_string(used) + " symbols in use cannot have codes of at most " + std::to_string(max_bits) + " bits"; return THMR_ERR_INVALID; }
    int32_t a[pngm::N_LL], b[pngm::N_LL];
    pngm::code_lengths(freq, n, max_bits, lens, a, b);
    return 0;
}

inline uint32_t crc32(const uint8_t* p, size_t n, uint32_t crc = 0) {
    static const struct Table {
        uint32_t t[8][256];
        Table() {
            for (uint32_t i = 0; i < 256; ++i) {
                uint32_t c = i;
                for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
                t[0][i] = c;
            }
            for (int s = 1; s < 8; ++s)
                for (uint32_t i = 0; i < 256; ++i) t[s][i] = t[0][t[s - 1][i] & 0xFF] ^ (t[s - 1][i] >> 8);
        }
    } T;
    crc = ~crc;
    while (n >= 8) {
        uint32_t a, b;
        memcpy(&a, p, 4); memcpy(&b, p + 4, 4);
        a ^= crc;
        crc = T.t[7][a & 0xFF] ^ T.t[6][(a >> 8) & 0xFF] ^ T.t[5][(a >> 16) & 0xFF] ^ T.t[4][a >> 24] ^
              T.t[3][b & 0xFF] ^ T.t[2][(b >> 8) & 0xFF] ^ T.t[1][(b >> 16) & 0xFF] ^ T.t[0][b >> 24];
        p += 8; n -= 8;
    }
    while (n--) crc = T.t[0][(crc ^ *p++) & 0xFF] ^ (crc >> 8);
    return ~crc;
}

// The CRC of two byte strings joined, from the CRC of each and the second one's length: crc1 is advanced over len2 zero bytes by
// repeated squaring of the "one zero bit" operator over GF(2), then the second CRC is added.  Chunks of one IDAT can so be summed apart.
inline uint32_t gf2_times(const uint32_t* mat, uint32_t vec) {
    uint32_t sum = 0;
    for (; vec; vec >>= 1, ++mat)
        if (vec & 1) sum ^= *mat;
    return sum;
}
inline void gf2_square(uint32_t* square, const uint32_t* mat) {
    for (int n = 0; n < 32; ++n) square[n] = gf2_times(mat, mat[n]);
}
inline uint32_t crc32_combine(uint32_t crc1, uint32_t crc2, uint64_t len2) {
    if (len2 == 0) return crc1;
    uint32_t even[32], odd[32];
    odd[0] = 0xEDB88320u;                       // the operator of one zero bit
    for (int n = 1; n < 32; ++n) odd[n] = 1u << (n - 1);
    gf2_square(even, odd);                      // two bits
    gf2_square(odd, even);                      // four
    for (;;) {
        gf2_square(even, odd);                  // the first pass: one zero byte
        if (len2 & 1) crc1 = gf2_times(even, crc1);
        if (!(len2 >>= 1)) break;
        gf2_square(odd, even);
        if (len2 & 1) crc1 = gf2_times(odd, crc1);
        if (!(len2 >>= 1)) break;
    }
    return crc1 ^ crc2;
}

inline void put32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v; }

// Everything of the file around the deflate segments, which already lie at out + IDAT_DATA_AT + 2 (`body` bytes of them).  body_crc:
// the CRC-32 of those bytes where the caller has it already (summed in chunks), else it is computed here.  Returns the file's length.
inline int64_t finish_file(uint8_t* out, int32_t w, int32_t h, int32_t c, int64_t body, uint32_t adler, const uint32_t* body_crc = nullptr) {
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    memcpy(out, sig, 8);
    uint8_t* p = out + 8;
    put32(p, 13); memcpy(p + 4, "IHDR", 4);
    put32(p + 8, (uint32_t)w); put32(p + 12, (uint32_t)h);
    p[16] = 8; p[17] = c == 1 ? 0 : c == 3 ? 2 : 6; p[18] = 0; p[19] = 0; p[20] = 0;
    put32(p + 21, crc32(p + 4, 17));
    p += 25;
    const int64_t zlen = 2 + body + 4;
    put32(p, (uint32_t)zlen); memcpy(p + 4, "IDAT", 4);
    p[8] = 0x78; p[9] = 0x01;
    put32(p + 10 + body, adler);
    uint32_t crc = crc32(p + 4, 6);             // "IDAT" 78 01
    crc = body_crc ? crc32_combine(crc, *body_crc, (uint64_t)body) : crc32(p + 10, (size_t)body, crc);
    put32(p + 8 + zlen, crc32(p + 10 + body, 4, crc));
    p += 12 + zlen;
    put32(p, 0); memcpy(p + 4, "IEND", 4); put32(p + 8, 0xAE426082u);
    return (p + 12) - out;
}

// LSB-first bit writer into a byte vector.
struct BitWriter {
    std::vector<uint8_t>& v;
    uint64_t acc = 0;
    int n = 0;
    void put(uint64_t bits, int k) {
        acc |= bits << n; n += k;
        while (n >= 8) { v.push_back((uint8_t)acc); acc >>= 8; n -= 8; }
    }
    void align() { if (n) { v.push_back((uint8_t)acc); acc = 0; n = 0; } }
};

inline void stored_block(const uint8_t* seg, int n, bool last, std::vector<uint8_t>& out) {
    out.push_back(last ? 1 : 0);
    out.push_back((uint8_t)n); out.push_back((uint8_t)(n >> 8));
    out.push_back((uint8_t)~n); out.push_back((uint8_t)(~n >> 8));
    out.insert(out.end(), seg, seg + n);
}

// How a coded segment ends behind its end-of-block code.
inline void end_segment(BitWriter& bw, bool last, std::vector<uint8_t>& out) {
    if (!last) {
        bw.put(0, 3);
        bw.align();
        const uint8_t sync[4] = {0, 0, 0xFF, 0xFF};
        out.insert(out.end(), sync, sync + 4);
    } else {
        bw.align();
    }
}

// The segment as a dynamic-Huffman block (the block rule of png_math.h), or as the stored block where that is smaller still; false,
// and nothing written, where the dynamic block does not take strictly fewer bits than the fixed one.
inline bool deflate_segment_dynamic(const uint8_t* seg, int n, bool last, const int* cand, int ncand, std::vector<uint8_t>& out) {
    struct Token { int lit, len, dist; };
    std::vector<Token> tokens;
    pngm::DynBlock k;
    memset(&k, 0, sizeof(k));
    int64_t fixed = 3 + 7;
    for (int p = 0; p < n;) {
        int len, dist, lsym, e, extra, dsym, de, dextra;
        pngm::find_match(seg, p, n, cand, ncand, len, dist);
        pngm::token_parts(seg[p], len, dist, lsym, e, extra, dsym, de, dextra);
        ++k.ll[lsym];
        if (dsym >= 0) ++k.d[dsym];
        fixed += pngm::fixed_token_bits(lsym, e, dsym, de);
        tokens.push_back({seg[p], len, dist});
        p += len ? len : 1;
    }
    const int64_t bits = pngm::dynamic_block(k);
    if (bits >= fixed) return false;
    const int eob = (int)((uint32_t)k.ll[pngm::END_OF_BLOCK] >> 16);
    if (pngm::coded_bytes(bits - eob, last, eob) > (int64_t)n + 5) {
        stored_block(seg, n, last, out);
        return true;
    }
    BitWriter bw{out};
    uint64_t t;
    int m;
    for (int i = 0; i < pngm::header_pieces(k); ++i) {
        pngm::header_piece(k, i, last, t, m);
        bw.put(t, m);
    }
    for (const Token& tk : tokens) {
        pngm::dynamic_token_bits(k, tk.lit, tk.len, tk.dist, t, m);
        bw.put(t, m);
    }
    bw.put((uint32_t)k.ll[pngm::END_OF_BLOCK] & 0xFFFFu, eob);
    end_segment(bw, last, out);
    return true;
}

// One segment (n bytes at seg, PAD readable bytes behind) -> its deflate bytes appended to out; the Adler partials in s1, s2.
inline void deflate_segment(const uint8_t* seg, int n, bool last, const int* cand, int ncand, int compression, std::vector<uint8_t>& out, uint32_t& s1,
                            uint32_t& s2) {
    uint64_t a = 0, b = 0;
    for (int i = 0; i < n; ++i) { a += seg[i]; b += (uint64_t)(n - i) * seg[i]; }
    s1 = (uint32_t)(a % pngm::ADLER_MOD); s2 = (uint32_t)(b % pngm::ADLER_MOD);
    if (compression == THMR_PNG_DYNAMIC && deflate_segment_dynamic(seg, n, last, cand, ncand, out)) return;
    const size_t start = out.size();
    BitWriter bw{out};
    bw.put((last ? 1u : 0u) | 2u, 3);                   // BFINAL, BTYPE 01
    int64_t bits = 3;
    for (int p = 0; p < n;) {
        int len, dist, k;
        uint64_t t;
        pngm::find_match(seg, p, n, cand, ncand, len, dist);
        pngm::token_bits(seg[p], len, dist, t, k);
        bw.put(t, k); bits += k;
        p += len ? len : 1;
    }
    if (pngm::coded_bytes(bits, last) > (int64_t)n + 5) {       // a stored block is smaller
        out.resize(start);
        stored_block(seg, n, last, out);
        return;
    }
    bw.put(0, 7);
    end_segment(bw, last, out);
}

// The filtered stream of an image whose pixels are host memory.
inline void filter_image(const pngm::Image& im, const void* pixels, std::vector<uint8_t>& stream) {
    const int rb = pngm::row_bytes(im);
    stream.assign((size_t)im.h * (1 + rb) + pngm::PAD, 0);
    for (int y = 0; y < im.h; ++y) {
        uint64_t sum[5] = {0, 0, 0, 0, 0};
        for (int i = 0; i < rb; ++i) {
            int x, a, b, c;
            pngm::neighbours(im, pixels, y, i, x, a, b, c);
            for (int f = 0; f < 5; ++f) sum[f] += pngm::cost(pngm::residual(f, x, a, b, c));
        }
        const int f = pngm::best_filter(sum);
        uint8_t* row = stream.data() + (size_t)y * (1 + rb);
        row[0] = (uint8_t)f;
        for (int i = 0; i < rb; ++i) {
            int x, a, b, c;
            pngm::neighbours(im, pixels, y, i, x, a, b, c);
            row[1 + i] = pngm::residual(f, x, a, b, c);
        }
    }
}

// The whole file on the CPU.  The item is already checked.
inline void encode(thmr_png_item& it) {
    const pngm::Image im = image_of(it);
    std::vector<uint8_t> stream, body, seg((size_t)pngm::SEGMENT + pngm::PAD);
    filter_image(im, it.pixels, stream);
    const int64_t total = stream_bytes(im.w, im.h, im.c), nseg = segments(total);
    int cand[pngm::MAX_CAND];
    const int ncand = pngm::candidates(im.c, 1 + pngm::row_bytes(im), cand);
    uint32_t a = 1, b = 0;
    for (int64_t s = 0; s < nseg; ++s) {
        const int64_t off = s * pngm::SEGMENT;
        const int n = (int)(total - off < pngm::SEGMENT ? total - off : pngm::SEGMENT);
        memcpy(seg.data(), stream.data() + off, (size_t)n);
        memset(seg.data() + n, 0, pngm::PAD);
        uint32_t s1, s2;
        deflate_segment(seg.data(), n, s == nseg - 1, cand, ncand, it.compression, body, s1, s2);
        pngm::adler_append(a, b, s1, s2, (uint32_t)n);
    }
    memcpy(it.out + IDAT_DATA_AT + 2, body.data(), body.size());
    it.written = finish_file(it.out, im.w, im.h, im.c, (int64_t)body.size(), (b << 16) | a);
}

}  // namespace pngh
