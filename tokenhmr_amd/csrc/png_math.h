// The arithmetic and the selection rules of the PNG encoder, shared by the kernels (png.hip) and the CPU encode (png_host.h): pixel
// conversion, the five row filters and their cost, the candidate distances and the match rule of the LZ77 stage, and the fixed-Huffman
// token codes.  Everything is integer (the one float product of the conversion has a single rounding), so both sides give the same bytes.
// Compiles with or without HIP: PNG_HD is __host__ __device__ under hipcc and nothing otherwise.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define PNG_HD __host__ __device__ inline
#else
#define PNG_HD inline
#endif

namespace pngm {

constexpr int SEGMENT = 16384;          // bytes of the filtered stream per independently compressed segment (<= 32768: every distance is legal)
constexpr int PAD = 8;                  // readable bytes a segment buffer keeps past its end (the match loop compares 4 at a time)
constexpr int MIN_MATCH = 3, MAX_MATCH = 258;
constexpr int FAR = 4096;               // a match further back than this needs 4 bytes: 3 would cost more bits than 3 literals
constexpr int MAX_CAND = 8;
constexpr uint32_t ADLER_MOD = 65521;

// What the encoder needs of one image besides its pixels.
struct Image {
    int32_t dtype, w, h, c;
    int64_t sy, sx, sc;
    float scale;
    int32_t rounding, swap_rb;
};

PNG_HD int row_bytes(const Image& im) { return im.w * im.c; }

// float -> byte.  rounding 0: nearest even, saturated; 1: clamped, then truncated.  NaN -> 0.
PNG_HD uint8_t convert(float x, float scale, int rounding) {
    const float v = x * scale;
    if (!(v > 0.0f)) return 0;          // negatives, -0, NaN
    if (v >= 255.0f) return 255;
    return (uint8_t)(int)(rounding == 0 ? rintf(v) : v);
}

// Byte i of row y of the image as the file holds it (channel order swapped where asked).
PNG_HD uint8_t sample(const Image& im, const void* pixels, int y, int i) {
    const int x = i / im.c;
    int ch = i - x * im.c;
    if (im.swap_rb && im.c >= 3 && ch < 3) ch = 2 - ch;
    const int64_t at = (int64_t)y * im.sy + (int64_t)x * im.sx + (int64_t)ch * im.sc;
    if (im.dtype == 0) return static_cast<const uint8_t*>(pixels)[at];
    return convert(static_cast<const float*>(pixels)[at], im.scale, im.rounding);
}

PNG_HD int paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// The residual of filter f for a byte x with left a, above b, above-left c.
PNG_HD uint8_t residual(int f, int x, int a, int b, int c) {
    switch (f) {
        case 0: return (uint8_t)x;
        case 1: return (uint8_t)(x - a);
        case 2: return (uint8_t)(x - b);
        case 3: return (uint8_t)(x - ((a + b) >> 1));
        default: return (uint8_t)(x - paeth(a, b, c));
    }
}

// libpng's heuristic: a residual counts as the magnitude of the signed byte.
PNG_HD uint32_t cost(uint8_t r) { return r < 128 ? r : 256u - r; }

// The filter with the smallest cost, ties to the lowest number.
PNG_HD int best_filter(const uint64_t* sum) {
    int best = 0;
    for (int f = 1; f < 5; ++f)
        if (sum[f] < sum[best]) best = f;
    return best;
}

// The four neighbours of byte i of row y (zero outside the image).
PNG_HD void neighbours(const Image& im, const void* pixels, int y, int i, int& x, int& a, int& b, int& c) {
    x = sample(im, pixels, y, i);
    a = i >= im.c ? sample(im, pixels, y, i - im.c) : 0;
    b = y > 0 ? sample(im, pixels, y - 1, i) : 0;
    c = (y > 0 && i >= im.c) ? sample(im, pixels, y - 1, i - im.c) : 0;
}

// The distances the matcher tries, in order of preference: the previous byte, the previous 1 ... 4 pixels, the previous 1 ... 3 rows.
PNG_HD int candidates(int bpp, int stride /* 1 + row bytes */, int* cand) {
    const int all[MAX_CAND] = {1, bpp, 2 * bpp, 3 * bpp, 4 * bpp, stride, 2 * stride, 3 * stride};
    int n = 0;
    for (int k = 0; k < MAX_CAND; ++k) {
        bool seen = all[k] >= SEGMENT;
        for (int j = 0; j < n; ++j) seen = seen || cand[j] == all[k];
        if (!seen) cand[n++] = all[k];
    }
    return n;
}

// Bytes from p on that equal the bytes `d` back, at most `limit`.  seg keeps PAD readable bytes past its end.
PNG_HD int run_length(const uint8_t* seg, int p, int d, int limit) {
    int len = 0;
    while (len < limit) {
        uint32_t x, y;
        memcpy(&x, seg + p + len, 4);
        memcpy(&y, seg + p + len - d, 4);
        const uint32_t diff = x ^ y;
        if (diff) { len += __builtin_ctz(diff) >> 3; break; }
        len += 4;
    }
    return len < limit ? len : limit;
}

// The match at position p of a segment of n bytes: the longest run over the candidates that lie inside the segment, the first
// candidate on a tie; len 0 = none.  It depends on the segment's bytes alone, never on what was chosen before p.
PNG_HD void find_match(const uint8_t* seg, int p, int n, const int* cand, int ncand, int& len, int& dist) {
    len = 0; dist = 0;
    const int limit = n - p < MAX_MATCH ? n - p : MAX_MATCH;
    if (limit < MIN_MATCH) return;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll          // the candidates stay in registers
#endif
    for (int k = 0; k < MAX_CAND; ++k) {
        if (k >= ncand) break;
        const int d = cand[k];
        if (d > p || seg[p] != seg[p - d]) continue;
        const int l = run_length(seg, p, d, limit);
        if (l > len && l >= (d > FAR ? MIN_MATCH + 1 : MIN_MATCH)) { len = l; dist = d; }
        if (len == limit) break;        // no later candidate is longer, and a tie goes to the earlier one
    }
}

PNG_HD uint32_t reverse_bits(uint32_t v, int n) {
    uint32_t r = 0;
    for (int i = 0; i < n; ++i) r |= ((v >> i) & 1u) << (n - 1 - i);
    return r;
}

// A literal / length symbol 0 ... 287 of the fixed Huffman code, already in stream order (codes go out most significant bit first).
PNG_HD void fixed_symbol(int s, uint32_t& bits, int& n) {
    if (s < 144) { bits = reverse_bits(0x30 + s, 8); n = 8; }
    else if (s < 256) { bits = reverse_bits(0x190 + (s - 144), 9); n = 9; }
    else if (s < 280) { bits = reverse_bits(s - 256, 7); n = 7; }
    else { bits = reverse_bits(0xC0 + (s - 280), 8); n = 8; }
}

// One token as stream bits (appended least significant bit first): a literal (len 0), or length + distance with their extra bits.
PNG_HD void token_bits(int lit, int len, int dist, uint64_t& bits, int& n) {
    uint32_t b; int k;
    if (len == 0) { fixed_symbol(lit, b, k); bits = b; n = k; return; }
    int code, e = 0, extra = 0;
    const int l = len - 3;
    if (len == 258) code = 285;
    else if (l < 8) code = 257 + l;
    else { e = (31 - __builtin_clz((unsigned)l)) - 2; code = 261 + 4 * e + ((l >> e) & 3); extra = l & ((1 << e) - 1); }
    fixed_symbol(code, b, k);
    bits = b; n = k;
    bits |= (uint64_t)extra << n; n += e;
    const int d = dist - 1;
    int dcode, de = 0, dextra = 0;
    if (d < 4) dcode = d;
    else { de = (31 - __builtin_clz((unsigned)d)) - 1; dcode = 2 * de + 2 + ((d >> de) & 1); dextra = d & ((1 << de) - 1); }
    bits |= (uint64_t)reverse_bits(dcode, 5) << n; n += 5;
    bits |= (uint64_t)dextra << n; n += de;
}

// How a segment ends, after the end-of-block code: bits of the trailer and the stream's byte length.
// coded bits so far (header + tokens) -> total bytes of the coded form, the sync marker of a non-final segment included.
PNG_HD int64_t coded_bytes(int64_t bits_before_eob, bool last) {
    int64_t bits = bits_before_eob + 7;                 // end of block: seven zero bits
    if (!last) bits += 3;                               // the empty stored block's header
    int64_t bytes = (bits + 7) >> 3;
    if (!last) bytes += 4;                              // 00 00 FF FF
    return bytes;
}

// Adler-32 of a stream from the per-segment partials s1 = sum of bytes, s2 = sum of (n - i) * byte[i], both mod 65521.
PNG_HD void adler_append(uint32_t& a, uint32_t& b, uint32_t s1, uint32_t s2, uint32_t n) {
    b = (uint32_t)((b + (uint64_t)(n % ADLER_MOD) * a + s2) % ADLER_MOD);
    a = (a + s1) % ADLER_MOD;
}

}  // namespace pngm
