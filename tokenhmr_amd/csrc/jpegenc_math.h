// The arithmetic and the coding rules of the baseline JPEG encoder, shared by the kernels (jpegenc.hip) and the CPU encode
// (jpegenc_host.h): libjpeg's default compression pipeline restated in integers — jccolor.c's 16-bit fixed-point RGB -> YCbCr, the h2v2
// box downsampler with its alternating bias and libjpeg's edge expansion, jfdctint.c (JDCT_ISLOW, the constants of jpeg_math.h),
// quantisation by 8 q with halves away from zero, and the Huffman coding of a block with the Annex K tables — or, for an image flagged
// THMR_JPEG_OPTIMIZE, with tables made from that image's own symbol statistics as libjpeg's optimize_coding makes them (the symbol
// walk, the table routine and its rule are at the end of this file).  The samples come from imgsrc::sample (image_source.h), the one
// pixel conversion of both encoders.  Everything is integer, so both sides give the same bytes.  Compiles with or without HIP.
//
// The bound of the optimised mode: of the two ways — a second bound, or a proof that the first holds — the second bound was chosen
// (thmr_jpeg_encode_bound_flags).  A DC table of an image's own has up to 12 symbols and the pseudo-symbol, so a DC code can take 12
// bits where Annex K's longest takes 11: MAX_BLOCK_BITS_OPT = MAX_BLOCK_BITS + 1.  An AC code stays within 16 bits by the limit, and
// such a table has no more symbols than an Annex K one (12 / 162), so the header is no longer.
#pragma once
#include <stdint.h>

#include "image_source.h"
#include "jpeg_math.h"

namespace jpegem {

constexpr int MAX_BLOCK_BITS = (11 + 11) + 63 * (16 + 10);      // Annex K: the longest DC code (chroma category 11) + its bits, 63 x the longest AC code + 10 bits
constexpr int TABLE_WORDS = 16 + 256;                           // one class's codes: DC categories 0 ... 11, then AC (run << 4 | size) at 16 +
constexpr int EOB = 0x00, ZRL = 0xF0;

// One image as the encoder sees it besides its pixels and tables.
struct Frame {
    imgsrc::Image im;
    int32_t ncomp;              // 1 (grey) or 3
    int32_t sub;                // 1: 4:2:0 (three components only), 0: 4:4:4
    int32_t mcux, mcuy;         // MCUs per row / column
    int32_t bpm;                // blocks per MCU: 1, 3 or 6
    int32_t lbw, lbh;           // real luma blocks per row / column: ceil(W / 8), ceil(H / 8)
};

JPEG_HD Frame frame_of(const imgsrc::Image& im, int sub) {
    Frame f;
    f.im = im;
    f.ncomp = im.c == 1 ? 1 : 3;
    f.sub = f.ncomp == 3 && sub ? 1 : 0;
    const int m = f.sub ? 16 : 8;
    f.mcux = (im.w + m - 1) / m; f.mcuy = (im.h + m - 1) / m;
    f.bpm = f.ncomp == 1 ? 1 : f.sub ? 6 : 3;
    f.lbw = (im.w + 7) / 8; f.lbh = (im.h + 7) / 8;
    return f;
}

JPEG_HD int zigzag_of_natural(int k) {
    const uint8_t z[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30, 41, 43, 9,  11, 18, 24, 31, 40, 44, 53,
                           10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};
    return z[k];
}

// Block k of MCU (mx, my): its component, its block coordinates in the component's grid, and whether it lies outside that grid (a
// dummy: luma of 4:2:0 only).
JPEG_HD void block_place(const Frame& f, int mx, int my, int k, int& comp, int& bx, int& by, bool& dummy) {
    dummy = false;
    if (f.sub && k < 4) {
        comp = 0; bx = 2 * mx + (k & 1); by = 2 * my + (k >> 1);
        dummy = bx >= f.lbw || by >= f.lbh;
    } else {
        comp = f.sub ? k - 3 : k; bx = mx; by = my;
    }
}

// The block (index in scan order) whose DC value predicts block b's: the nearest real block of the same component before it, -1 for
// the first.  Block 0 of an MCU is always real.
JPEG_HD int64_t dc_predecessor(const Frame& f, int64_t b) {
    const int64_t m = b / f.bpm;
    const int k = (int)(b - m * f.bpm);
    if (f.sub && k < 4) {
        int comp, bx, by;
        bool dummy;
        const int64_t m0 = k > 0 ? m : m - 1;
        if (m0 < 0) return -1;
        const int my = (int)(m0 / f.mcux), mx = (int)(m0 - (int64_t)my * f.mcux);
        for (int j = k > 0 ? k - 1 : 3; j > 0; --j) {
            block_place(f, mx, my, j, comp, bx, by, dummy);
            if (!dummy) return m0 * f.bpm + j;
        }
        return m0 * f.bpm;
    }
    return m > 0 ? b - f.bpm : -1;
}

JPEG_HD void rgb_to_ycc(int r, int g, int b, int& y, int& cb, int& cr) {
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    cb = (-11059 * r - 21709 * g + 32768 * b + 8388608 + 32767) >> 16;
    cr = (32768 * r - 27439 * g - 5329 * b + 8388608 + 32767) >> 16;
}

// Component `comp` of pixel (x, y), both inside the image.  The alpha of a 4-channel image is never read.
JPEG_HD int pixel_component(const imgsrc::Image& im, const void* pixels, int comp, int y, int x) {
    if (im.c == 1) return imgsrc::sample(im, pixels, y, x);
    const int r = imgsrc::sample(im, pixels, y, x * im.c), g = imgsrc::sample(im, pixels, y, x * im.c + 1), b = imgsrc::sample(im, pixels, y, x * im.c + 2);
    int yy, cb, cr;
    rgb_to_ycc(r, g, b, yy, cb, cr);
    return comp == 0 ? yy : comp == 1 ? cb : cr;
}

// Sample (row, col) of a component's padded plane, as libjpeg's edge expansion and h2v2 downsampler leave it.  A full-resolution
// component replicates the last pixel column and row.  A 4:2:0 chroma plane replicates its last DOWNSAMPLED row (not the pixel
// row), takes the pixel rows 2r and min(2r + 1, H - 1), the columns min(2c, W - 1) and min(2c + 1, W - 1), and rounds with the bias 1 for
// an even column and 2 for an odd one.
JPEG_HD int component_sample(const Frame& f, const void* pixels, int comp, int row, int col) {
    const imgsrc::Image& im = f.im;
    if (!(f.sub && comp > 0)) return pixel_component(im, pixels, comp, row < im.h ? row : im.h - 1, col < im.w ? col : im.w - 1);
    const int ch = (im.h + 1) / 2;
    const int r = row < ch ? row : ch - 1;
    const int y0 = 2 * r, y1 = 2 * r + 1 < im.h ? 2 * r + 1 : im.h - 1;
    const int x0 = 2 * col < im.w ? 2 * col : im.w - 1, x1 = 2 * col + 1 < im.w ? 2 * col + 1 : im.w - 1;
    const int sum = pixel_component(im, pixels, comp, y0, x0) + pixel_component(im, pixels, comp, y0, x1) + pixel_component(im, pixels, comp, y1, x0) +
                    pixel_component(im, pixels, comp, y1, x1);
    return (sum + ((col & 1) ? 2 : 1)) >> 2;
}

// One 8-point pass of jpeg_fdct_islow, v[0..7] in place.  first: the row pass (outputs scaled up by PASS1_BITS); else the column pass.
JPEG_HD void fdct8(int* v, bool first) {
    using namespace jpegm;
    const int tmp0 = v[0] + v[7], tmp7 = v[0] - v[7], tmp1 = v[1] + v[6], tmp6 = v[1] - v[6];
    const int tmp2 = v[2] + v[5], tmp5 = v[2] - v[5], tmp3 = v[3] + v[4], tmp4 = v[3] - v[4];
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    const int shift = first ? CONST_BITS - PASS1_BITS : CONST_BITS + PASS1_BITS;
    if (first) {
        v[0] = shl(tmp10 + tmp11, PASS1_BITS);
        v[4] = shl(tmp10 - tmp11, PASS1_BITS);
    } else {
        v[0] = descale(tmp10 + tmp11, PASS1_BITS);
        v[4] = descale(tmp10 - tmp11, PASS1_BITS);
    }
    int z1 = (tmp12 + tmp13) * FIX_0_541196100;
    v[2] = descale(z1 + tmp13 * FIX_0_765366865, shift);
    v[6] = descale(z1 + tmp12 * -FIX_1_847759065, shift);
    z1 = tmp4 + tmp7;
    int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
    const int z5 = (z3 + z4) * FIX_1_175875602;
    const int t4 = tmp4 * FIX_0_298631336, t5 = tmp5 * FIX_2_053119869, t6 = tmp6 * FIX_3_072711026, t7 = tmp7 * FIX_1_501321110;
    z1 *= -FIX_0_899976223; z2 *= -FIX_2_562915447;
    z3 = z3 * -FIX_1_961570560 + z5; z4 = z4 * -FIX_0_390180644 + z5;
    v[7] = descale(t4 + z1 + z3, shift);
    v[5] = descale(t5 + z2 + z4, shift);
    v[3] = descale(t6 + z2 + z3, shift);
    v[1] = descale(t7 + z1 + z4, shift);
}

// A DCT output (scaled by 8) over the table entry q: halves away from zero.
JPEG_HD int quantise(int c, int q) {
    const int a = c < 0 ? -c : c;
    const int v = (a + 4 * q) / (8 * q);
    return c < 0 ? -v : v;
}

// Entry k (natural order) of the table for `quality` 1 ... 100: cls 0 luma, 1 chroma.
JPEG_HD int quant_entry(int cls, int k, int quality) {
    const uint8_t luma[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                              18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,  49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
    const uint8_t chroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                                99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    const int v = ((cls ? chroma[k] : luma[k]) * s + 50) / 100;
    return v < 1 ? 1 : v > 255 ? 255 : v;
}

// The block of component `comp` at (bx, by): level shift, rows, columns, quantisation; out[zigzag position], q in zigzag order too.
// (The kernel runs the same two passes with one row / column per lane.)
JPEG_HD void forward_block(const Frame& f, const void* pixels, int comp, int bx, int by, const uint16_t* q, int16_t* out) {
    int ws[64];
    for (int r = 0; r < 8; ++r) {
        for (int c = 0; c < 8; ++c) ws[r * 8 + c] = component_sample(f, pixels, comp, by * 8 + r, bx * 8 + c) - 128;
        fdct8(ws + r * 8, true);
    }
    for (int c = 0; c < 8; ++c) {
        int v[8];
        for (int r = 0; r < 8; ++r) v[r] = ws[r * 8 + c];
        fdct8(v, false);
        for (int r = 0; r < 8; ++r) {
            const int z = zigzag_of_natural(r * 8 + c);
            out[z] = (int16_t)quantise(v[r], q[z]);
        }
    }
}

JPEG_HD int category(int v) {
    const unsigned a = (unsigned)(v < 0 ? -v : v);
    return a ? 32 - __builtin_clz(a) : 0;
}

// The symbols of one block, in order, through visit(slot, value bits, count of value bits): slot is the symbol's place in a class's
// TABLE_WORDS entries — the DC category 0 ... 11, or 16 + (run << 4 | size), 16 + ZRL, 16 + EOB.  zz: the coefficients in zigzag order
// (zz[0] is not read: diff is the DC difference).  A negative value sends the low bits of v - 1.  Counting (the statistics of the
// optimised mode) and coding both go through this walk, so they visit exactly the same symbols.
template <typename Visit>
JPEG_HD void walk_block(const int16_t* zz, int diff, Visit&& visit) {
    int s = category(diff);
    visit(s, (uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << s) - 1), s);
    int run = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll          // the coefficients stay in registers
#endif
    for (int k = 1; k < 64; ++k) {
        const int v = zz[k];
        if (v == 0) { ++run; continue; }
        for (; run > 15; run -= 16) visit(16 + ZRL, 0u, 0);
        s = category(v);
        visit(16 + (run << 4 | s), (uint32_t)(v < 0 ? v - 1 : v) & ((1u << s) - 1), s);
        run = 0;
    }
    if (run > 0) visit(16 + EOB, 0u, 0);
}

// A dummy block: difference 0, then the end-of-block.  It is coded, so it is counted.
template <typename Visit>
JPEG_HD void walk_dummy(Visit&& visit) {
    visit(0, 0u, 0);
    visit(16 + EOB, 0u, 0);
}

// The codes of one block, in order, through emit(bits, count): each call carries one Huffman code with the value bits behind it, at
// most 26 bits (16 + 10 for an AC symbol, 12 + 11 for a DC category of an optimised table).  table: the class's TABLE_WORDS entries
// code | length << 16.
template <typename Emit>
JPEG_HD void code_block(const int16_t* zz, int diff, const uint32_t* table, Emit&& emit) {
    walk_block(zz, diff, [&](int slot, uint32_t value, int s) {
        const uint32_t e = table[slot];
        emit(((e & 0xFFFFu) << s) | value, (int)(e >> 16) + s);
    });
}

template <typename Emit>
JPEG_HD void code_dummy(const uint32_t* table, Emit&& emit) {
    walk_dummy([&](int slot, uint32_t, int) { emit(table[slot] & 0xFFFFu, (int)(table[slot] >> 16)); });
}

// ---- optimised coding: the tables of ONE image from its own symbol statistics (libjpeg's optimize_coding) ----
//
// jpeg_gen_optimal_table (jchuff.c) restated.  The symbols in use (frequency > 0) are taken in symbol order, and a pseudo-symbol 256
// with frequency 1 is put behind them, which keeps the all-ones code unused.  The two least frequent entries are merged until one is
// left; among equal frequencies the LARGER symbol is taken first (so the pseudo-symbol wins every tie), the first of the two keeps the
// sum.  A symbol's code size is the number of merges its tree took part in; it can reach 32 and more.  The sizes above 16 are then
// brought down by libjpeg's adjustment of the COUNTS per length (from 32 down to 17: two symbols of length i leave, one goes to i - 1,
// and a symbol of the longest length j <= i - 2 in use becomes the prefix of two of length j + 1), and one count is taken from the
// longest length in use for the pseudo-symbol.  huffval lists the real symbols by their size BEFORE the adjustment, then by symbol
// value; canonical codes (Annex C) go to them in that order.  Pillow's bytes (libjpeg-turbo) are the arbiter of every detail here:
// tests/test_jpeg_enc_optimize_host.py holds the files and the DHT payloads to them, and where this text and Pillow ever disagree,
// Pillow is right.
//
// The routine is written once, over a `Par` that says how its four kinds of step run: one(f) — f() once; each(n, f) — f(i) for every
// i < n, in any order; compact(n, pred, put) — put(i, p) for every i < n with pred(i), p counting them in the order of i, and their
// number; min2(n, key, k1, k2) — the two smallest of the distinct keys key(i).  SerialPar runs them in order on one
// thread (thmr_jpeg_optimal_table, the host encode); the table kernel runs them on one wave (jpegenc.hip).  Neither changes a result.
constexpr int OPT_SYMBOLS = 257, OPT_MAX_CLEN = 32;
constexpr int32_t OPT_MERGED = 1000000001;                     // the frequency of an entry that was merged away: above every real sum
constexpr uint64_t OPT_NO_KEY = ~(uint64_t)0;
constexpr int64_t OPT_MAX_BLOCKS = (int64_t)1 << 23;           // 64 symbols a block at the most: every sum stays below 10^9, as libjpeg needs
constexpr int MAX_BLOCK_BITS_OPT = (12 + 11) + 63 * (16 + 10); // 12 DC symbols and the pseudo-symbol: a DC code can take 12 bits

struct OptimalWork {
    int32_t freq[OPT_SYMBOLS], root[OPT_SYMBOLS], codesize[OPT_SYMBOLS], sym[OPT_SYMBOLS];
};

// What a table kernel or a caller gets back: bits[0] is the longest code size BEFORE the limit (above 16: the adjustment ran), bits[1
// ... 16] the codes per length, huffval the nsym symbols in code order.  nsym < 0: a size above 32, which libjpeg refuses as well.
struct OptimalTable {
    uint8_t bits[17];
    uint8_t pad[3];
    int32_t nsym;
    uint8_t huffval[256];
};
static_assert(sizeof(OptimalTable) == 280, "the tables lie in an array, device and host");

struct SerialPar {
    template <typename F> void one(F&& f) { f(); }
    template <typename F> void each(int n, F&& f) { for (int i = 0; i < n; ++i) f(i); }
    template <typename Pred, typename Put> int compact(int n, Pred&& pred, Put&& put) {
        int p = 0;
        for (int i = 0; i < n; ++i)
            if (pred(i)) put(i, p++);
        return p;
    }
    template <typename Key> void min2(int n, Key&& key, uint64_t& k1, uint64_t& k2) {
        k1 = k2 = OPT_NO_KEY;
        for (int i = 0; i < n; ++i) {
            const uint64_t k = key(i);
            if (k < k1) { k2 = k1; k1 = k; } else if (k < k2) k2 = k;
        }
    }
};

// hist[0 ... nhist): the frequencies by symbol (nhist <= 256, none negative).  out is written inside one().
template <typename Par>
JPEG_HD void optimal_table(const int32_t* hist, int nhist, OptimalWork& w, Par& par, OptimalTable* out) {
    const int n = 1 + par.compact(nhist, [&](int i) { return hist[i] > 0; }, [&](int i, int p) { w.sym[p] = i; w.freq[p] = hist[i]; });
    par.each(n, [&](int i) {
        if (i == n - 1) { w.sym[i] = 256; w.freq[i] = 1; }
        w.root[i] = i; w.codesize[i] = 0;
    });
    for (;;) {
        // smaller frequency first, then the larger index; an entry merged away has no key
        uint64_t k1, k2;
        par.min2(n, [&](int i) { return w.freq[i] >= OPT_MERGED ? OPT_NO_KEY : ((uint64_t)w.freq[i] << 16) | (uint64_t)(0xFFFF - i); }, k1, k2);
        if (k2 == OPT_NO_KEY) break;
        const int c1 = 0xFFFF - (int)(k1 & 0xFFFF), c2 = 0xFFFF - (int)(k2 & 0xFFFF);
        const int32_t f2 = (int32_t)(k2 >> 16);         // c2's frequency, which its key carries
        par.each(n, [&](int i) {                // c1 keeps the sum, c2 leaves; every symbol of the two trees is one bit longer, the tree is c1's now
            if (i == c1) w.freq[i] += f2; else if (i == c2) w.freq[i] = OPT_MERGED;
            const int r = w.root[i];
            if (r == c1 || r == c2) { ++w.codesize[i]; w.root[i] = c1; }
        });
    }
    par.one([&]() {
        int cnt[OPT_MAX_CLEN + 1], pos[OPT_MAX_CLEN + 1];
        for (int i = 0; i <= OPT_MAX_CLEN; ++i) cnt[i] = 0;
        int longest = 0;
        bool over = false;
        for (int i = 0; i < n; ++i) {
            int cs = w.codesize[i];
            if (cs > OPT_MAX_CLEN) { over = true; cs = OPT_MAX_CLEN; w.codesize[i] = cs; }
            ++cnt[cs];
            if (cs > longest) longest = cs;
        }
        int p = 0;
        for (int i = 1; i <= OPT_MAX_CLEN; ++i) { pos[i] = p; p += cnt[i]; }
        for (int i = 0; i < 17; ++i) out->bits[i] = 0;
        out->pad[0] = out->pad[1] = out->pad[2] = 0;
        out->nsym = over ? -1 : n - 1;
        if (n < 2) return;                      // no symbol in use
        for (int i = OPT_MAX_CLEN; i > 16; --i)
            while (cnt[i] > 0) {
                int j = i - 2;
                while (cnt[j] == 0) --j;
                cnt[i] -= 2; ++cnt[i - 1]; cnt[j + 1] += 2; --cnt[j];
            }
        int top = 16;
        while (cnt[top] == 0) --top;
        --cnt[top];                             // the pseudo-symbol's code
        out->bits[0] = (uint8_t)longest;
        for (int i = 1; i <= 16; ++i) out->bits[i] = (uint8_t)cnt[i];
        for (int i = 0; i < n - 1; ++i) out->huffval[pos[w.codesize[i]]++] = (uint8_t)w.sym[i];
    });
}

// The canonical codes of one table into a class's TABLE_WORDS entries: slot = table + 0 (DC) or table + 16 (AC), zeroed before.  The
// codes of one length are consecutive, so symbol k of huffval takes (the first code of its length) + (k - the first position of its
// length); w is scratch.
template <typename Par>
JPEG_HD void code_words(const OptimalTable& t, OptimalWork& w, Par& par, uint32_t* slot) {
    par.one([&]() {
        uint32_t code = 0;
        int k = 0;
        for (int len = 1; len <= 16; ++len, code <<= 1) {
            w.root[len] = (int32_t)(code - (uint32_t)k);        // + k: the code at position k
            code += t.bits[len]; k += t.bits[len];
            w.codesize[len] = k;                                // the positions of this length end here
        }
    });
    par.each(t.nsym < 0 ? 0 : t.nsym, [&](int k) {
        int len = 1;
        while (w.codesize[len] <= k) ++len;
        slot[t.huffval[k]] = ((uint32_t)w.root[len] + (uint32_t)k) | (uint32_t)len << 16;
    });
}

}  // namespace jpegem
