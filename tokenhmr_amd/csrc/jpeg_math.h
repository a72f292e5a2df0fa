// The arithmetic of the JPEG decoder's second half, shared by the kernels (jpeg.hip) and the CPU decode (thmr_jpeg_decode_host): libjpeg's
// default pipeline restated in integers — the JDCT_ISLOW inverse DCT, h2v1 / h2v2 "fancy" upsampling, fixed-point YCbCr -> RGB.
// Compiles with or without HIP: JPEG_HD is __host__ __device__ under hipcc and nothing otherwise.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define JPEG_HD __host__ __device__ inline
#else
#define JPEG_HD inline
#endif

namespace jpegm {

// round(x * 2^13) of the decimals in the names
constexpr int CONST_BITS = 13, PASS1_BITS = 2;
constexpr int FIX_0_298631336 = 2446, FIX_0_390180644 = 3196, FIX_0_541196100 = 4433, FIX_0_765366865 = 6270, FIX_0_899976223 = 7373,
              FIX_1_175875602 = 9633, FIX_1_501321110 = 12299, FIX_1_847759065 = 15137, FIX_1_961570560 = 16069, FIX_2_053119869 = 16819,
              FIX_2_562915447 = 20995, FIX_3_072711026 = 25172;

// Products and sums wrap like the 32-bit registers of the SIMD implementations; unsigned arithmetic keeps a corrupt file's overflow defined.
JPEG_HD int mul(int a, int b) { return (int)((uint32_t)a * (uint32_t)b); }
JPEG_HD int add(int a, int b) { return (int)((uint32_t)a + (uint32_t)b); }
JPEG_HD int sub(int a, int b) { return (int)((uint32_t)a - (uint32_t)b); }
JPEG_HD int shl(int a, int n) { return (int)((uint32_t)a << n); }
JPEG_HD int descale(int x, int n) { return add(x, 1 << (n - 1)) >> n; }

// One 8-point pass of jpeg_idct_islow: v[0..7] in place, every output descaled by `shift` bits (pass 1: CONST_BITS - PASS1_BITS on the
// columns of the dequantised block; pass 2: CONST_BITS + PASS1_BITS + 3 on the rows of the workspace).  libjpeg's zero-AC shortcuts give
// the same values as this general form, so they are left out.
JPEG_HD void idct8(int* v, int shift) {
    int z2 = v[2], z3 = v[6];
    int z1 = mul(add(z2, z3), FIX_0_541196100);
    int tmp2 = add(z1, mul(z3, -FIX_1_847759065));
    int tmp3 = add(z1, mul(z2, FIX_0_765366865));
    z2 = v[0]; z3 = v[4];
    int tmp0 = shl(add(z2, z3), CONST_BITS);
    int tmp1 = shl(sub(z2, z3), CONST_BITS);
    const int tmp10 = add(tmp0, tmp3), tmp13 = sub(tmp0, tmp3), tmp11 = add(tmp1, tmp2), tmp12 = sub(tmp1, tmp2);
    tmp0 = v[7]; tmp1 = v[5]; tmp2 = v[3]; tmp3 = v[1];
    z1 = add(tmp0, tmp3); z2 = add(tmp1, tmp2); z3 = add(tmp0, tmp2);
    int z4 = add(tmp1, tmp3);
    const int z5 = mul(add(z3, z4), FIX_1_175875602);
    tmp0 = mul(tmp0, FIX_0_298631336); tmp1 = mul(tmp1, FIX_2_053119869);
    tmp2 = mul(tmp2, FIX_3_072711026); tmp3 = mul(tmp3, FIX_1_501321110);
    z1 = mul(z1, -FIX_0_899976223); z2 = mul(z2, -FIX_2_562915447);
    z3 = mul(z3, -FIX_1_961570560); z4 = mul(z4, -FIX_0_390180644);
    z3 = add(z3, z5); z4 = add(z4, z5);
    tmp0 = add(tmp0, add(z1, z3)); tmp1 = add(tmp1, add(z2, z4));
    tmp2 = add(tmp2, add(z2, z3)); tmp3 = add(tmp3, add(z1, z4));
    v[0] = descale(add(tmp10, tmp3), shift); v[7] = descale(sub(tmp10, tmp3), shift);
    v[1] = descale(add(tmp11, tmp2), shift); v[6] = descale(sub(tmp11, tmp2), shift);
    v[2] = descale(add(tmp12, tmp1), shift); v[5] = descale(sub(tmp12, tmp1), shift);
    v[3] = descale(add(tmp13, tmp0), shift); v[4] = descale(sub(tmp13, tmp0), shift);
}

// libjpeg's IDCT range limit: the +128 level shift and the clamp to 0..255, indexed with `x & 1023` as its table is (values more than
// 384 out of range wrap, which only a corrupt file produces).
JPEG_HD int range_limit_idct(int x) {
    const int v = x & 1023;
    return v < 128 ? v + 128 : v < 512 ? 255 : v < 896 ? 0 : v - 896;
}

JPEG_HD int clamp255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// A component plane as the IDCT wrote it: the block rectangle [bx0, bx0 + bw) x [by0, by0 + bh) of the component, 8 * bw bytes per row.
struct Plane {
    const uint8_t* p;
    int stride;     // bytes per row = 8 * bw
    int x0, y0;     // component sample coordinates of p[0] = 8 * bx0, 8 * by0
};
JPEG_HD int at(const Plane& pl, int y, int x) { return pl.p[(int64_t)(y - pl.y0) * pl.stride + (x - pl.x0)]; }

// The chroma sample libjpeg's upsampler puts at full-resolution pixel (x, y): hs, vs the luma sampling factors, cw x ch the TRUE
// downsampled component size ceil(W / hs) x ceil(H / vs).  Fancy (triangle) where cw > 2, replication otherwise (jdsample.c's choice).
//   h2v1  even x: (3 in[c] + in[c-1] + 1) >> 2, odd x: (3 in[c] + in[c+1] + 2) >> 2; column 0's left and column cw-1's right output = in[c]
//   h2v2  colsum[c] = 3 in[r][c] + in[r'][c], r' the row above for an even y and below for an odd one, replicated at rows 0 and ch-1;
//         even x: (3 this + last + 8) >> 4, odd x: (3 this + next + 7) >> 4; the two outer outputs (4 this + 8) >> 4 and (4 this + 7) >> 4
JPEG_HD int chroma_at(const Plane& pl, int hs, int vs, int cw, int ch, int x, int y) {
    if (hs == 1) return at(pl, y, x);
    const int c = x >> 1;
    if (vs == 1) {
        const int in = at(pl, y, c);
        if (cw <= 2) return in;
        if (!(x & 1)) return c == 0 ? in : (3 * in + at(pl, y, c - 1) + 1) >> 2;
        return c == cw - 1 ? in : (3 * in + at(pl, y, c + 1) + 2) >> 2;
    }
    const int r = y >> 1;
    if (cw <= 2) return at(pl, r, c);
    int r2 = (y & 1) ? r + 1 : r - 1;
    r2 = r2 < 0 ? 0 : r2 > ch - 1 ? ch - 1 : r2;
    const int cur = 3 * at(pl, r, c) + at(pl, r2, c);
    if (!(x & 1)) return c == 0 ? (cur * 4 + 8) >> 4 : (cur * 3 + 3 * at(pl, r, c - 1) + at(pl, r2, c - 1) + 8) >> 4;
    return c == cw - 1 ? (cur * 4 + 7) >> 4 : (cur * 3 + 3 * at(pl, r, c + 1) + at(pl, r2, c + 1) + 7) >> 4;
}

// jdcolor.c's tables as arithmetic: FIX(x) = round(x * 2^16), ONE_HALF = 2^15, arithmetic right shifts.
JPEG_HD void ycc_to_rgb(int y, int cb, int cr, int& r, int& g, int& b) {
    cb -= 128; cr -= 128;
    r = clamp255(y + ((91881 * cr + 32768) >> 16));
    g = clamp255(y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
    b = clamp255(y + ((116130 * cb + 32768) >> 16));
}

// One block: dequantise, columns, rows, range limit.  coef and quant in natural order; out[r * 8 + c].  (The kernel runs the same two
// passes with one column / row per lane.)
JPEG_HD void idct_block(const int16_t* coef, const uint16_t* quant, uint8_t* out) {
    int ws[64];
    for (int c = 0; c < 8; ++c) {
        int v[8];
        for (int r = 0; r < 8; ++r) v[r] = mul(coef[r * 8 + c], quant[r * 8 + c]);
        idct8(v, CONST_BITS - PASS1_BITS);
        for (int r = 0; r < 8; ++r) ws[r * 8 + c] = v[r];
    }
    for (int r = 0; r < 8; ++r) {
        idct8(ws + r * 8, CONST_BITS + PASS1_BITS + 3);
        for (int c = 0; c < 8; ++c) out[r * 8 + c] = (uint8_t)range_limit_idct(ws[r * 8 + c]);
    }
}

// The rectangle of component samples the window's pixels read, before clipping: luma (and un-subsampled chroma) the window itself,
// sub-sampled chroma the covered samples and one more on each side.
JPEG_HD void comp_sample_range(int lo, int n, int samp, int size, int& s0, int& s1) {
    if (samp == 1) { s0 = lo; s1 = lo + n - 1; return; }
    s0 = (lo >> 1) - 1; s1 = ((lo + n - 1) >> 1) + 1;
    if (s0 < 0) s0 = 0;
    if (s1 > size - 1) s1 = size - 1;
}

}  // namespace jpegm
