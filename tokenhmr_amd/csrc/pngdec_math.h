// The arithmetic of the PNG decoder, shared by the kernels (pngdec.hip) and the CPU decode (pngdec_host.h): the five reconstructions of
// the row filters and the conversion of one unfiltered pixel to the three output bytes.  Everything is integer, so both sides give the
// same bytes.  Compiles with or without HIP (PNG_HD is png_math.h's macro); pngm::paeth is the encoder's.
#pragma once
#include <stdint.h>

#include "png_math.h"

namespace pngdm {

constexpr int BAND_ROWS = 64;           // rows the un-filter kernel takes at once: one per lane of a wave (thmr_png_decode_band_rows)

// The byte a filter f residual x stands for, with left a, above b, above-left c (each 0 ... 255; zero outside the image, so in row 0
// Up is the identity, Avg a >> 1 and Paeth a).  The Avg sum has 9 bits; every result wraps mod 256.
PNG_HD uint8_t reconstruct(int f, int x, int a, int b, int c) {
    switch (f) {
        case 0: return (uint8_t)x;
        case 1: return (uint8_t)(x + a);
        case 2: return (uint8_t)(x + b);
        case 3: return (uint8_t)(x + ((a + b) >> 1));
        default: return (uint8_t)(x + pngm::paeth(a, b, c));
    }
}

// Bytes per pixel of a supported (colour type, bit depth) pair: 1, 2, 3, 4, 6 or 8; 0 for any other pair.
PNG_HD int bytes_per_pixel(int colour_type, int bit_depth) {
    if (bit_depth != 8 && !(bit_depth == 16 && colour_type != 3)) return 0;
    const int ch = colour_type == 0 ? 1 : colour_type == 2 ? 3 : colour_type == 3 ? 1 : colour_type == 4 ? 2 : colour_type == 6 ? 4 : 0;
    return ch * (bit_depth >> 3);
}

// One unfiltered pixel (px: its bpp bytes) -> three output bytes.  Grey is replicated, a palette index goes through `palette`
// (256 x 3, R G B, zero beyond the file's entries: the host refuses such an index before the device sees it), alpha is dropped and a
// 16-bit sample becomes its high byte, which is its first.
PNG_HD void to_bgr(int colour_type, int bit_depth, const uint8_t* px, const uint8_t* palette, int bgr, uint8_t* o) {
    const int s = bit_depth >> 3;
    int r, g, b;
    if (colour_type == 3) {
        const uint8_t* e = palette + 3 * px[0];
        r = e[0]; g = e[1]; b = e[2];
    } else if (colour_type == 0 || colour_type == 4) {
        r = g = b = px[0];
    } else {
        r = px[0]; g = px[s]; b = px[2 * s];
    }
    o[0] = (uint8_t)(bgr ? b : r); o[1] = (uint8_t)g; o[2] = (uint8_t)(bgr ? r : b);
}

}  // namespace pngdm
