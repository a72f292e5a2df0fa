// A source image as the PNG and the JPEG encoder read it (png_math.h, jpegenc_math.h): where its samples lie, and the ONE conversion of
// a sample to the byte a file holds.  Shared by the kernels and the CPU encodes of both, so all four agree on every byte.  The one float
// product of the conversion has a single rounding.  Compiles with or without HIP: IMGSRC_HD is __host__ __device__ under hipcc and
// nothing otherwise.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define IMGSRC_HD __host__ __device__ inline
#else
#define IMGSRC_HD inline
#endif

namespace imgsrc {

// What an encoder needs of one image besides its pixels.
struct Image {
    int32_t dtype, w, h, c;
    int64_t sy, sx, sc;
    float scale;
    int32_t rounding, swap_rb;
};

IMGSRC_HD int row_bytes(const Image& im) { return im.w * im.c; }

// float -> byte.  rounding 0: nearest even, saturated; 1: clamped, then truncated.  NaN -> 0.
IMGSRC_HD uint8_t convert(float x, float scale, int rounding) {
    const float v = x * scale;
    if (!(v > 0.0f)) return 0;          // negatives, -0, NaN
    if (v >= 255.0f) return 255;
    return (uint8_t)(int)(rounding == 0 ? rintf(v) : v);
}

// Byte i of row y of the image as the file holds it (channel order swapped where asked).
IMGSRC_HD uint8_t sample(const Image& im, const void* pixels, int y, int i) {
    const int x = i / im.c;
    int ch = i - x * im.c;
    if (im.swap_rb && im.c >= 3 && ch < 3) ch = 2 - ch;
    const int64_t at = (int64_t)y * im.sy + (int64_t)x * im.sx + (int64_t)ch * im.sc;
    if (im.dtype == 0) return static_cast<const uint8_t*>(pixels)[at];
    return convert(static_cast<const float*>(pixels)[at], im.scale, im.rounding);
}

}  // namespace imgsrc
