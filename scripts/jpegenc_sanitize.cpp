// A stand-alone CPU program over the host JPEG encoder (tokenhmr_amd/csrc/jpegenc_host.h, free of HIP), for a sanitizer build:
//
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/jpegenc_sanitize.cpp -o jpegenc_sanitize
//     ./jpegenc_sanitize
//
// Every edge size of tests/test_jpeg_enc_host.py x {grey, 3, 4 channels} x {4:4:4, 4:2:0} x {q 1, 50, 100} x {noise, checkerboard, flat},
// uint8 and float32, with the pixels and the output in heap buffers of EXACTLY the size the encoder is told: a read or a write one byte
// outside either is reported.  Prints the number of files and a checksum of their bytes; exits non-zero where a file breaks its bound.
#include <stdio.h>
#include <stdlib.h>

#include "../tokenhmr_amd/csrc/jpegenc_host.h"

int main() {
    const int sizes[][2] = {{1, 1}, {7, 9}, {8, 8}, {16, 16}, {17, 23}, {24, 8}, {12, 20}, {33, 64}, {100, 75}, {2, 1}, {1, 17}, {31, 15}};
    const int channels[] = {1, 3, 4}, samplings[] = {THMR_JPEG_444, THMR_JPEG_420}, qualities[] = {1, 50, 100};
    uint64_t files = 0, sum = 0, seed = 0x9E3779B97F4A7C15ull;
    for (const auto& s : sizes)
        for (int c : channels)
            for (int sub : samplings)
                for (int q : qualities)
                    for (int kind = 0; kind < 3; ++kind)
                        for (int dtype : {THMR_PNG_U8, THMR_PNG_F32}) {
                            const int w = s[0], h = s[1];
                            const size_t n = (size_t)w * h * c;
                            uint8_t* u8 = dtype == THMR_PNG_U8 ? (uint8_t*)malloc(n) : nullptr;
                            float* f32 = dtype == THMR_PNG_F32 ? (float*)malloc(n * sizeof(float)) : nullptr;
                            for (size_t i = 0; i < n; ++i) {
                                seed = seed * 6364136223846793005ull + 1442695040888963407ull;
                                const size_t px = i / c;
                                const int v = kind == 0 ? (int)(seed >> 56) : kind == 1 ? (((px % w) + (px / w)) & 1 ? 255 : 0) : 200;
                                if (u8) u8[i] = (uint8_t)v; else f32[i] = (float)v / 255.0f;
                            }
                            thmr_png_item it;
                            memset(&it, 0, sizeof(it));
                            it.pixels = u8 ? (const void*)u8 : (const void*)f32;
                            it.dtype = dtype; it.width = w; it.height = h; it.channels = c;
                            it.stride_y = (int64_t)w * c; it.stride_x = c; it.stride_c = 1;
                            it.scale = 255.0f; it.rounding = kind == 0 ? THMR_PNG_ROUND_TRUNC : THMR_PNG_ROUND_NEAREST; it.swap_rb = kind & 1;
                            it.capacity = jpegeh::bound(w, h, c, sub);
                            it.out = (uint8_t*)malloc((size_t)it.capacity);
                            std::string err;
                            if (jpegeh::check_item(it, q, sub, err) != 0) { fprintf(stderr, "refused: %s\n", err.c_str()); return 1; }
                            jpegeh::encode(it, q, sub);
                            if (it.written < 4 || it.written > it.capacity || it.out[0] != 0xFF || it.out[1] != 0xD8 || it.out[it.written - 1] != 0xD9) {
                                fprintf(stderr, "%dx%dx%d sub %d q %d: %lld bytes of %lld\n", w, h, c, sub, q, (long long)it.written, (long long)it.capacity);
                                return 1;
                            }
                            for (int64_t i = 0; i < it.written; ++i) sum = sum * 1099511628211ull + it.out[i];
                            ++files;
                            free(it.out); free(u8); free(f32);
                        }
    printf("%llu files, checksum %016llx\n", (unsigned long long)files, (unsigned long long)sum);
    return 0;
}
