// A stand-alone CPU program over the host JPEG encoder (tokenhmr_amd/csrc/jpegenc_host.h, free of HIP), for a sanitizer build:
//
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/jpegenc_sanitize.cpp -o jpegenc_sanitize
//     ./jpegenc_sanitize
//
// Every edge size of tests/test_jpeg_enc_host.py x {grey, 3, 4 channels} x {4:4:4, 4:2:0} x {q 1, 50, 100} x {noise, checkerboard, flat},
// uint8 and float32, each in the default mode and with THMR_JPEG_OPTIMIZE (the statistics, the table routine of
// thmr_jpeg_optimal_table, the image's own code words), with the pixels and the output in heap buffers of EXACTLY the size the encoder
// is told: a read or a write one byte outside either is reported.  Then the table routine alone on statistics that drive it to its
// ends: one symbol, all 256, frequencies whose unlimited code is far longer than 16 bits.  Prints the number of files and a checksum of
// their bytes; exits non-zero where a file breaks its bound or a table is no prefix code.
#include <stdio.h>
#include <stdlib.h>

#include "../tokenhmr_amd/csrc/jpegenc_host.h"

// The table of `freq` in heap buffers of exactly 17 and (symbols in use) bytes; false where it is no code for them.
static bool table_ok(const int32_t* freq) {
    jpegem::OptimalTable t;
    uint32_t* words = (uint32_t*)calloc(256, sizeof(uint32_t));
    jpegeh::optimal_table(freq, 256, t, words);
    int used = 0;
    for (int i = 0; i < 256; ++i) used += freq[i] > 0;
    if (t.nsym != used) { free(words); return false; }
    uint8_t* bits = (uint8_t*)malloc(17);
    uint8_t* vals = (uint8_t*)malloc((size_t)used);
    memcpy(bits, t.bits, 17);
    memcpy(vals, t.huffval, (size_t)used);
    uint64_t kraft = 0;         // in units of 2^-16, with the reserved all-ones code
    int total = 0, longest = 0;
    for (int len = 1; len <= 16; ++len) { kraft += (uint64_t)bits[len] << (16 - len); total += bits[len]; if (bits[len]) longest = len; }
    bool ok = total == used && longest > 0 && kraft + ((uint64_t)1 << (16 - longest)) <= 65536;
    for (int i = 0; i < used; ++i) ok = ok && freq[vals[i]] > 0;
    for (int i = 0; i < 256; ++i) ok = ok && ((words[i] != 0) == (freq[i] > 0));
    free(bits); free(vals); free(words);
    return ok;
}

int main() {
    const int sizes[][2] = {{1, 1}, {7, 9}, {8, 8}, {16, 16}, {17, 23}, {24, 8}, {12, 20}, {33, 64}, {100, 75}, {2, 1}, {1, 17}, {31, 15}};
    const int channels[] = {1, 3, 4}, samplings[] = {THMR_JPEG_444, THMR_JPEG_420}, qualities[] = {1, 50, 100};
    uint64_t files = 0, sum = 0, seed = 0x9E3779B97F4A7C15ull;
    for (const auto& s : sizes)
        for (int c : channels)
            for (int sub : samplings)
                for (int q : qualities)
                    for (int kind = 0; kind < 3; ++kind)
                        for (int dtype : {THMR_PNG_U8, THMR_PNG_F32})
                            for (int flags : {0, (int)THMR_JPEG_OPTIMIZE}) {
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
                            it.capacity = jpegeh::bound(w, h, c, sub, flags);
                            it.out = (uint8_t*)malloc((size_t)it.capacity);
                            std::string err;
                            if (jpegeh::check_item(it, q, sub, err, flags) != 0) { fprintf(stderr, "refused: %s\n", err.c_str()); return 1; }
                            if (jpegeh::encode(it, q, sub, flags, err) != 0) { fprintf(stderr, "failed: %s\n", err.c_str()); return 1; }
                            if (it.written < 4 || it.written > it.capacity || it.out[0] != 0xFF || it.out[1] != 0xD8 || it.out[it.written - 1] != 0xD9) {
                                fprintf(stderr, "%dx%dx%d sub %d q %d flags %d: %lld bytes of %lld\n", w, h, c, sub, q, flags, (long long)it.written, (long long)it.capacity);
                                return 1;
                            }
                            for (int64_t i = 0; i < it.written; ++i) sum = sum * 1099511628211ull + it.out[i];
                            ++files;
                            free(it.out); free(u8); free(f32);
                        }
    int32_t freq[256];
    int tables = 0;
    for (int kind = 0; kind < 6; ++kind)
        for (int round = 0; round < 8; ++round) {
            for (int i = 0; i < 256; ++i) {
                seed = seed * 6364136223846793005ull + 1442695040888963407ull;
                const int r = (int)(seed >> 40);
                freq[i] = kind == 0 ? (i == round * 31 ? 5 : 0)                                 // one symbol
                        : kind == 1 ? 1 + round                                                 // all 256, flat
                        : kind == 2 ? (i >= round && i < round + 25 ? 1 << (i - round) : 0)     // powers of two: a code 25 deep before the limit
                        : kind == 3 ? (r % 7 == 0 ? r % 100000 : 0)                             // sparse
                        : kind == 4 ? r % 3                                                     // many ties
                                    : (i < 200 ? 1 << (r % 20) : 0);                            // a long thin tail
            }
            if (kind == 4) freq[255] = 1;
            if (!table_ok(freq)) { fprintf(stderr, "table kind %d round %d is no code for its statistics\n", kind, round); return 1; }
            ++tables;
        }
    printf("%llu files, %d tables, checksum %016llx\n", (unsigned long long)files, tables, (unsigned long long)sum);
    return 0;
}
