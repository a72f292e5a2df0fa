// A stand-alone CPU program over the host PNG decoder (tokenhmr_amd/csrc/pngdec_host.h, free of HIP), for a sanitizer build:
//
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/pngdec_sanitize.cpp -o pngdec_sanitize
//     ./pngdec_sanitize
//
// The files come from this project's own host encoder (png_host.h; both compression modes; grey, RGB, RGBA; the edge sizes of
// tests/test_png_dec_host.py) and are re-wrapped to reach what the encoder never writes: the zlib stream split over several IDAT chunks
// (a 1-byte one first), the same bytes declared as a palette image (256 and 100 entries), as grey + alpha, and as 16-bit samples.
// Every file, every prefix of it and every single-byte 0x00 / 0xFF corruption of its first 700 bytes — as it stands (the CRCs stop most)
// and with the chunk CRCs repaired, so that the damage reaches the inflate — goes through probe, the size-only call, inflate_window for
// three windows and the full decode, with the input, the row buffer and the output in heap buffers of EXACTLY the size the decoder is
// told: a read or a write one byte outside either is reported.  The raw zlib streams go through the inflate alone the same way.  A
// valid file must decode to the pixels it was written from.  Prints the number of inputs and a checksum; exits non-zero on a mismatch
// or a positive return code.
#include <stdio.h>
#include <stdlib.h>

#include "../tokenhmr_amd/csrc/pngdec_host.h"

static uint64_t g_inputs = 0, g_ok = 0, g_sum = 0;

static std::vector<uint8_t> chunk(const char* type, const uint8_t* body, size_t n) {
    std::vector<uint8_t> c(12 + n);
    pngh::put32(c.data(), (uint32_t)n);
    memcpy(c.data() + 4, type, 4);
    if (n) memcpy(c.data() + 8, body, n);
    pngh::put32(c.data() + 8 + n, pngh::crc32(c.data() + 4, 4 + n));
    return c;
}

// signature + IHDR + (PLTE) + the stream over `pieces` IDAT chunks (the first of one byte when there are several) + IEND
static std::vector<uint8_t> wrap(int w, int h, int depth, int ctype, int palette_entries, const uint8_t* z, size_t zn, int pieces) {
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    std::vector<uint8_t> f(sig, sig + 8);
    uint8_t hd[13];
    pngh::put32(hd, (uint32_t)w); pngh::put32(hd + 4, (uint32_t)h);
    hd[8] = (uint8_t)depth; hd[9] = (uint8_t)ctype; hd[10] = hd[11] = hd[12] = 0;
    auto add = [&](const std::vector<uint8_t>& c) { f.insert(f.end(), c.begin(), c.end()); };
    add(chunk("IHDR", hd, 13));
    add(chunk("gAMA", hd, 4));
    if (palette_entries) {
        std::vector<uint8_t> p((size_t)palette_entries * 3);
        for (size_t i = 0; i < p.size(); ++i) p[i] = (uint8_t)(i * 37 + 11);
        add(chunk("PLTE", p.data(), p.size()));
    }
    size_t at = 0;
    for (int k = 0; k < pieces; ++k) {
        size_t n = k == pieces - 1 ? zn - at : (k == 0 && pieces > 1) ? 1 : (zn - at) / (size_t)(pieces - k);
        if (n > zn - at) n = zn - at;
        add(chunk("IDAT", z + at, n));
        at += n;
    }
    add(chunk("IEND", nullptr, 0));
    return f;
}

// Every chunk's CRC recomputed over what the chunk now holds (as far as the chunk structure can still be walked).
static void repair_crcs(std::vector<uint8_t>& f) {
    size_t pos = 8;
    while (f.size() >= 12 && pos <= f.size() - 12) {
        const uint32_t n = pngdh::be32(f.data() + pos);
        if ((size_t)n > f.size() - pos - 12) break;
        pngh::put32(f.data() + pos + 8 + n, pngh::crc32(f.data() + pos + 4, 4 + (size_t)n));
        pos += 12 + (size_t)n;
    }
}

// One input through every host entry.  want: the (H, W, 3) B, G, R pixels a valid file must give, or null.  Returns the decode's status.
static int run(const uint8_t* file, size_t len, const uint8_t* want) {
    ++g_inputs;
    uint8_t* data = (uint8_t*)malloc(len ? len : 1);            // exactly len bytes
    if (len) memcpy(data, file, len);
    std::string err;
    pngdh::Header h;
    int rc = pngdh::parse(data, len, true, h, err);
    if (rc > 0) { fprintf(stderr, "probe returned %d\n", rc); exit(1); }
    if (rc == 0 && !h.unsupported) {
        const int32_t W = h.W, H = h.H;
        const int32_t wins[3][4] = {{0, 0, W, H}, {W / 3, H / 2, W - W / 3 - W / 4, H - H / 2 - H / 5}, {W / 2, H / 2, 0, 0}};
        for (const auto& win : wins) {
            pngdh::Plan plan;
            int64_t need = 0;
            rc = pngdh::inflate_window(data, len, win, nullptr, 0, plan, &need, err);
            if (rc > 0) { fprintf(stderr, "inflate_window returned %d\n", rc); exit(1); }
            if (rc == 0 && need > 0 && need < ((int64_t)1 << 28)) {
                uint8_t* rows = (uint8_t*)malloc((size_t)need);
                rc = pngdh::inflate_window(data, len, win, rows, need, plan, &need, err);
                if (rc > 0 || (rc == 0 && (plan.rows_inflated > win[1] + win[3] || plan.row0 > win[1] || plan.row0 + plan.rows_kept != win[1] + win[3]))) {
                    fprintf(stderr, "inflate_window: rc %d, an inconsistent plan\n", rc); exit(1);
                }
                if (rc == 0) for (int64_t i = 0; i < need; i += 97) g_sum = g_sum * 1099511628211ull + rows[i];
                free(rows);
            }
            if (win[2] > 0 && win[3] > 0 && (int64_t)win[2] * win[3] < ((int64_t)1 << 26)) {
                const size_t nout = (size_t)win[2] * (size_t)win[3] * 3;
                uint8_t* out = (uint8_t*)malloc(nout);
                rc = pngdh::decode(data, len, win, 1, out, (int64_t)win[2] * 3, err);
                if (rc > 0) { fprintf(stderr, "decode returned %d\n", rc); exit(1); }
                if (rc == 0) {
                    ++g_ok;
                    for (size_t i = 0; i < nout; i += 31) g_sum = g_sum * 1099511628211ull + out[i];
                    if (want)
                        for (int32_t y = 0; y < win[3]; ++y)
                            if (memcmp(out + (size_t)y * win[2] * 3, want + ((size_t)(win[1] + y) * W + win[0]) * 3, (size_t)win[2] * 3) != 0) {
                                fprintf(stderr, "a valid %d x %d file decodes to other pixels (window %d %d %d %d, row %d)\n", W, H, win[0], win[1], win[2], win[3], y);
                                exit(1);
                            }
                } else if (want) { fprintf(stderr, "a valid file is refused: %s\n", err.c_str()); exit(1); }
                free(out);
            }
        }
    } else if (want) { fprintf(stderr, "a valid file does not parse: %s\n", err.c_str()); exit(1); }
    free(data);
    return rc;
}

static void run_stream(const uint8_t* z, size_t len, size_t plain) {
    ++g_inputs;
    uint8_t* data = (uint8_t*)malloc(len ? len : 1);
    if (len) memcpy(data, z, len);
    uint8_t* out = (uint8_t*)malloc(plain ? plain : 1);
    int64_t written = 0;
    std::string err;
    const int rc = pngdh::inflate_buffer(data, len, out, (int64_t)plain, written, err);
    if (rc > 0 || written < 0 || written > (int64_t)plain) { fprintf(stderr, "inflate: rc %d, %lld bytes of %zu\n", rc, (long long)written, plain); exit(1); }
    if (rc == 0) { ++g_ok; for (int64_t i = 0; i < written; i += 13) g_sum = g_sum * 1099511628211ull + out[i]; }
    free(out); free(data);
}

static void corruptions(const std::vector<uint8_t>& f) {
    const size_t step = f.size() > 4000 ? 1 + f.size() / 1500 : 1;
    for (size_t cut = 0; cut < f.size(); cut += step) run(f.data(), cut, nullptr);
    for (size_t at = 0; at < f.size() && at < 700; ++at)
        for (int v : {0x00, 0xFF}) {
            if (f[at] == v) continue;
            std::vector<uint8_t> g = f;
            g[at] = (uint8_t)v;
            run(g.data(), g.size(), nullptr);
            if (at >= 8) { repair_crcs(g); run(g.data(), g.size(), nullptr); }
        }
}

int main() {
    const int sizes[][2] = {{1, 1}, {9, 1}, {1, 9}, {7, 5}, {30, 40}, {200, 150}};
    uint64_t seed = 0x9E3779B97F4A7C15ull;
    for (const auto& s : sizes)
        for (int c : {1, 3, 4})
            for (int kind = 0; kind < 2; ++kind)
                for (int compression : {THMR_PNG_FIXED, THMR_PNG_DYNAMIC}) {
                    const int w = s[0], h = s[1];
                    const size_t n = (size_t)w * h * c;
                    std::vector<uint8_t> px(n), want((size_t)w * h * 3);
                    for (size_t i = 0; i < n; ++i) {
                        seed = seed * 6364136223846793005ull + 1442695040888963407ull;
                        const size_t p = i / c;
                        px[i] = kind == 0 ? (uint8_t)(seed >> 56) : (uint8_t)(3 * (p / w) + 2 * (p % w) + 40 * (i % c) + ((seed >> 60) & 1));
                    }
                    for (size_t p = 0; p < (size_t)w * h; ++p)          // the file holds R, G, B(, A) = the buffer's order; the decode writes B, G, R
                        for (int k = 0; k < 3; ++k) want[p * 3 + k] = c == 1 ? px[p] : px[p * c + (2 - k)];
                    thmr_png_item it;
                    memset(&it, 0, sizeof(it));
                    it.pixels = px.data(); it.dtype = THMR_PNG_U8; it.width = w; it.height = h; it.channels = c;
                    it.stride_y = (int64_t)w * c; it.stride_x = c; it.stride_c = 1; it.compression = compression;
                    it.capacity = pngh::bound(w, h, c);
                    std::vector<uint8_t> file((size_t)it.capacity);
                    it.out = file.data();
                    std::string err;
                    if (pngh::check_item(it, err) != 0) { fprintf(stderr, "the encoder refuses: %s\n", err.c_str()); return 1; }
                    pngh::encode(it);
                    file.resize((size_t)it.written);
                    run(file.data(), file.size(), want.data());
                    const uint8_t* z = file.data() + pngh::IDAT_DATA_AT;
                    const size_t zn = (size_t)pngdh::be32(file.data() + 33);
                    const size_t plain = (size_t)h * (1 + (size_t)w * c);
                    std::vector<std::vector<uint8_t>> variants;
                    for (int pieces : {1, 2, 5}) variants.push_back(wrap(w, h, 8, c == 1 ? 0 : c == 3 ? 2 : 6, 0, z, zn, pieces));
                    for (const auto& v : variants) run(v.data(), v.size(), want.data());
                    if (c == 1) {
                        variants.push_back(wrap(w, h, 8, 3, 256, z, zn, 3));
                        variants.push_back(wrap(w, h, 8, 3, 100, z, zn, 1));          // noise holds indices beyond 100 entries: refused
                        if (w % 2 == 0) { variants.push_back(wrap(w / 2, h, 8, 4, 0, z, zn, 2)); variants.push_back(wrap(w / 2, h, 16, 0, 0, z, zn, 2)); }
                    }
                    if (c == 3 && w % 2 == 0) variants.push_back(wrap(w / 2, h, 16, 2, 0, z, zn, 2));
                    if (c == 4) {
                        variants.push_back(wrap(w, h, 16, 4, 0, z, zn, 3));
                        if (w % 2 == 0) variants.push_back(wrap(w / 2, h, 16, 6, 0, z, zn, 2));
                    }
                    for (size_t k = 3; k < variants.size(); ++k) run(variants[k].data(), variants[k].size(), nullptr);
                    if (w * h <= 1200)
                        for (const auto& v : variants) corruptions(v);
                    run_stream(z, zn, plain);
                    if (w * h <= 1200) {
                        for (size_t cut = 0; cut < zn; ++cut) run_stream(z, cut, plain);
                        for (size_t at = 0; at < zn && at < 700; ++at)
                            for (int v : {0x00, 0xFF, (int)(z[at] ^ (1u << (at % 8)))}) {
                                if (z[at] == v) continue;
                                std::vector<uint8_t> g(z, z + zn);
                                g[at] = (uint8_t)v;
                                run_stream(g.data(), zn, plain);
                                run_stream(g.data(), zn, plain / 2);
                            }
                    }
                }
    printf("%llu inputs, %llu decoded, checksum %016llx\n", (unsigned long long)g_inputs, (unsigned long long)g_ok, (unsigned long long)g_sum);
    return 0;
}
