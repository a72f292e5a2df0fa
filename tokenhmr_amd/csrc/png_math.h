// The arithmetic and the selection rules of the PNG encoder, shared by the kernels (png.hip) and the CPU encode (png_host.h): the
// five row filters and their cost, the candidate distances and the match rule of the LZ77 stage, and the fixed-Huffman
// token codes, and the dynamic-Huffman block of the opt-in mode (its rule stands above token_parts).  The pixels come through
// image_source.h.  Everything is integer, so both sides give the same bytes.  Compiles with or without HIP (PNG_HD is image_source.h's macro).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "image_source.h"

#define PNG_HD IMGSRC_HD

namespace pngm {

using imgsrc::Image;            // the source image and its pixel conversion: image_source.h, shared with the JPEG encoder
using imgsrc::row_bytes;
using imgsrc::sample;

constexpr int SEGMENT = 16384;          // bytes of the filtered stream per independently compressed segment (<= 32768: every distance is legal)
constexpr int PAD = 8;                  // readable bytes a segment buffer keeps past its end (the match loop compares 4 at a time)
constexpr int MIN_MATCH = 3, MAX_MATCH = 258;
constexpr int FAR = 4096;               // a match further back than this needs 4 bytes: 3 would cost more bits than 3 literals
constexpr int MAX_CAND = 8;
constexpr uint32_t ADLER_MOD = 65521;

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

// ---- dynamic-Huffman blocks (compression "dynamic") ----
// The block rule, one for the CPU encode and the kernels.  The tokens are the greedy chain above, whatever the mode.  Their literal /
// length and distance symbols are counted, plus one end-of-block; a distance alphabet with fewer than two symbols in use is padded to
// two with its lowest unused symbols at frequency 1 (what zlib does, so that the code is complete).  code_lengths gives each alphabet
// optimal lengths limited to 15 bits, assign_codes the canonical codes of RFC 1951 3.2.2.  The header trims HLIT (>= 257), HDIST (>= 1)
// and HCLEN (>= 4) to the last length in use; the HLIT + HDIST lengths, as ONE sequence, are run-length coded by rle_lengths, and
// the code-length alphabet gets lengths limited to 7 bits from the frequencies of that coding.  A segment is a dynamic block only if
// header + tokens + end-of-block take strictly fewer bits than the fixed block; the stored-block rule then applies to the winner.

constexpr int N_LL = 286, N_DIST = 30, N_CL = 19;
constexpr int MAX_BITS = 15, MAX_CL_BITS = 7;
constexpr int END_OF_BLOCK = 256;

// A token's symbols and extra bits, without any code: lsym the literal or the length symbol 257 ... 285; dsym -1 for a literal.
PNG_HD void token_parts(int lit, int len, int dist, int& lsym, int& e, int& extra, int& dsym, int& de, int& dextra) {
    e = 0; extra = 0; dsym = -1; de = 0; dextra = 0;
    if (len == 0) { lsym = lit; return; }
    const int l = len - 3;
    if (len == 258) lsym = 285;
    else if (l < 8) lsym = 257 + l;
    else { e = (31 - __builtin_clz((unsigned)l)) - 2; lsym = 261 + 4 * e + ((l >> e) & 3); extra = l & ((1 << e) - 1); }
    const int d = dist - 1;
    if (d < 4) dsym = d;
    else { de = (31 - __builtin_clz((unsigned)d)) - 1; dsym = 2 * de + 2 + ((d >> de) & 1); dextra = d & ((1 << de) - 1); }
}

PNG_HD int fixed_symbol_bits(int s) { return s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8; }
PNG_HD int length_extra_bits(int s) { return (s < 265 || s == 285) ? 0 : (s - 261) >> 2; }
PNG_HD int distance_extra_bits(int s) { return s < 4 ? 0 : (s >> 1) - 1; }

// Optimal prefix-code lengths of n symbols (n <= 286) with frequencies freq, none longer than max_bits; lens[s] = 0 where freq[s] <= 0.
// The symbols in use are ordered by frequency, the higher index first among equals; the in-place method of Moffat and Katajainen
// (1995) turns the ordered frequencies into the depths of a Huffman tree.  Where a depth exceeds max_bits the COUNTS of codes per
// length are repaired with zlib's step (gen_bitlen): every too deep leaf is lifted to max_bits, which takes the Kraft sum over 1 by
// a whole number of 2^-max_bits; each step moves a leaf of the deepest shorter length one level down and makes one leaf of max_bits
// its sibling there, which takes exactly 2^-max_bits off; as many steps as units bring the sum back to exactly 1.  The
// lengths are then dealt out along the order, the longest to the rarest: a more frequent symbol never gets the longer code, and of
// two equally frequent ones the lower index never does.  One symbol in use gets length 1.  a, b: scratch of n words each.  Returns
// the number of symbols in use.  Precondition: frequencies below 2^22, so that an index fits beside one in a word.
PNG_HD int code_lengths(const int32_t* freq, int n, int max_bits, int32_t* lens, int32_t* a, int32_t* b) {
    int m = 0;
    for (int s = 0; s < n; ++s) {
        lens[s] = 0;
        if (freq[s] > 0) b[m++] = (freq[s] << 9) | (511 - s);
    }
    if (m == 0) return 0;
    if (m == 1) { lens[511 - (b[0] & 511)] = 1; return 1; }
    const int gaps[6] = {132, 57, 23, 10, 4, 1};            // Shell sort, ascending: the keys are distinct
    for (int g = 0; g < 6; ++g) {
        const int gap = gaps[g];
        for (int i = gap; i < m; ++i) {
            const int32_t key = b[i];
            int j = i;
            for (; j >= gap && b[j - gap] > key; j -= gap) b[j] = b[j - gap];
            b[j] = key;
        }
    }
    for (int i = 0; i < m; ++i) a[i] = b[i] >> 9;
    // Moffat-Katajainen: a[] ascending weights -> parent indices -> internal depths -> leaf depths (non-increasing)
    a[0] += a[1];
    int root = 0, leaf = 2;
    for (int next = 1; next < m - 1; ++next) {
        if (leaf >= m || a[root] < a[leaf]) { a[next] = a[root]; a[root++] = next; } else a[next] = a[leaf++];
        if (leaf >= m || (root < next && a[root] < a[leaf])) { a[next] += a[root]; a[root++] = next; } else a[next] += a[leaf++];
    }
    a[m - 2] = 0;
    for (int next = m - 3; next >= 0; --next) a[next] = a[a[next]] + 1;
    int avail = 1, used = 0, depth = 0, next = m - 1;
    root = m - 2;
    while (avail > 0) {
        while (root >= 0 && a[root] == depth) { ++used; --root; }
        while (avail > used) { a[next--] = depth; --avail; }
        avail = 2 * used; ++depth; used = 0;
    }
    // codes per length, with the limit
    int count[32];
    for (int k = 0; k < 32; ++k) count[k] = 0;
    for (int i = 0; i < m; ++i) ++count[a[i] < max_bits ? a[i] : max_bits];
    int excess = -(1 << max_bits);                          // the Kraft sum over 1, in units of 2^-max_bits
    for (int k = 1; k <= max_bits; ++k) excess += count[k] << (max_bits - k);
    for (; excess > 0; --excess) {                          // one step takes exactly one unit off
        int bits = max_bits - 1;
        while (bits > 1 && count[bits] == 0) --bits;      // (there is one while the sum is over 1 and 2^max_bits >= m)
        --count[bits]; count[bits + 1] += 2; --count[max_bits];
    }
    int i = 0;
    for (int bits = max_bits; bits >= 1; --bits)
        for (int k = count[bits]; k > 0; --k) lens[511 - (b[i++] & 511)] = bits;
    return m;
}

// t[s] = the code length of symbol s  ->  t[s] = the canonical code, bit-reversed into stream order, | length << 16.
PNG_HD void assign_codes(int32_t* t, int n) {
    int count[MAX_BITS + 1], next[MAX_BITS + 2];
    for (int k = 0; k <= MAX_BITS; ++k) count[k] = 0;
    for (int s = 0; s < n; ++s) ++count[t[s]];
    count[0] = 0; next[0] = 0;
    for (int k = 1; k <= MAX_BITS; ++k) next[k] = (next[k - 1] + count[k - 1]) << 1;
    for (int s = 0; s < n; ++s) {
        const int len = t[s];
        if (len) t[s] = (int32_t)(reverse_bits((uint32_t)next[len]++, len) | ((uint32_t)len << 16));
    }
}

// Everything of one segment's dynamic block.  In: ll, d hold the token frequencies (the end-of-block not yet counted).  Out of
// dynamic_block: ll, d, cl hold code | length << 16; rle the run-length coding of the lengths, symbol | extra bits' value << 8.
struct DynBlock {
    int32_t ll[N_LL + 2], d[N_DIST + 2], cl[N_CL + 1];
    int32_t seq[N_LL + N_DIST + 4], dl[N_DIST + 2];        // the joined length sequence of the header; the distance (then the code-length) lengths
    int32_t a[N_LL + 2], b[N_LL + 2];                      // scratch of code_lengths
    uint16_t rle[N_LL + N_DIST + 4];
    int32_t nrle, hlit, hdist, hclen;
};

PNG_HD int cl_order(int k) {
    const uint8_t order[N_CL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    return order[k];
}
PNG_HD int cl_extra_bits(int s) { return s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0; }

// The greedy run-length coding of a sequence of n code lengths, one rule per position i with value v, r = the run of v from i on:
// v == 0 and r >= 3: symbol 17 (r <= 10) or 18, covering min(r, 138) zeros; v != 0, equal to the length before i and r >= 3:
// symbol 16 covering min(r, 6); else v itself.  out[k] = symbol | (repeat count - its base) << 8.  Returns the count of symbols.
PNG_HD int rle_lengths(const int32_t* seq, int n, uint16_t* out) {
    int k = 0;
    for (int i = 0; i < n;) {
        const int v = seq[i];
        int r = 1;
        while (i + r < n && seq[i + r] == v) ++r;
        if (v == 0 && r >= 3) {
            if (r > 138) r = 138;
            out[k++] = (uint16_t)(r <= 10 ? 17 | (r - 3) << 8 : 18 | (r - 11) << 8);
            i += r;
        } else if (v != 0 && i > 0 && seq[i - 1] == v && r >= 3) {
            if (r > 6) r = 6;
            out[k++] = (uint16_t)(16 | (r - 3) << 8);
            i += r;
        } else {
            out[k++] = (uint16_t)v;
            ++i;
        }
    }
    return k;
}

// Frequencies -> codes and header; returns the bits of the whole block, its 3-bit block header and the end-of-block included.
PNG_HD int64_t dynamic_block(DynBlock& k) {
    k.ll[END_OF_BLOCK] += 1;
    int used = 0, padded = 0, pad[2] = {0, 0};
    for (int s = 0; s < N_DIST; ++s) used += k.d[s] > 0;
    for (int s = 0; used < 2; ++s)
        if (k.d[s] == 0) { k.d[s] = 1; ++used; pad[padded++] = s; }
    code_lengths(k.ll, N_LL, MAX_BITS, k.seq, k.a, k.b);
    code_lengths(k.d, N_DIST, MAX_BITS, k.dl, k.a, k.b);
    int64_t bits = 3 + 5 + 5 + 4;
    for (int s = 0; s < N_LL; ++s) bits += (int64_t)k.ll[s] * (k.seq[s] + length_extra_bits(s));
    for (int s = 0; s < N_DIST; ++s) bits += (int64_t)k.d[s] * (k.dl[s] + distance_extra_bits(s));
    for (int i = 0; i < padded; ++i) bits -= k.dl[pad[i]];          // a padded leaf is never sent (it is symbol 0 or 1: no extra bits)
    k.hlit = N_LL;
    while (k.hlit > 257 && k.seq[k.hlit - 1] == 0) --k.hlit;
    k.hdist = N_DIST;
    while (k.hdist > 1 && k.dl[k.hdist - 1] == 0) --k.hdist;
    for (int s = 0; s < N_LL; ++s) k.ll[s] = k.seq[s];
    for (int s = 0; s < N_DIST; ++s) k.d[s] = k.dl[s];
    for (int s = 0; s < k.hdist; ++s) k.seq[k.hlit + s] = k.dl[s];
    k.nrle = rle_lengths(k.seq, k.hlit + k.hdist, k.rle);
    for (int s = 0; s < N_CL; ++s) k.cl[s] = 0;
    for (int i = 0; i < k.nrle; ++i) ++k.cl[k.rle[i] & 255];
    code_lengths(k.cl, N_CL, MAX_CL_BITS, k.dl, k.a, k.b);
    for (int s = 0; s < N_CL; ++s) bits += (int64_t)k.cl[s] * (k.dl[s] + cl_extra_bits(s));
    k.hclen = N_CL;
    while (k.hclen > 4 && k.dl[cl_order(k.hclen - 1)] == 0) --k.hclen;
    bits += 3 * k.hclen;
    for (int s = 0; s < N_CL; ++s) k.cl[s] = k.dl[s];
    assign_codes(k.ll, N_LL);
    assign_codes(k.d, N_DIST);
    assign_codes(k.cl, N_CL);
    return bits;
}

// The header goes out in 1 + hclen + nrle pieces of at most 17 bits: the block header with HLIT, HDIST and HCLEN; the lengths of the
// code-length code in the order of RFC 1951; the run-length coded lengths.
PNG_HD int header_pieces(const DynBlock& k) { return 1 + k.hclen + k.nrle; }
PNG_HD void header_piece(const DynBlock& k, int i, bool last, uint64_t& bits, int& n) {
    if (i == 0) {
        bits = (last ? 1u : 0u) | 4u | (uint32_t)(k.hlit - 257) << 3 | (uint32_t)(k.hdist - 1) << 8 | (uint32_t)(k.hclen - 4) << 13;     // BTYPE 10
        n = 17;
    } else if (i <= k.hclen) {
        bits = (uint32_t)k.cl[cl_order(i - 1)] >> 16;
        n = 3;
    } else {
        const uint32_t r = k.rle[i - 1 - k.hclen], c = (uint32_t)k.cl[r & 255];
        n = (int)(c >> 16);
        bits = (c & 0xFFFFu) | (uint64_t)(r >> 8) << n;
        n += cl_extra_bits((int)(r & 255));
    }
}

// One token in the block's own codes (token_bits is the same in the fixed ones); the end-of-block is ll[END_OF_BLOCK].
PNG_HD void dynamic_token_bits(const DynBlock& k, int lit, int len, int dist, uint64_t& bits, int& n) {
    int lsym, e, extra, dsym, de, dextra;
    token_parts(lit, len, dist, lsym, e, extra, dsym, de, dextra);
    uint32_t c = (uint32_t)k.ll[lsym];
    n = (int)(c >> 16);
    bits = (c & 0xFFFFu) | (uint64_t)extra << n; n += e;
    if (dsym < 0) return;
    c = (uint32_t)k.d[dsym];
    bits |= (uint64_t)(c & 0xFFFFu) << n; n += (int)(c >> 16);
    bits |= (uint64_t)dextra << n; n += de;
}

// The bits a token takes in the fixed code, from its symbols.
PNG_HD int fixed_token_bits(int lsym, int e, int dsym, int de) { return fixed_symbol_bits(lsym) + e + (dsym < 0 ? 0 : 5 + de); }

// How a segment ends, after the end-of-block code: bits of the trailer and the stream's byte length.
// coded bits so far (header + tokens) -> total bytes of the coded form, the sync marker of a non-final segment included.
PNG_HD int64_t coded_bytes(int64_t bits_before_eob, bool last, int eob_bits = 7) {
    int64_t bits = bits_before_eob + eob_bits;          // end of block: seven zero bits in the fixed code
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
