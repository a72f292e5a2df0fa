// Mesh renderer: the GPU restatement of the reference's pyrender scenes (tokenhmr/lib/utils/renderer.py) —
// crop overlays and side views (B images, one mesh each) and the all-people frame (one image, N meshes) in one code path.
//
// Pipeline, all asynchronous on the caller's stream:
//   1. render_vertex_kernel    camera-frame transform p = R v + t (or R (v + t)), projection u = fx X/Z + cx, snap to 1/256 px
//   2. render_normal_kernel    angle-weighted smooth vertex normals, gathered through a vertex -> face CSR (no float atomics)
//   3. render_setup_kernel     cull (back face, degenerate, znear, off screen), per-face record (snapped corners, 1/Z plane),
//                              count the 16x16 tiles a small face's box touches; faces spanning > 4 tiles go to a per-image list
//   4. render_scan_kernel      exclusive scan of the tile counts (one workgroup)
//   5. render_fill_kernel      small faces into their tiles' bins
//   6. render_raster_kernel    one workgroup per (image, tile), one lane per pixel: exact integer coverage at 1 or 4 samples,
//                              nearest key (fp32 depth, mesh, face) per sample in registers, face records streamed through LDS;
//                              then shade once per (pixel, distinct winning face), resolve, 8-bit round, composite, store.
//
// Determinism: coverage is integer arithmetic; the per-sample winner is the minimum of a total order, so the bin order the
// atomics produce cannot change any pixel.  The only atomics are the bin counters and cursors.
//
// Compiled contract-off: the vertex transform and projection are fp32 operations in a fixed order, which the NumPy restatement
// (tests/render_numpy.py) repeats bit for bit — that is what makes its coverage (and alpha) exact.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <string>
#include <vector>

#include "handle_util.h"

#pragma clang fp contract(off)

namespace {

constexpr int TILE = 16;
constexpr int SMALL_TILES = 4;                 // faces whose pixel box spans more tiles than this go to the per-image list
constexpr float GUARD_PX = 2097152.f;          // 2^21 px: snapped coordinates stay below 2^29, edge products below 2^61
constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr float PI_F = 3.14159265358979f;

struct FaceRec {                               // 48 B; corners oriented so that the image-frame doubled area is positive
    int32_t x0, y0, x1, y1, x2, y2;            // snapped corners, 1/256 px
    float za, zb, zc;                          // 1/Z = za + zb (x - x0) + zc (y - y0), x / y in 1/256 px
    uint32_t id;                               // mesh * F + face, NONE = rejected
    int32_t bx, by;                            // pixel box: x0 | x1 << 16, y0 | y1 << 16
};

struct Light {
    int32_t type;
    float v[3], c[3];
};

struct Params {
    int32_t W, H, S, mode, tr_first, N, V, F, n_img, tiles_x, tiles_y, ch, has_colors, has_img;
    float fx, fy, cx, cy, znear;
    float R[9];
    float base[3], bg[3], amb[3], mean[3], stdv[3];
    float metallic, roughness;
    int32_t n_lights;
    Light L[THMR_RENDER_MAX_LIGHTS];
};

struct Scratch {                   // grow-only, sized exactly
    DevBuf<float> pos;             // (N, V, 3) camera frame
    DevBuf<int2> fix;              // (N, V) snapped u, v; x = INT_MIN: vertex unusable
    DevBuf<float> nrm;             // (N, V, 3)
    DevBuf<FaceRec> rec;           // (N, F)
    DevBuf<uint32_t> cnt;          // (T) tile counts, then (T + 1) offsets, (T) cursors, (n_img) large counts
    DevBuf<uint32_t> off;
    DevBuf<uint32_t> cur;
    DevBuf<uint32_t> lcnt;
    DevBuf<uint32_t> bins;         // (N F SMALL_TILES)
    DevBuf<uint32_t> large;        // (N F)
    DevBuf<float> colors;          // (N, 3)
};

thread_local ErrorSink<thmr_renderer> g_render_err;

__device__ __forceinline__ int64_t edge(int32_t ax, int32_t ay, int32_t bx, int32_t by, int32_t px, int32_t py) {
    return (int64_t)(bx - ax) * (int64_t)(py - ay) - (int64_t)(by - ay) * (int64_t)(px - ax);
}

// top-left rule in the image frame (x right, y down) for a positively oriented triangle: an edge a -> b owns the samples that
// lie exactly on it when it is a top edge (dy == 0, dx > 0) or a left edge (dy < 0)
__device__ __forceinline__ bool inside(int64_t e, int32_t dx, int32_t dy) {
    return e > 0 || (e == 0 && (dy < 0 || (dy == 0 && dx > 0)));
}

__global__ void render_vertex_kernel(Params p, const float* __restrict__ verts, const float* __restrict__ cam_t, float* __restrict__ pos,
                                     int2* __restrict__ fix) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)p.N * p.V) return;
    const int m = (int)(i / p.V);
    float x = verts[i * 3], y = verts[i * 3 + 1], z = verts[i * 3 + 2];
    const float tx = cam_t[m * 3], ty = cam_t[m * 3 + 1], tz = cam_t[m * 3 + 2];
    if (p.tr_first) { x = x + tx; y = y + ty; z = z + tz; }
    float X = p.R[0] * x + p.R[1] * y + p.R[2] * z;
    float Y = p.R[3] * x + p.R[4] * y + p.R[5] * z;
    float Z = p.R[6] * x + p.R[7] * y + p.R[8] * z;
    if (!p.tr_first) { X = X + tx; Y = Y + ty; Z = Z + tz; }
    pos[i * 3] = X; pos[i * 3 + 1] = Y; pos[i * 3 + 2] = Z;
    const float u = X / Z * p.fx + p.cx, v = Y / Z * p.fy + p.cy;
    int2 f = make_int2(INT_MIN, INT_MIN);
    if (Z >= p.znear && fabsf(u) <= GUARD_PX && fabsf(v) <= GUARD_PX)       // false for NaN as well
        f = make_int2((int)rintf(u * 256.f), (int)rintf(v * 256.f));
    fix[i] = f;
}

__global__ void render_normal_kernel(Params p, const int32_t* __restrict__ faces, const int32_t* __restrict__ csr_off,
                                     const int32_t* __restrict__ csr, const float* __restrict__ pos, float* __restrict__ nrm) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)p.N * p.V) return;
    const int m = (int)(i / p.V), v = (int)(i - (int64_t)m * p.V);
    const float* P = pos + (int64_t)m * p.V * 3;
    float nx = 0.f, ny = 0.f, nz = 0.f;
    for (int k = csr_off[v]; k < csr_off[v + 1]; ++k) {
        const int f = csr[k] >> 2, c = csr[k] & 3;
        const int32_t* fv = faces + (int64_t)f * 3;
        const float* a = P + (int64_t)fv[0] * 3;
        const float* b = P + (int64_t)fv[1] * 3;
        const float* d = P + (int64_t)fv[2] * 3;
        const float e1x = b[0] - a[0], e1y = b[1] - a[1], e1z = b[2] - a[2];
        const float e2x = d[0] - a[0], e2y = d[1] - a[1], e2z = d[2] - a[2];
        float fnx = e1y * e2z - e1z * e2y, fny = e1z * e2x - e1x * e2z, fnz = e1x * e2y - e1y * e2x;
        const float fl = sqrtf(fnx * fnx + fny * fny + fnz * fnz);
        if (!(fl > 0.f) || !isfinite(fl)) continue;                  // degenerate face: no normal, no weight
        fnx = fnx / fl; fny = fny / fl; fnz = fnz / fl;
        const float* o = P + (int64_t)fv[c] * 3;                      // interior angle at this corner
        const float* q = P + (int64_t)fv[(c + 1) % 3] * 3;
        const float* r = P + (int64_t)fv[(c + 2) % 3] * 3;
        const float ax = q[0] - o[0], ay = q[1] - o[1], az = q[2] - o[2];
        const float bx = r[0] - o[0], by = r[1] - o[1], bz = r[2] - o[2];
        const float la = sqrtf(ax * ax + ay * ay + az * az), lb = sqrtf(bx * bx + by * by + bz * bz);
        if (!(la > 0.f) || !(lb > 0.f)) continue;
        const float cs = fminf(fmaxf((ax * bx + ay * by + az * bz) / (la * lb), -1.f), 1.f);
        const float w = acosf(cs);
        nx = nx + w * fnx; ny = ny + w * fny; nz = nz + w * fnz;
    }
    const float l = sqrtf(nx * nx + ny * ny + nz * nz);
    if (l > 0.f) { nx = nx / l; ny = ny / l; nz = nz / l; }
    nrm[i * 3] = nx; nrm[i * 3 + 1] = ny; nrm[i * 3 + 2] = nz;
}

__device__ __forceinline__ void face_tiles(const FaceRec& r, int& tx0, int& tx1, int& ty0, int& ty1) {
    tx0 = (r.bx & 0xFFFF) / TILE; tx1 = (r.bx >> 16) / TILE;
    ty0 = (r.by & 0xFFFF) / TILE; ty1 = (r.by >> 16) / TILE;
}

__global__ void render_setup_kernel(Params p, const int32_t* __restrict__ faces, const float* __restrict__ pos, const int2* __restrict__ fix,
                                    FaceRec* __restrict__ rec, uint32_t* __restrict__ cnt, uint32_t* __restrict__ lcnt,
                                    uint32_t* __restrict__ large) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)p.N * p.F) return;
    const int m = (int)(i / p.F), f = (int)(i - (int64_t)m * p.F);
    FaceRec r;
    r.id = NONE; r.bx = r.by = 0;
    r.x0 = r.y0 = r.x1 = r.y1 = r.x2 = r.y2 = 0; r.za = r.zb = r.zc = 0.f;
    const int32_t* fv = faces + (int64_t)f * 3;
    const int64_t base = (int64_t)m * p.V;
    int2 a = fix[base + fv[0]], b = fix[base + fv[1]], c = fix[base + fv[2]];
    double Za = pos[(base + fv[0]) * 3 + 2], Zb = pos[(base + fv[1]) * 3 + 2], Zc = pos[(base + fv[2]) * 3 + 2];
    // an unusable corner (INT_MIN marker) rejects the face before any arithmetic on it: the marker's differences overflow int32
    const bool usable = a.x != INT_MIN && b.x != INT_MIN && c.x != INT_MIN;
    // front faces are counter-clockwise in GL window coordinates (y up), i.e. negative doubled area in the image frame
    if (usable && edge(a.x, a.y, b.x, b.y, c.x, c.y) < 0) {
        { int2 t = b; b = c; c = t; double tz = Zb; Zb = Zc; Zc = tz; }   // orient positively
        const int px0 = min(a.x, min(b.x, c.x)) >> 8, px1 = max(a.x, max(b.x, c.x)) >> 8;
        const int py0 = min(a.y, min(b.y, c.y)) >> 8, py1 = max(a.y, max(b.y, c.y)) >> 8;
        if (px1 >= 0 && py1 >= 0 && px0 < p.W && py0 < p.H) {
            r.x0 = a.x; r.y0 = a.y; r.x1 = b.x; r.y1 = b.y; r.x2 = c.x; r.y2 = c.y;
            r.bx = max(px0, 0) | (min(px1, p.W - 1) << 16);
            r.by = max(py0, 0) | (min(py1, p.H - 1) << 16);
            // 1/Z plane over the snapped corners, in double, relative to corner 0
            const double i0 = 1.0 / Za, i1 = 1.0 / Zb, i2 = 1.0 / Zc;
            const double d1x = (double)(b.x - a.x), d1y = (double)(b.y - a.y), d2x = (double)(c.x - a.x), d2y = (double)(c.y - a.y);
            const double det = d1x * d2y - d2x * d1y;
            r.za = (float)i0;
            r.zb = (float)(((i1 - i0) * d2y - (i2 - i0) * d1y) / det);
            r.zc = (float)(((i2 - i0) * d1x - (i1 - i0) * d2x) / det);
            r.id = (uint32_t)i;
            const int img = p.mode ? 0 : m;
            int tx0, tx1, ty0, ty1;
            face_tiles(r, tx0, tx1, ty0, ty1);
            if ((tx1 - tx0 + 1) * (ty1 - ty0 + 1) <= SMALL_TILES) {
                for (int ty = ty0; ty <= ty1; ++ty)
                    for (int tx = tx0; tx <= tx1; ++tx)
                        atomicAdd(&cnt[((int64_t)img * p.tiles_y + ty) * p.tiles_x + tx], 1u);
            } else {
                const int64_t cap = p.mode ? (int64_t)p.N * p.F : p.F;
                const uint32_t slot = atomicAdd(&lcnt[img], 1u);
                large[img * cap + slot] = (uint32_t)i;
            }
        }
    }
    rec[i] = r;
}

__global__ void __launch_bounds__(1024) render_scan_kernel(const uint32_t* __restrict__ cnt, uint32_t* __restrict__ off,
                                                           uint32_t* __restrict__ cur, int64_t T) {
    __shared__ uint32_t part[1024];
    const int t = threadIdx.x;
    const int64_t chunk = (T + 1023) / 1024, lo = min<int64_t>(T, t * chunk), hi = min<int64_t>(T, lo + chunk);
    uint32_t s = 0;
    for (int64_t k = lo; k < hi; ++k) s += cnt[k];
    part[t] = s;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {                             // Hillis-Steele inclusive scan of the 1024 chunk sums
        const uint32_t v = t >= d ? part[t - d] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint32_t run = part[t] - s;
    for (int64_t k = lo; k < hi; ++k) { off[k] = run; cur[k] = run; run += cnt[k]; }
    if (t == 1023) off[T] = part[1023];
}

__global__ void render_fill_kernel(Params p, const FaceRec* __restrict__ rec, uint32_t* __restrict__ cur, uint32_t* __restrict__ bins) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)p.N * p.F) return;
    const FaceRec r = rec[i];
    if (r.id == NONE) return;
    int tx0, tx1, ty0, ty1;
    face_tiles(r, tx0, tx1, ty0, ty1);
    if ((tx1 - tx0 + 1) * (ty1 - ty0 + 1) > SMALL_TILES) return;
    const int img = p.mode ? 0 : (int)(i / p.F);
    for (int ty = ty0; ty <= ty1; ++ty)
        for (int tx = tx0; tx <= tx1; ++tx) {
            const uint32_t slot = atomicAdd(&cur[((int64_t)img * p.tiles_y + ty) * p.tiles_x + tx], 1u);
            bins[slot] = (uint32_t)i;
        }
}

__device__ __forceinline__ float3 shade(const Params& p, uint32_t id, int px, int py, const int32_t* __restrict__ faces,
                                        const float* __restrict__ pos, const int2* __restrict__ fix, const float* __restrict__ nrm,
                                        const float* __restrict__ colors) {
    const int m = (int)(id / (uint32_t)p.F), f = (int)(id - (uint32_t)m * (uint32_t)p.F);
    const int32_t* fv = faces + (int64_t)f * 3;
    const int64_t base = (int64_t)m * p.V;
    const int2 a = fix[base + fv[0]], b = fix[base + fv[1]], c = fix[base + fv[2]];
    // screen-space barycentrics at the pixel centre (may lie outside the face: no centroid sampling, as in GL), then
    // perspective-correct weights
    const int32_t sx = px * 256 + 128, sy = py * 256 + 128;
    const double area = (double)edge(a.x, a.y, b.x, b.y, c.x, c.y);
    const double l0 = (double)edge(b.x, b.y, c.x, c.y, sx, sy) / area, l1 = (double)edge(c.x, c.y, a.x, a.y, sx, sy) / area;
    const double l2 = 1.0 - l0 - l1;
    const float* P0 = pos + (base + fv[0]) * 3;
    const float* P1 = pos + (base + fv[1]) * 3;
    const float* P2 = pos + (base + fv[2]) * 3;
    double w0 = l0 / P0[2], w1 = l1 / P1[2], w2 = l2 / P2[2];
    const double ws = w0 + w1 + w2;
    w0 /= ws; w1 /= ws; w2 /= ws;
    const float* N0 = nrm + (base + fv[0]) * 3;
    const float* N1 = nrm + (base + fv[1]) * 3;
    const float* N2 = nrm + (base + fv[2]) * 3;
    float P[3], N[3];
    for (int k = 0; k < 3; ++k) {
        P[k] = (float)(w0 * P0[k] + w1 * P1[k] + w2 * P2[k]);
        N[k] = (float)(w0 * N0[k] + w1 * N1[k] + w2 * N2[k]);
    }
    float nl = sqrtf(N[0] * N[0] + N[1] * N[1] + N[2] * N[2]);
    nl = nl > 0.f ? nl : 1.f;
    N[0] /= nl; N[1] /= nl; N[2] /= nl;
    float V[3] = {-P[0], -P[1], -P[2]};
    float vl = sqrtf(V[0] * V[0] + V[1] * V[1] + V[2] * V[2]);
    vl = vl > 0.f ? vl : 1.f;
    V[0] /= vl; V[1] /= vl; V[2] /= vl;
    float base_c[3];
    for (int k = 0; k < 3; ++k) base_c[k] = p.has_colors ? colors[m * 3 + k] : p.base[k];
    // glTF metallic-roughness (pyrender's mesh shader, restated — DESIGN.md §3.6)
    const float met = p.metallic, alpha = p.roughness * p.roughness, a2 = alpha * alpha;
    float cdiff[3], f0[3];
    for (int k = 0; k < 3; ++k) {
        cdiff[k] = base_c[k] * (1.f - 0.04f) * (1.f - met);
        f0[k] = 0.04f * (1.f - met) + base_c[k] * met;
    }
    const float f90 = fminf(fmaxf(fmaxf(f0[0], fmaxf(f0[1], f0[2])) * 25.f, 0.f), 1.f);
    const float ndv = fminf(fmaxf(fabsf(N[0] * V[0] + N[1] * V[1] + N[2] * V[2]), 0.001f), 1.f);
    float col[3] = {p.amb[0] * base_c[0], p.amb[1] * base_c[1], p.amb[2] * base_c[2]};
    for (int li = 0; li < p.n_lights; ++li) {
        const Light& L = p.L[li];
        float l[3], att = 1.f;
        if (L.type == 0) {
            l[0] = -L.v[0]; l[1] = -L.v[1]; l[2] = -L.v[2];
        } else {
            l[0] = L.v[0] - P[0]; l[1] = L.v[1] - P[1]; l[2] = L.v[2] - P[2];
            const float d2 = l[0] * l[0] + l[1] * l[1] + l[2] * l[2];
            att = 1.f / d2;
        }
        const float ll = sqrtf(l[0] * l[0] + l[1] * l[1] + l[2] * l[2]);
        if (!(ll > 0.f)) continue;
        l[0] /= ll; l[1] /= ll; l[2] /= ll;
        float h[3] = {l[0] + V[0], l[1] + V[1], l[2] + V[2]};
        float hl = sqrtf(h[0] * h[0] + h[1] * h[1] + h[2] * h[2]);
        hl = hl > 0.f ? hl : 1.f;
        h[0] /= hl; h[1] /= hl; h[2] /= hl;
        const float ndl = fminf(fmaxf(N[0] * l[0] + N[1] * l[1] + N[2] * l[2], 0.001f), 1.f);
        const float ndh = fminf(fmaxf(N[0] * h[0] + N[1] * h[1] + N[2] * h[2], 0.f), 1.f);
        const float vdh = fminf(fmaxf(V[0] * h[0] + V[1] * h[1] + V[2] * h[2], 0.f), 1.f);
        const float fs = powf(1.f - vdh, 5.f);
        const float G = (2.f * ndl / (ndl + sqrtf(a2 + (1.f - a2) * ndl * ndl))) * (2.f * ndv / (ndv + sqrtf(a2 + (1.f - a2) * ndv * ndv)));
        const float dd = ndh * ndh * (a2 - 1.f) + 1.f;
        const float D = a2 / (PI_F * dd * dd);
        for (int k = 0; k < 3; ++k) {
            const float F = f0[k] + (f90 - f0[k]) * fs;
            const float diff = (1.f - F) * cdiff[k] / PI_F;
            const float spec = F * G * D / (4.f * ndl * ndv);
            col[k] += att * L.c[k] * ndl * (diff + spec);
        }
    }
    float3 o;
    o.x = fminf(fmaxf(powf(fmaxf(col[0], 0.f), 1.f / 2.2f), 0.f), 1.f);
    o.y = fminf(fmaxf(powf(fmaxf(col[1], 0.f), 1.f / 2.2f), 0.f), 1.f);
    o.z = fminf(fmaxf(powf(fmaxf(col[2], 0.f), 1.f / 2.2f), 0.f), 1.f);
    return o;
}

__device__ __forceinline__ float to8(float v) { return rintf(fminf(fmaxf(v, 0.f), 1.f) * 255.f) / 255.0f; }

template <int S>
__global__ void __launch_bounds__(256) render_raster_kernel(Params p, const int32_t* __restrict__ faces, const float* __restrict__ pos,
                                                            const int2* __restrict__ fix, const float* __restrict__ nrm,
                                                            const float* __restrict__ colors, const FaceRec* __restrict__ rec,
                                                            const uint32_t* __restrict__ off, const uint32_t* __restrict__ bins,
                                                            const uint32_t* __restrict__ lcnt, const uint32_t* __restrict__ large,
                                                            const float* __restrict__ img_in, float* __restrict__ out,
                                                            uint32_t* __restrict__ ids_out) {
    __shared__ FaceRec lds[256];
    const int lane = threadIdx.x, img = blockIdx.y;
    const int tile = blockIdx.x, tx = tile % p.tiles_x, ty = tile / p.tiles_x;
    const int px = tx * TILE + (lane & 15), py = ty * TILE + (lane >> 4);
    // the standard 4x rotated-grid positions in 1/256 px; one sample = the pixel centre
    const int ox[4] = {96, 224, 32, 160}, oy[4] = {32, 96, 160, 224};
    int32_t sxs[S], sys[S];
    uint32_t bz[S], bid[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        sxs[s] = px * 256 + (S == 1 ? 128 : ox[s]);
        sys[s] = py * 256 + (S == 1 ? 128 : oy[s]);
        bz[s] = NONE; bid[s] = NONE;
    }
    const int64_t t = ((int64_t)img * p.tiles_y + ty) * p.tiles_x + tx;
    const int64_t lcap = p.mode ? (int64_t)p.N * p.F : p.F;
    for (int list = 0; list < 2; ++list) {
        const uint32_t* ids = list == 0 ? bins + off[t] : large + img * lcap;
        const uint32_t n = list == 0 ? off[t + 1] - off[t] : lcnt[img];
        for (uint32_t b0 = 0; b0 < n; b0 += 256) {
            if (b0 + lane < n) lds[lane] = rec[ids[b0 + lane]];
            __syncthreads();
            const uint32_t cnt = min(256u, n - b0);
            for (uint32_t k = 0; k < cnt; ++k) {
                const FaceRec& r = lds[k];
                if (px < (r.bx & 0xFFFF) || px > (r.bx >> 16) || py < (r.by & 0xFFFF) || py > (r.by >> 16)) continue;
#pragma unroll
                for (int s = 0; s < S; ++s) {
                    const int32_t sx = sxs[s], sy = sys[s];
                    if (!inside(edge(r.x1, r.y1, r.x2, r.y2, sx, sy), r.x2 - r.x1, r.y2 - r.y1)) continue;
                    if (!inside(edge(r.x2, r.y2, r.x0, r.y0, sx, sy), r.x0 - r.x2, r.y0 - r.y2)) continue;
                    if (!inside(edge(r.x0, r.y0, r.x1, r.y1, sx, sy), r.x1 - r.x0, r.y1 - r.y0)) continue;
                    const float iz = r.za + r.zb * (float)(sx - r.x0) + r.zc * (float)(sy - r.y0);
                    const uint32_t z = iz > 0.f ? __float_as_uint(1.f / iz) : 0x7F800000u;
                    if (z < bz[s] || (z == bz[s] && r.id < bid[s])) { bz[s] = z; bid[s] = r.id; }
                }
            }
            __syncthreads();
        }
    }
    if (px >= p.W || py >= p.H) return;
    // resolve: shade once per distinct winning face (MSAA), average with the background over the uncovered samples
    float sum[3] = {0.f, 0.f, 0.f};
    int k = 0;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        if (bid[s] == NONE) continue;
        ++k;
        bool seen = false;
#pragma unroll
        for (int q = 0; q < s; ++q) seen = seen || bid[q] == bid[s];
        if (seen) continue;
        int mult = 0;
#pragma unroll
        for (int q = s; q < S; ++q) mult += bid[q] == bid[s];
        const float3 c = shade(p, bid[s], px, py, faces, pos, fix, nrm, colors);
        sum[0] += (float)mult * c.x; sum[1] += (float)mult * c.y; sum[2] += (float)mult * c.z;
    }
    const float unc = (float)(S - k), inv = 1.f / (float)S;
    float rgb[3];
    for (int c = 0; c < 3; ++c) rgb[c] = to8((sum[c] + unc * p.bg[c]) * inv);
    const float a = to8((float)k * inv);
    const int64_t pix = ((int64_t)img * p.H + py) * p.W + px;
    float* o = out + pix * p.ch;
    if (p.has_img) {                       // Renderer.__call__: color * valid_mask + (1 - valid_mask) * image, in fp32
        const int64_t plane = (int64_t)p.H * p.W;
        const float* src = img_in + (int64_t)img * 3 * plane + (int64_t)py * p.W + px;
        for (int c = 0; c < 3; ++c) {
            const float im = src[c * plane] * p.stdv[c] + p.mean[c];
            o[c] = rgb[c] * a + (1.f - a) * im;
        }
    } else {
        for (int c = 0; c < 3; ++c) o[c] = rgb[c];
        if (p.ch == 4) o[3] = a;
    }
    if (ids_out)
#pragma unroll
        for (int s = 0; s < S; ++s) ids_out[pix * S + s] = bid[s];
}

}  // namespace

struct thmr_renderer {
    int device = 0;
    int32_t F = 0, V = 0;
    DevBuf<int32_t> faces;         // (F, 3) device
    DevBuf<int32_t> csr_off;       // (V + 1)
    DevBuf<int32_t> csr;           // (3F) face << 2 | corner, by vertex, face-ascending
    Scratch s;
    std::string err;
};

extern "C" {

const char* thmr_renderer_last_error(const thmr_renderer* r) { return g_render_err.read(r); }

int thmr_renderer_create(int32_t device, const int32_t* faces_host, int32_t F, int32_t V, thmr_renderer** out) {
    if (!out) return g_render_err.invalid(nullptr, "null out");
    *out = nullptr;
    if (!faces_host) return g_render_err.invalid(nullptr, "null faces");
    if (F <= 0 || V <= 0 || V > (1 << 28) || F > (1 << 28)) return g_render_err.invalid(nullptr, "bad face / vertex count");
    std::vector<int32_t> cnt((size_t)V + 1, 0);
    for (int64_t k = 0; k < (int64_t)F * 3; ++k) {
        const int32_t v = faces_host[k];
        if (v < 0 || v >= V) return g_render_err.invalid(nullptr, "face " + std::to_string(k / 3) + " indexes vertex " + std::to_string(v) +
                                                            " outside [0, " + std::to_string(V) + ")");
        ++cnt[v + 1];
    }
    for (int32_t v = 0; v < V; ++v) cnt[v + 1] += cnt[v];
    std::vector<int32_t> csr((size_t)F * 3), fill(cnt.begin(), cnt.end() - 1);
    for (int32_t f = 0; f < F; ++f)
        for (int c = 0; c < 3; ++c) csr[fill[faces_host[(int64_t)f * 3 + c]]++] = (f << 2) | c;
    if (!check_device(device)) return g_render_err.fail(nullptr, THMR_ERR_HIP, "no such HIP device (the render kernels have no CPU fallback)");
    if (hipSetDevice(device) != hipSuccess) return g_render_err.fail(nullptr, THMR_ERR_HIP, "hipSetDevice failed");
    thmr_renderer* r = new thmr_renderer();
    r->device = device; r->F = F; r->V = V;
    hipError_t e = r->faces.reserve((size_t)F * 3, (size_t)F * 3);
    if (e == hipSuccess) e = r->csr_off.reserve((size_t)V + 1, (size_t)V + 1);
    if (e == hipSuccess) e = r->csr.reserve((size_t)F * 3, (size_t)F * 3);
    if (e == hipSuccess) e = hipMemcpy(r->faces, faces_host, sizeof(int32_t) * (size_t)F * 3, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(r->csr_off, cnt.data(), sizeof(int32_t) * ((size_t)V + 1), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(r->csr, csr.data(), sizeof(int32_t) * (size_t)F * 3, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        const std::string m = std::string("renderer setup: ") + hipGetErrorString(e);
        thmr_renderer_destroy(r);
        return g_render_err.fail(nullptr, THMR_ERR_HIP, m);
    }
    *out = r;
    return 0;
}

void thmr_renderer_destroy(thmr_renderer* r) {
    if (!r) return;
    (void)hipSetDevice(r->device);
    delete r;          // the buffers free themselves
}

int thmr_renderer_run(thmr_renderer* r, const thmr_render_desc* d, const float* verts_dev, const float* cam_t_dev, int32_t N,
                      const float* bg_dev, float* out_dev, void* stream) {
    if (!r) return g_render_err.invalid(nullptr, "null renderer");
    if (!d || !verts_dev || !cam_t_dev || !out_dev) return g_render_err.invalid(r, "null descriptor or buffer");
    if (d->width < 1 || d->height < 1 || d->width > 8192 || d->height > 8192)
        return g_render_err.invalid(r, "image size must be 1 ... 8192 per side");
    if (d->samples != 1 && d->samples != 4) return g_render_err.invalid(r, "samples must be 1 or 4");
    if (N < 1) return g_render_err.invalid(r, "N must be >= 1");
    if (d->mode != THMR_RENDER_PER_IMAGE && d->mode != THMR_RENDER_ONE_IMAGE)
        return g_render_err.invalid(r, "mode must be THMR_RENDER_PER_IMAGE or THMR_RENDER_ONE_IMAGE");
    if (d->out_channels != 3 && d->out_channels != 4) return g_render_err.invalid(r, "out_channels must be 3 or 4");
    if (bg_dev && d->out_channels != 3) return g_render_err.invalid(r, "compositing over background images writes 3 channels");
    if (d->n_lights < 0 || d->n_lights > THMR_RENDER_MAX_LIGHTS) return g_render_err.invalid(r, "n_lights must be 0 ... THMR_RENDER_MAX_LIGHTS");
    if ((int64_t)N * r->F * SMALL_TILES >= (int64_t)NONE || (int64_t)N * r->V * 3 >= ((int64_t)1 << 40))
        return g_render_err.invalid(r, "too many meshes");
    const float fl[] = {d->fx, d->fy, d->cx, d->cy};
    for (float v : fl)
        if (!std::isfinite(v)) return g_render_err.invalid(r, "non-finite intrinsics");
    if (!(d->znear > 0.f) || !std::isfinite(d->znear)) return g_render_err.invalid(r, "znear must be a positive number");
    for (int k = 0; k < 9; ++k)
        if (!std::isfinite(d->rot[k])) return g_render_err.invalid(r, "non-finite rotation");
    for (int i = 0; i < d->n_lights; ++i)
        if (d->lights[i].type != THMR_LIGHT_DIRECTIONAL && d->lights[i].type != THMR_LIGHT_POINT)
            return g_render_err.invalid(r, "light " + std::to_string(i) + ": unknown type");

    Params p{};
    p.W = d->width; p.H = d->height; p.S = d->samples; p.mode = d->mode; p.tr_first = d->translate_first ? 1 : 0;
    p.N = N; p.V = r->V; p.F = r->F; p.n_img = d->mode == THMR_RENDER_ONE_IMAGE ? 1 : N;
    p.tiles_x = (p.W + TILE - 1) / TILE; p.tiles_y = (p.H + TILE - 1) / TILE;
    p.ch = d->out_channels; p.has_colors = d->mesh_colors ? 1 : 0; p.has_img = bg_dev ? 1 : 0;
    p.fx = d->fx; p.fy = d->fy; p.cx = d->cx; p.cy = d->cy; p.znear = d->znear;
    for (int k = 0; k < 9; ++k) p.R[k] = d->rot[k];
    for (int k = 0; k < 3; ++k) {
        p.base[k] = d->base_color[k]; p.bg[k] = d->bg_color[k]; p.amb[k] = d->ambient[k];
        p.mean[k] = d->img_mean[k]; p.stdv[k] = d->img_std[k];
    }
    p.metallic = d->metallic; p.roughness = d->roughness; p.n_lights = d->n_lights;
    for (int i = 0; i < d->n_lights; ++i) {
        const thmr_render_light& L = d->lights[i];
        p.L[i].type = L.type;
        for (int k = 0; k < 3; ++k) { p.L[i].v[k] = L.vec[k]; p.L[i].c[k] = L.color[k] * L.intensity; }
    }
    const int64_t T = (int64_t)p.n_img * p.tiles_x * p.tiles_y;
    const size_t NV = (size_t)N * r->V, NF = (size_t)N * r->F;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (hipSetDevice(r->device) != hipSuccess) return g_render_err.invalid(r, "hipSetDevice failed");
    hipError_t e;
    Scratch& s = r->s;
    const char* what;
    auto exact = [](auto& buf, size_t n) { return buf.want(n, n, "hipMalloc(render scratch)"); };
    if ((e = grow_synced(st, {exact(s.pos, NV * 3), exact(s.nrm, NV * 3), exact(s.fix, NV), exact(s.rec, NF), exact(s.cnt, (size_t)T),
                              exact(s.off, (size_t)T + 1), exact(s.cur, (size_t)T), exact(s.lcnt, (size_t)p.n_img),
                              exact(s.bins, NF * SMALL_TILES), exact(s.large, NF), exact(s.colors, (size_t)N * 3)}, what)) != hipSuccess)
        return g_render_err.hip(r, what, e);
    if (d->mesh_colors &&
        (e = hipMemcpyAsync(s.colors, d->mesh_colors, sizeof(float) * (size_t)N * 3, hipMemcpyHostToDevice, st)) != hipSuccess)
        return g_render_err.hip(r, "hipMemcpyAsync(mesh colours)", e);
    if ((e = hipMemsetAsync(s.cnt, 0, sizeof(uint32_t) * (size_t)T, st)) != hipSuccess) return g_render_err.hip(r, "hipMemsetAsync", e);
    if ((e = hipMemsetAsync(s.lcnt, 0, sizeof(uint32_t) * (size_t)p.n_img, st)) != hipSuccess) return g_render_err.hip(r, "hipMemsetAsync", e);
    const unsigned gv = (unsigned)((NV + 255) / 256), gf = (unsigned)((NF + 255) / 256);
    hipLaunchKernelGGL(render_vertex_kernel, dim3(gv), dim3(256), 0, st, p, verts_dev, cam_t_dev, s.pos, s.fix);
    hipLaunchKernelGGL(render_normal_kernel, dim3(gv), dim3(256), 0, st, p, r->faces, r->csr_off, r->csr, s.pos, s.nrm);
    hipLaunchKernelGGL(render_setup_kernel, dim3(gf), dim3(256), 0, st, p, r->faces, s.pos, s.fix, s.rec, s.cnt, s.lcnt, s.large);
    hipLaunchKernelGGL(render_scan_kernel, dim3(1), dim3(1024), 0, st, s.cnt, s.off, s.cur, T);
    hipLaunchKernelGGL(render_fill_kernel, dim3(gf), dim3(256), 0, st, p, s.rec, s.cur, s.bins);
    const dim3 grid((unsigned)(p.tiles_x * p.tiles_y), (unsigned)p.n_img);
    if (p.S == 4)
        hipLaunchKernelGGL(render_raster_kernel<4>, grid, dim3(256), 0, st, p, r->faces, s.pos, s.fix, s.nrm, s.colors, s.rec, s.off,
                           s.bins, s.lcnt, s.large, bg_dev, out_dev, d->ids_dev);
    else
        hipLaunchKernelGGL(render_raster_kernel<1>, grid, dim3(256), 0, st, p, r->faces, s.pos, s.fix, s.nrm, s.colors, s.rec, s.off,
                           s.bins, s.lcnt, s.large, bg_dev, out_dev, d->ids_dev);
    if ((e = hipGetLastError()) != hipSuccess) return g_render_err.hip(r, "render kernel launch", e);
    return 0;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ contact sheet
// MeshRenderer.visualize / visualize_tensorboard (tokenhmr/lib/utils/mesh_renderer.py) in two launches on the caller's stream:
//   sheet_build_kernel   one wave per skeleton: the keypoints -> pixels scaling, visualize_tensorboard's keypoint remap, the
//                        rectangle / thickness arithmetic of render_openpose and its draw list as THMR_SHEET_RECORDS records
//   sheet_kernel         the whole make_grid canvas: padding, image panels, hard-mask mesh panels (alpha > 0.8) and skeleton
//                        panels (records walked last to first per pixel, first hit wins: the painter's order without hazards)
// No atomics, no allocation, no synchronisation; every value is integer or single-rounded fp32 arithmetic, which the NumPy
// restatement (tests/overlay_numpy.py) repeats bit for bit.
namespace {

constexpr int SK_REC = THMR_SHEET_RECORDS;
constexpr int SK_WORDS = THMR_SHEET_RECORD_WORDS;
constexpr int SK_KP = THMR_SHEET_KEYPOINTS;
constexpr int SK_BODY = 25;
constexpr int SK_LIMBS = 24;
constexpr float SK_RANGE = 16385.f;            // |trunc(v)| <= 16384  <=>  |v| < 16385; NaN and inf fail the comparison
enum { PANEL_IMAGE = 0, PANEL_FRONT = 1, PANEL_SIDE = 2, PANEL_PRED = 3, PANEL_GT = 4 };
enum { REC_KIND = 0, REC_X0, REC_Y0, REC_X1, REC_Y1, REC_RADIUS, REC_THICK, REC_COLOR, REC_BX0, REC_BY0, REC_BX1, REC_BY1 };

// OpenPose BODY_25: the limbs it renders (pairs of keypoint indices; a limb takes the colour of its second keypoint) and its palette
__constant__ uint8_t SK_LIMB[SK_LIMBS][2] = {{1, 8},   {1, 2},   {1, 5},   {2, 3},   {3, 4},   {5, 6},   {6, 7},   {8, 9},
                                             {9, 10},  {10, 11}, {8, 12},  {12, 13}, {13, 14}, {1, 0},   {0, 15},  {15, 17},
                                             {0, 16},  {16, 18}, {14, 19}, {19, 20}, {14, 21}, {11, 22}, {22, 23}, {11, 24}};
__constant__ uint8_t SK_COLOR[SK_BODY][3] = {{255, 0, 85},  {255, 0, 0},   {255, 85, 0},  {255, 170, 0}, {255, 255, 0}, {170, 255, 0}, {85, 255, 0},
                                             {0, 255, 0},   {255, 0, 0},   {0, 255, 85},  {0, 255, 170}, {0, 255, 255}, {0, 170, 255}, {0, 85, 255},
                                             {0, 0, 255},   {255, 0, 170}, {170, 0, 255}, {255, 0, 255}, {85, 0, 255},  {0, 0, 255},   {0, 0, 255},
                                             {0, 0, 255},   {0, 255, 255}, {0, 255, 255}, {0, 255, 255}};
// visualize_tensorboard's keypoint_matches: body keypoint i takes extra keypoint SK_REMAP[i] (the 19 after the 25), -1 = keeps its own
__constant__ int8_t SK_REMAP[SK_BODY] = {-1, 12, 8, 7, 6, 9, 10, 11, 14, 2, 1, 0, 3, 4, 5, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1};

struct SheetParams {
    int32_t B, W, H, img_res, n_panels, xmaps, ymaps, pad, Wg, Hg, vec, has_pred, has_gt;
    int32_t kind[5];
    double thick;                              // sqrt(area) * thickness_circle_ratio = sqrt(3 W) / 75, rounded as the host rounds it
};

__device__ __forceinline__ void sk_store(int32_t* rec, int slot, int kind, int x0, int y0, int x1, int y1, int radius, int thick, int color,
                                         int ext, int W, int H) {
    int4 a = make_int4(0, 0, 0, 0), b = a, c = a;
    if (kind) {
        a = make_int4(kind, x0, y0, x1);
        b = make_int4(y1, radius, thick, color);
        c = make_int4(max(min(x0, x1) - ext, 0), max(min(y0, y1) - ext, 0), min(max(x0, x1) + ext, W - 1), min(max(y0, y1) + ext, H - 1));
    }
    int4* o = reinterpret_cast<int4*>(rec + slot * SK_WORDS);
    o[0] = a; o[1] = b; o[2] = c;
}

__global__ void __launch_bounds__(64) sheet_build_kernel(SheetParams p, const float* __restrict__ pred, float* gt, int32_t* __restrict__ rec) {
    const int s = blockIdx.x, l = threadIdx.x;                     // skeleton s: the B predicted ones first, then the B ground-truth ones
    const bool is_gt = !p.has_pred || s >= p.B;
    const int b = (is_gt && p.has_pred) ? s - p.B : s;
    const float res = (float)p.img_res;
    float x = 0.f, y = 0.f, c = 0.f;
    float* g = is_gt ? gt + ((int64_t)b * SK_KP + l) * 3 : nullptr;
    if (l < SK_KP) {
        const float* k = is_gt ? g : pred + ((int64_t)b * SK_KP + l) * 2;
        x = __fmul_rn(res, __fadd_rn(k[0], 0.5f));                // img_res * (k + 0.5) in fp32
        y = __fmul_rn(res, __fadd_rn(k[1], 0.5f));
        c = is_gt ? k[2] : 1.f;                                    // predicted keypoints get confidence 1
    }
    const int src = l < SK_BODY ? SK_REMAP[l] : -1;
    const int from = SK_BODY + (src < 0 ? 0 : src);
    const float ex = __shfl(x, from), ey = __shfl(y, from), ec = __shfl(c, from);
    if (src >= 0 && (!is_gt || (ec > 0.f && c == 0.f))) { x = ex; y = ey; c = ec; }      // unconditional for predictions
    if (is_gt) {
        __syncthreads();                                           // every lane's loads are back before a keypoint is overwritten
        if (l < SK_KP) { g[0] = x; g[1] = y; g[2] = c; }           // the reference scales and remaps the caller's array in place
    }
    // get_keypoints_rectangle over the body keypoints above 0.1; numpy's max / min carry a NaN, which leaves area > 0 false
    const bool body = l < SK_BODY, vr = body && c > 0.1f;
    const bool has_nan = __ballot(vr && (x != x || y != y)) != 0;
    float mxx = vr ? x : -INFINITY, mnx = vr ? x : INFINITY, mxy = vr ? y : -INFINITY, mny = vr ? y : INFINITY;
    for (int o = 32; o; o >>= 1) {
        mxx = fmaxf(mxx, __shfl_xor(mxx, o)); mnx = fminf(mnx, __shfl_xor(mnx, o));
        mxy = fmaxf(mxy, __shfl_xor(mxy, o)); mny = fminf(mny, __shfl_xor(mny, o));
    }
    bool draw = false;
    int t_line = 0, t_circle = 0, radius = 0;
    if (__ballot(vr) != 0 && !has_nan) {
        const float pw = __fsub_rn(mxx, mnx), ph = __fsub_rn(mxy, mny), area = __fmul_rn(pw, ph);
        if (area > 0.f) {
            // the reference reads width, height = img.shape[1], img.shape[2] of an HWC image: "height" is the 3 channels
            const float rw = __fdiv_rn(pw, (float)p.W), rh = __fdiv_rn(ph, 3.f);
            const float m = rh > rw ? rh : rw, ratio = m < 1.f ? m : 1.f;
            const double tr = fmax(rint(p.thick * (double)ratio), 2.0);            // np.round: half to even
            t_circle = (int)(ratio > 0.05f ? tr : 1.0);                               // maximum(1, -1) = 1 on the other branch
            t_line = (int)fmax(1.0, rint(tr * 0.75));
            radius = (int)rint(tr * 0.5);
            draw = true;                                                              // W <= 8192: tr = 2, so all three are <= 2
        }
    }
    rec += (int64_t)s * SK_REC * SK_WORDS;
    const int i1 = l < SK_LIMBS ? SK_LIMB[l][0] : 0, i2 = l < SK_LIMBS ? SK_LIMB[l][1] : 0;
    const float ax = __shfl(x, i1), ay = __shfl(y, i1), ac = __shfl(c, i1), bx = __shfl(x, i2), by = __shfl(y, i2), bc = __shfl(c, i2);
    if (l < SK_LIMBS) {
        const bool ok = draw && ac > 0.1f && bc > 0.1f && fabsf(ax) < SK_RANGE && fabsf(ay) < SK_RANGE && fabsf(bx) < SK_RANGE && fabsf(by) < SK_RANGE;
        sk_store(rec, l, ok ? 1 : 0, (int)ax, (int)ay, (int)bx, (int)by, 0, t_line, i2, (t_line + 1) >> 1, p.W, p.H);
    }
    if (body) {
        const bool ok = draw && c > 0.1f && fabsf(x) < SK_RANGE && fabsf(y) < SK_RANGE;
        sk_store(rec, SK_LIMBS + l, ok ? 2 : 0, (int)x, (int)y, (int)x, (int)y, radius, t_circle, l, radius + ((t_circle + 1) >> 1), p.W, p.H);
    }
}

// Does the primitive cover the pixel whose centre is the integer point (px, py)?  Exact in int64: |coordinate| <= 16384 and
// 0 <= px, py < 8192 keep every difference below 2^15 + 2^13 and |b - a|^2 <= 2^31; radius and thickness are <= 2 from the builder
// (any value below 2^14 would do).  So dot, cross < 2^31.2, cross^2 < 2^62.4 and t^2 |ab|^2 <= 2^33 fit — whereas 4 cross^2 could
// reach 2^64, hence the comparison against (t^2 |ab|^2) >> 2, which is the same predicate because cross^2 is an integer.
__device__ __forceinline__ bool sk_covers(const int32_t* R, int px, int py) {
    const int64_t t = R[REC_THICK], wx = px - R[REC_X0], wy = py - R[REC_Y0], d2 = wx * wx + wy * wy;
    if (R[REC_KIND] == 1) {                    // capsule: distance to the closed segment <= t / 2
        const int64_t dx = R[REC_X1] - R[REC_X0], dy = R[REC_Y1] - R[REC_Y0], len2 = dx * dx + dy * dy, dot = wx * dx + wy * dy;
        if (dot <= 0) return 4 * d2 <= t * t;                      // before a, and a == b
        if (dot >= len2) {
            const int64_t ux = px - R[REC_X1], uy = py - R[REC_Y1];
            return 4 * (ux * ux + uy * uy) <= t * t;
        }
        const int64_t cr = wx * dy - wy * dx;
        return cr * cr <= ((t * t * len2) >> 2);
    }
    const int64_t r = R[REC_RADIUS];           // ring of width k about radius r; k < 0: the filled disc
    if (t < 0) return d2 <= r * r;
    const int64_t lo = 2 * r - t, hi = 2 * r + t;
    return 4 * d2 <= hi * hi && (lo <= 0 || lo * lo <= 4 * d2);
}

// One workgroup works inside one grid cell (a tile with the padding above and left of it; the last column / row of cells also own
// the canvas's right / bottom padding), so it stages at most one skeleton.  A lane owns 4 consecutive canvas x, aligned to 16 B in the
// canvas row: with Wg % 4 == 0 every run inside the cell is one dwordx4 store per plane.
__global__ void __launch_bounds__(256) sheet_kernel(SheetParams p, const float* __restrict__ images, const float* __restrict__ front,
                                                    const float* __restrict__ side, const int32_t* __restrict__ rec, float* __restrict__ canvas) {
    __shared__ int32_t srec[SK_REC * SK_WORDS];
    const int cell = blockIdx.y, cxi = cell % p.xmaps, cyi = cell / p.xmaps;
    const int cw = p.W + p.pad, ch = p.H + p.pad;
    const int X0 = cxi * cw, X1 = cxi == p.xmaps - 1 ? p.Wg : X0 + cw;
    const int Y0 = cyi * ch, Y1 = cyi == p.ymaps - 1 ? p.Hg : Y0 + ch;
    const int person = cell / p.n_panels;
    const int kind = person < p.B ? p.kind[cell % p.n_panels] : -1;                 // make_grid leaves the cells past the last tile at 0
    const bool skel = kind == PANEL_PRED || kind == PANEL_GT;
    if (skel) {
        const int32_t* src = rec + (int64_t)((kind == PANEL_GT && p.has_pred ? p.B : 0) + person) * SK_REC * SK_WORDS;
        for (int i = threadIdx.x; i < SK_REC * SK_WORDS; i += 256) srec[i] = src[i];
    }
    __syncthreads();
    const int q0 = X0 >> 2, nq = ((X1 + 3) >> 2) - q0;
    const int item = blockIdx.x * 256 + threadIdx.x, row = item / nq;
    if (row >= Y1 - Y0) return;
    const int xs = (q0 + item % nq) * 4, y = Y0 + row, ly = y - Y0 - p.pad, lx0 = xs - X0 - p.pad;
    const bool row_in = kind >= 0 && ly >= 0 && ly < p.H;
    unsigned own = 0, inside = 0;
    for (int j = 0; j < 4; ++j) {
        if (xs + j >= X0 && xs + j < X1) own |= 1u << j;
        if (row_in && lx0 + j >= 0 && lx0 + j < p.W) inside |= 1u << j;
    }
    int col[4] = {-1, -1, -1, -1};
    if (skel) {
        unsigned pending = inside;
        for (int r = SK_REC - 1; r >= 0 && pending; --r) {
            const int32_t* R = srec + r * SK_WORDS;
            if (R[REC_KIND] == 0 || ly < R[REC_BY0] || ly > R[REC_BY1] || lx0 + 3 < R[REC_BX0] || lx0 > R[REC_BX1]) continue;
            for (int j = 0; j < 4; ++j)
                if ((pending >> j & 1) && sk_covers(R, lx0 + j, ly)) { col[j] = R[REC_COLOR]; pending &= ~(1u << j); }
        }
    }
    const int64_t plane = (int64_t)p.H * p.W;
    float v[3][4];
    for (int j = 0; j < 4; ++j) {
        v[0][j] = v[1][j] = v[2][j] = 0.f;
        if (!(inside >> j & 1)) continue;
        const int64_t pix = (int64_t)ly * p.W + lx0 + j;
        const float* im = images + (int64_t)person * 3 * plane + pix;
        if (kind == PANEL_IMAGE) {
            for (int c = 0; c < 3; ++c) v[c][j] = im[c * plane];
        } else if (skel) {
            for (int c = 0; c < 3; ++c)                            // render_openpose(255 * img) / 255: two roundings where nothing is drawn
                v[c][j] = col[j] >= 0 ? __fdiv_rn((float)SK_COLOR[col[j]][c], 255.f) : __fdiv_rn(__fmul_rn(255.f, im[c * plane]), 255.f);
        } else {                                                   // color * valid_mask + (1 - valid_mask) * bg, valid = alpha > 0.8
            const float4 px = reinterpret_cast<const float4*>(kind == PANEL_FRONT ? front : side)[(int64_t)person * plane + pix];
            const bool valid = px.w > 0.8f;
            v[0][j] = valid ? px.x : (kind == PANEL_FRONT ? im[0] : 1.f);
            v[1][j] = valid ? px.y : (kind == PANEL_FRONT ? im[plane] : 1.f);
            v[2][j] = valid ? px.z : (kind == PANEL_FRONT ? im[2 * plane] : 1.f);
        }
    }
    const int64_t gplane = (int64_t)p.Hg * p.Wg;
    float* dst = canvas + (int64_t)y * p.Wg + xs;
    for (int c = 0; c < 3; ++c, dst += gplane) {
        if (p.vec && own == 15u) {
            *reinterpret_cast<float4*>(dst) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
        } else {
            for (int j = 0; j < 4; ++j)
                if (own >> j & 1) dst[j] = v[c][j];
        }
    }
}

}  // namespace

extern "C" {

int thmr_renderer_sheet(thmr_renderer* r, const thmr_sheet_desc* d, const float* images_dev, const float* front_dev, const float* side_dev,
                        const float* pred_kp_dev, float* gt_kp_dev, int32_t* records_dev, float* canvas_dev, void* stream) {
    if (!r) return g_render_err.invalid(nullptr, "null renderer");
    if (!d || !images_dev || !canvas_dev) return g_render_err.invalid(r, "null descriptor or buffer");
    if (d->n < 1 || d->n > (1 << 20)) return g_render_err.invalid(r, "n must be 1 ... 2^20 people");
    if (d->width < 1 || d->height < 1 || d->width > 8192 || d->height > 8192)
        return g_render_err.invalid(r, "image size must be 1 ... 8192 per side");
    if (d->img_res < 1 || d->img_res > 8192) return g_render_err.invalid(r, "img_res must be 1 ... 8192");
    if (d->nrow < 1 || d->padding < 0 || d->padding > 4096) return g_render_err.invalid(r, "nrow must be >= 1 and padding 0 ... 4096");
    if (d->panels & ~(THMR_SHEET_IMAGE | THMR_SHEET_FRONT | THMR_SHEET_SIDE)) return g_render_err.invalid(r, "unknown panel bit");
    if (((d->panels & THMR_SHEET_FRONT) && !front_dev) || ((d->panels & THMR_SHEET_SIDE) && !side_dev))
        return g_render_err.invalid(r, "a requested mesh panel has no render");
    if ((pred_kp_dev || gt_kp_dev) && !records_dev) return g_render_err.invalid(r, "skeleton panels need the records buffer");
    if (reinterpret_cast<uintptr_t>(records_dev) % 16 || reinterpret_cast<uintptr_t>(front_dev) % 16 || reinterpret_cast<uintptr_t>(side_dev) % 16)
        return g_render_err.invalid(r, "records and RGBA buffers must be 16-byte aligned");
    SheetParams p{};
    p.B = d->n; p.W = d->width; p.H = d->height; p.img_res = d->img_res; p.pad = d->padding;
    p.has_pred = pred_kp_dev ? 1 : 0; p.has_gt = gt_kp_dev ? 1 : 0;
    if (d->panels & THMR_SHEET_IMAGE) p.kind[p.n_panels++] = PANEL_IMAGE;
    if (d->panels & THMR_SHEET_FRONT) p.kind[p.n_panels++] = PANEL_FRONT;
    if (d->panels & THMR_SHEET_SIDE) p.kind[p.n_panels++] = PANEL_SIDE;
    if (p.has_pred) p.kind[p.n_panels++] = PANEL_PRED;
    if (p.has_gt) p.kind[p.n_panels++] = PANEL_GT;
    if (!p.n_panels) return g_render_err.invalid(r, "no panel requested");
    // torchvision.utils.make_grid(list, nrow, padding), pad value 0
    const int64_t tiles = (int64_t)p.B * p.n_panels;
    const int64_t xmaps = std::min<int64_t>(d->nrow, tiles), ymaps = (tiles + xmaps - 1) / xmaps;
    const int64_t Wg = xmaps * (p.W + p.pad) + p.pad, Hg = ymaps * (p.H + p.pad) + p.pad;
    if (Wg > (1 << 24) || Hg > (1 << 24)) return g_render_err.invalid(r, "canvas beyond 2^24 per side");
    if (d->canvas_width != Wg || d->canvas_height != Hg)
        return g_render_err.invalid(r, "canvas must be " + std::to_string(Hg) + " x " + std::to_string(Wg) + " for these tiles");
    p.xmaps = (int32_t)xmaps; p.ymaps = (int32_t)ymaps; p.Wg = (int32_t)Wg; p.Hg = (int32_t)Hg;
    p.vec = (Wg % 4 == 0 && reinterpret_cast<uintptr_t>(canvas_dev) % 16 == 0) ? 1 : 0;
    p.thick = std::sqrt((double)((int64_t)p.W * 3)) * (1.0 / 75.0);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (hipSetDevice(r->device) != hipSuccess) return g_render_err.invalid(r, "hipSetDevice failed");
    const int n_skel = (p.has_pred + p.has_gt) * p.B;
    if (n_skel) hipLaunchKernelGGL(sheet_build_kernel, dim3((unsigned)n_skel), dim3(64), 0, st, p, pred_kp_dev, gt_kp_dev, records_dev);
    const int64_t items = (int64_t)(((p.W + 2 * p.pad + 3) >> 2) + 1) * (p.H + 2 * p.pad);
    const int64_t cells = xmaps * ymaps;
    if (cells > 65535) return g_render_err.invalid(r, "more than 65535 grid cells");
    hipLaunchKernelGGL(sheet_kernel, dim3((unsigned)((items + 255) / 256), (unsigned)cells), dim3(256), 0, st, p, images_dev, front_dev, side_dev,
                       records_dev, canvas_dev);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return g_render_err.hip(r, "sheet kernel launch", e);
    return 0;
}

}  // extern "C"
