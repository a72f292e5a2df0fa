// Device helpers of the kernels that run over a whole batch of items at once (png.hip, jpeg.hip, jpegenc.hip): which item a global row /
// segment / block / chunk belongs to, and the wave and workgroup sums and scans over 64-lane waves.  Device only; everything is forced
// inline, so each kernel gets the code it had when these were written out in its own file.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// The last item whose first row / segment / block / chunk (the member at `first`, int32_t or int64_t) is <= g.  Items without any (an
// empty window) share the value with their successor, which is then the one found.
template <auto first, typename Item, typename G>
__device__ __forceinline__ int item_of(const Item* items, int n, G g) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (items[mid].*first <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// The integer sum over a wave, in every lane (common.h has the float one).
__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// Inclusive prefix sum over the 64 lanes of a wave.
template <typename T>
__device__ __forceinline__ T wave_scan_inclusive(T v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T up = __shfl_up(v, d);
        if (lane >= d) v += up;
    }
    return v;
}

// Exclusive prefix sum over the 256 lanes of a workgroup; total: the sum, in every lane.  part: 4 words of LDS.
template <typename T>
__device__ __forceinline__ T block_scan(T v, T* part, T& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const T incl = wave_scan_inclusive(v, lane);
    __syncthreads();                // the previous use of part is over
    if (lane == 63) part[w] = incl;
    __syncthreads();
    T before = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (i < w) before += part[i];
        total += part[i];
    }
    return before + incl - v;
}
