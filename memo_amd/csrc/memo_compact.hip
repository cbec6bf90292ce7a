// memo_compact.hip -- what the count / scan / scatter passes of the library share that is no template: the one-workgroup scan of the
// tile counts (memo_compact.h's compaction, memo_text.hip's line numbers) and the gather of the bases at the plane boundaries.
#include "memo_common.h"

namespace {

// exclusive scan of the tile counts into int64 bases, their sum into *total: one workgroup, 1024 tiles a round (a 300 MB text has
// 2 * 10^4 tiles)
__global__ __launch_bounds__(1024) void tile_counts_scan_kernel(const uint32_t *__restrict__ counts, int64_t ntiles, int64_t *__restrict__ bases,
                                                                int64_t *total_out) {
    __shared__ long long wsum[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long carry = 0;
    for (int64_t c0 = 0; c0 < ntiles; c0 += 1024) {
        const int64_t i = c0 + threadIdx.x;
        const long long x = i < ntiles ? (long long)counts[i] : 0;
        long long s = x;  // inclusive scan inside the wave
        for (int off = 1; off < 64; off <<= 1) {
            const long long t = __shfl_up(s, off, 64);
            if (lane >= off) s += t;
        }
        if (lane == 63) wsum[wave] = s;
        __syncthreads();
        long long before = 0, total = 0;
        for (int w = 0; w < 16; ++w) {
            const long long t = wsum[w];
            before += w < wave ? t : 0;
            total += t;
        }
        if (i < ntiles) bases[i] = carry + before + s - x;
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total_out = carry;
}

// out[pl] = the base of plane pl's first tile, out[planes] = the total
__global__ __launch_bounds__(256) void mems_plane_bases(const int64_t *__restrict__ bases, const int64_t *__restrict__ total,
                                                          int64_t tiles_per_plane, int64_t planes, int64_t *__restrict__ out) {
    const int64_t pl = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (pl < planes) out[pl] = bases[pl * tiles_per_plane];
    else if (pl == planes) out[pl] = *total;
}

}  // namespace

hipError_t memo::scan_tile_counts(const uint32_t *d_counts, int64_t ntiles, int64_t *d_bases, int64_t *d_total, hipStream_t st) {
    hipLaunchKernelGGL(tile_counts_scan_kernel, dim3(1), dim3(1024), 0, st, d_counts, ntiles, d_bases, d_total);
    return hipGetLastError();
}

hipError_t memo::plane_bases(const int64_t *d_bases, const int64_t *d_total, int64_t tiles_per_plane, int64_t planes, int64_t *d_out, hipStream_t st) {
    hipLaunchKernelGGL(mems_plane_bases, dim3((unsigned)(planes / 256 + 1)), dim3(256), 0, st, d_bases, d_total, tiles_per_plane, planes, d_out);
    return hipGetLastError();
}
