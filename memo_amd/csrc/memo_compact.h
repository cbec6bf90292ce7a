// memo_compact.h -- count, scan and scatter of flagged positions: the compaction that `memo regions` (memo_runs.hip) and `memo mems`
// (memo_mems.hip) make of a result that is still in HBM, and the two device pieces of it that the text parser (memo_text.hip) uses on
// its own tiles.  Not part of the public ABI.
//
// A KEY says what is flagged.  It supplies
//   kPer                      positions a lane owns per load; a tile is 256 lanes x kCompactIters loads x kPer positions
//   Start                     the type of a stored position: int64_t (runs) or uint32_t (mems)
//   tile_of(block, plane, p0) the plane and first position of tile `block`: tiles never cross a plane, and their order is plane-major
//                             (one plane: plane 0, p0 = block x tile)
//   flags(plane, p)           bit j: position p + j (p a multiple of kPer) is flagged; called by whole waves (it may shuffle); a position
//                             at or past the plane's end sets no bit
//   store(plane, rank, i)     the payload of flagged position i, which is the rank-th of all
// Launches, ordered by the stream:
//   compact_count_kernel      per tile its flags counted, one uint32 per tile, no atomics
//   the scan                  memo::scan_tile_counts (memo_compact.hip): int64 bases and the total; with planes, memo::plane_bases gathers the
//                             bases at the plane boundaries and the total into planes + 1 entries
//   compact_scatter_kernel    the flags recomputed; rank = tile base + the flags of the waves before + of the loads before + of the lanes
//                             below (ballot / mbcnt); starts[rank] = i and the key's payload
// The host reads the total (the plane bases) between the scan and the scatter, and the caller allocates exactly that many entries.
// No workgroup waits for another; the scatter writes no rank at or past the total.
#ifndef MEMO_COMPACT_H
#define MEMO_COMPACT_H

#include <vector>

#include "memo_common.h"

namespace memo {

constexpr int kCompactThreads = 256, kCompactIters = 4;  // a wave owns kCompactIters x 64 x kPer positions in a row

// the count tail: a lane's count summed over the workgroup (wave reduce, the four wave sums through LDS) into counts[tile]
__device__ __forceinline__ void store_tile_count(uint32_t n, uint32_t *__restrict__ counts) {
    __shared__ uint32_t wsum[kCompactThreads / 64];
    for (int off = 32; off; off >>= 1) n += __shfl_xor(n, off, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// the ranks: mask[it] holds the PER flags of a lane's load `it`; rank[it] becomes the rank of the first of them among its wave's -- the
// lanes below by ballot + mbcnt, the loads before by a running sum -- and the flags of the waves before come back (wtot: LDS [4]; one
// barrier, all lanes call it)
template <int PER>
__device__ __forceinline__ uint32_t rank_flags(const uint32_t (&mask)[kCompactIters], uint32_t (&rank)[kCompactIters], uint32_t *wtot) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t running = 0;
#pragma unroll
    for (int it = 0; it < kCompactIters; ++it) {
        uint32_t below = 0, count = 0;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const unsigned long long bal = __ballot((mask[it] >> j) & 1u);
            below += __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
            count += (uint32_t)__popcll(bal);
        }
        rank[it] = running + below;
        running += count;
    }
    if (lane == 0) wtot[wave] = running;
    __syncthreads();
    uint32_t before = 0;
    for (int w = 0; w < wave; ++w) before += wtot[w];
    return before;
}

template <typename Key>
constexpr int tile_positions() { return kCompactThreads * kCompactIters * Key::kPer; }

template <typename Key>
__device__ __forceinline__ int64_t chunk_pos(int64_t p0, int it) {
    return p0 + (int64_t)(((threadIdx.x >> 6) * kCompactIters + it) * 64 + (threadIdx.x & 63)) * Key::kPer;
}

template <typename Key>
__global__ __launch_bounds__(kCompactThreads) void compact_count_kernel(Key key, uint32_t *__restrict__ counts) {
    int64_t plane, p0;
    key.tile_of(blockIdx.x, plane, p0);
    uint32_t n = 0;
#pragma unroll
    for (int it = 0; it < kCompactIters; ++it) n += (uint32_t)__popc(key.flags(plane, chunk_pos<Key>(p0, it)));
    store_tile_count(n, counts);
}

template <typename Key>
__global__ __launch_bounds__(kCompactThreads) void compact_scatter_kernel(Key key, const int64_t *__restrict__ bases, int64_t total,
                                                                          typename Key::Start *__restrict__ starts) {
    __shared__ uint32_t wtot[kCompactThreads / 64];
    int64_t plane, p0;
    key.tile_of(blockIdx.x, plane, p0);
    uint32_t mask[kCompactIters], rank[kCompactIters];
#pragma unroll
    for (int it = 0; it < kCompactIters; ++it) mask[it] = key.flags(plane, chunk_pos<Key>(p0, it));
    const int64_t base = bases[blockIdx.x] + rank_flags<Key::kPer>(mask, rank, wtot);
#pragma unroll
    for (int it = 0; it < kCompactIters; ++it) {
        int64_t idx = base + rank[it];
        const int64_t p = chunk_pos<Key>(p0, it);
        for (uint32_t m = mask[it]; m; m &= m - 1, ++idx) {
            if (idx >= total) break;  // (cannot happen while both passes see the same input: a caller that writes it meanwhile)
            const int64_t i = p + __builtin_ctz(m);
            starts[idx] = (typename Key::Start)i;
            key.store(plane, idx, i);
        }
    }
}

// The host sequence.  lay_out: one work allocation -- the total, the tiles' bases, with planes their bases and the total again, the
// tiles' counts.  count: count, scan, the total (planes: the plane bases) to the host; blocking.  Then the caller allocates total()
// entries, and scatter fills them; blocking.  The laps are a timed call's (mems): count, scan + plane bases, scatter.
struct Compaction {
    hipStream_t st;
    Laps laps;
    int64_t ntiles = 0, planes = 0;  // planes 0: one plane, and only the total comes to the host
    DevPtr<int64_t> work;
    size_t work_bytes = 0;
    std::vector<int64_t> plane_base;  // [planes + 1]: where a plane's entries begin; the last one the total
    Compaction(hipStream_t s, const int &timed, float *ms) : st(s), laps(s, timed, ms) {}

    hipError_t lay_out(int64_t tiles, int64_t pl) {
        ntiles = tiles, planes = pl;
        const size_t words = (size_t)(1 + ntiles + (planes ? planes + 1 : 0) + (ntiles + 1) / 2);
        work_bytes = words * sizeof(int64_t);
        return work.alloc(words);
    }
    int64_t *d_total() const { return work; }
    int64_t *d_bases() const { return work + 1; }
    int64_t total() const { return plane_base.back(); }

    template <typename Key>
    int count(const Key &key) {
        int64_t *d_plane = d_bases() + ntiles;
        uint32_t *d_counts = reinterpret_cast<uint32_t *>(d_plane + (planes ? planes + 1 : 0));
        if (int rc = laps.start()) return rc;
        hipLaunchKernelGGL(compact_count_kernel<Key>, dim3((unsigned)ntiles), dim3(kCompactThreads), 0, st, key, d_counts);
        HIP_TRY(hipGetLastError());
        if (int rc = laps.lap(0)) return rc;
        HIP_TRY(scan_tile_counts(d_counts, ntiles, d_bases(), d_total(), st));
        if (planes) HIP_TRY(plane_bases(d_bases(), d_total(), ntiles / planes, planes, d_plane, st));
        if (int rc = laps.lap(1)) return rc;
        plane_base.assign((size_t)planes + 1, 0);
        HIP_TRY(hipMemcpyAsync(plane_base.data(), planes ? d_plane : d_total(), plane_base.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return MEMO_OK;
    }

    template <typename Key>
    int scatter(const Key &key, typename Key::Start *starts) {
        if (int rc = laps.start()) return rc;
        hipLaunchKernelGGL(compact_scatter_kernel<Key>, dim3((unsigned)ntiles), dim3(kCompactThreads), 0, st, key, d_bases(), total(), starts);
        HIP_TRY(hipGetLastError());
        if (int rc = laps.lap(2)) return rc;
        HIP_TRY(hipStreamSynchronize(st));
        return MEMO_OK;
    }
};

}  // namespace memo

#endif  // MEMO_COMPACT_H
