// memo_planes_dap.h -- the one body of the three planes-to-matrix kernels: convert_dap_kernel (memo_convert.hip), add_dap_kernel
// (memo_add.hip) and merge_dap_kernel (memo_merge.hip).  Each turns a finished slice of genome-major uint32 planes (memo_lengths.hip:
// cell[plane][p], how far that genome matches the pivot from position p) into the position-major int32 matrix the row builder reads
// (memo_dap.hip: one row per position), clipped at the end of the record:
//     dap[i][c] = min( cell[plane of column c][first + i], remaining - i )        0 <= i < positions, 0 <= c < cols
// They differ in where a column's plane comes from (the two sources below) and in nothing else that is here; what one kernel adds
// stands in its own file.  Not part of the public ABI.
//
// The kernel is a transposition through LDS.  A workgroup of 256 lanes takes a tile of kTP = 128 positions x kTG = 64 columns.
// Position tiles lie at multiples of kTP of the PLANE (not of `first`): the planes are 16-byte aligned and pitch % 4 == 0, so a whole
// tile loads with 16-byte loads whatever `first` is.  The workgroup index is position tile * column tiles + column tile: the workgroups
// that write the pieces of one output row run side by side.
//   load   a whole tile: every lane holds 8 uint4 (4 neighbouring positions of one plane each), all in flight before the first goes to
//          LDS.  A 32-lane group is 8 quads x 4 columns: 128 bytes in a row from each of four planes.
//          a tile that crosses `first` or `first + positions`: element by element, 32 neighbouring lanes on 32 neighbouring positions of
//          one plane, nothing outside [first, first + positions) is read.  Columns past the source's n are skipped in both forms.
//   source Straight: column g is plane g from a base (convert; add's old columns).  No key is read.
//          Mapped: the plane comes from a column map (merge); an entry outside [0, planes) names no plane, loads nothing and puts 0 into
//          LDS.  Every lane reads ITS OWN entries straight from global memory.  In a whole tile a lane's eight 16-byte loads go to eight
//          columns, g = 8 u + 4 (t >> 7) + ((t & 31) >> 3): eight 4-byte loads, issued together in front of the plane loads, neighbouring
//          lanes on the same or neighbouring words of one 256-byte piece of the map (all of it stays in L2 and L1: at most 8 KiB, read by
//          every workgroup).  They cost one cache round trip in front of the plane loads, which is what merge_dap_kernel is behind
//          convert_dap_kernel on the same planes: 0.083 against 0.077 ms at 2.2 M positions x 15 columns, identity and permuted map alike
//          (profiles/merge_timing.txt; four workgroups a CU leave a round trip per tile in the open).  The other way, staging the tile's
//          64 entries in LDS once, pays the same round trip (64 lanes load, all wait), then a barrier before the first plane load can
//          issue and eight LDS reads a lane, for 256 bytes of LDS: it saves 7 of 8 global loads that hit the cache anyway and puts the
//          whole load phase behind a workgroup barrier.  Not chosen, and not built.  Built and dropped: the wave's 32 entries by scalar
//          loads (a wave's columns are the same for all its lanes but two bits) -- the compiler waits for each before it issues the
//          next, 24 round trips instead of one.  An edge tile reads the entry of every element's column, one word for the 128 lanes and
//          steps that share the column.
//          A source hands out a column's key as ONE select with a sentinel (g < n ? entry : -1) and says with ONE predicate,
//          named(key, n), whether the key names a plane.  A key assigned under `if (g < n)` and loads guarded by `g < n && named` gave
//          the same registers and the same loads in a prototype, but the compiler then waited for each pair of plane loads before it
//          issued the next.
//   LDS    uint32 tile[kTG][kStride], kStride = kTP + 1 = 129 words (33 024 bytes).  The stride is odd, so both sides spread over the banks
//          (64 banks of 4 bytes; a ds_write_b32 and a ds_read_b32 are served in two groups of 32 lanes over (a / 4) mod 32):
//            the store of dword j of a quad: word = g * 129 + 4 q + j with 8 q and 4 g per group -- g * 129 mod 4 tells the four
//              columns apart, 4 q the eight quads: 32 banks (four ds_write_b32 per uint4: a 16-byte store would need a stride that is a
//              multiple of 4 words, which puts the read side 4-way on a bank)
//            the read of a run of columns at position i: word = g * 129 + i, 32 neighbouring g per group: 32 banks.  Where a group runs over
//              the end of one position's columns into the next position's it is 2-way at most.
//          The bank argument is about LDS addresses, which a column map does not touch.
//   store  the tile's output laid end to end, element f = i * ng + g (ng columns in this tile): lane t takes f = t, t + 256 ...  A full
//          column tile writes 256 bytes in a row per position and wave; a matrix of fewer than 64 columns is written as one contiguous
//          run.  Plain 4-byte stores: an output row starts at 4 cols i bytes, 16-byte aligned for some widths only.  (i, g) advance by
//          (256 / ng, 256 % ng) with one carry: one division per lane and tile.
//
// Conditions the code holds:
//   - no workgroup waits for another: no look-back, no flag in memory, no cooperative launch
//   - nothing is read outside [first, first + positions) of a plane that a column names; a map entry is compared with [0, planes) as an
//     unsigned number before it becomes an offset: whatever the map holds, nothing outside the `planes` planes is read
//   - nothing is written outside positions * cols integers, and every one of them is written once
//   - a tile that crosses either edge is taken element by element
//   - MEMO_EINVAL before any launch (refuse): pitch % 4 != 0, first + positions > pitch, remaining < positions, remaining > 2^31 - 1,
//     cells that are not 16-byte aligned, another array or an output that is not 4-byte aligned, a negative count; each entry point adds
//     the limits of its own counts and the NULL pointers with positions > 0; positions == 0 launches nothing
//   - offsets into the planes and the matrix are 64-bit (65 536 planes of pitch 2^31 are 2^47 cells); a value is at most
//     remaining - i <= 2^31 - 1 and fits the int32 it becomes
//   - values are written with vector stores only; there is no inline assembly
#ifndef MEMO_PLANES_DAP_H
#define MEMO_PLANES_DAP_H

#include <algorithm>

#include "memo_common.h"

namespace memo {
namespace planes_dap {

constexpr int kThreads = 256;
constexpr int kTP = 128;                  // positions per tile
constexpr int kTG = 64;                   // columns per tile
constexpr int kStride = kTP + 1;          // words per column in LDS: odd (see the header)
constexpr int kQuads = kTP / 4;           // 16-byte loads per column and tile
constexpr int kLoads = kTG * kQuads / kThreads;  // 16-byte loads a lane has in flight: 8
constexpr int64_t kMaxRemaining = 0x7FFFFFFF;
static_assert(kStride % 2 == 1 && kTG * kQuads % kThreads == 0 && kTP % 32 == 0, "the lane layout of the load");

// what the three kernels' arguments share (every kernel's argument struct begins with one, as `f`)
struct Frame {
    int32_t *dap;
    int64_t pitch, first, positions, remaining;
    int cols;    // of the matrix
    int ctiles;  // column tiles
};

struct Tile {
    int64_t t0, end;  // the tile's first position in the plane; first + positions
    int c0, ng;       // its columns [c0, c0 + ng)
    bool whole;       // no position of it lies outside [first, first + positions)
};

__device__ __forceinline__ Tile tile_of(const Frame &F) {
    const int64_t wg = blockIdx.x;
    Tile T;
    T.t0 = (F.first / kTP + wg / F.ctiles) * kTP;
    T.c0 = (int)(wg % F.ctiles) * kTG, T.ng = min(kTG, F.cols - T.c0);
    T.end = F.first + F.positions;
    T.whole = T.t0 >= F.first && T.t0 + kTP <= T.end;
    return T;
}

struct Straight {
    const uint32_t *base;  // the plane of the tile's column 0
    __device__ __forceinline__ int key(int g, int n) const { return g; }
    __device__ __forceinline__ bool named(int key, int n) const { return key < n; }
    __device__ __forceinline__ const uint32_t *plane(int key, int64_t pitch) const { return base + (int64_t)key * pitch; }
};

struct Mapped {
    const uint32_t *cells;  // plane 0 of the stack
    const int32_t *map;     // the entry of the tile's column 0
    int planes;
    __device__ __forceinline__ int32_t key(int g, int n) const { return g < n ? map[g] : -1; }
    __device__ __forceinline__ bool named(int32_t key, int n) const { return (uint32_t)key < (uint32_t)planes; }
    __device__ __forceinline__ const uint32_t *plane(int32_t key, int64_t pitch) const { return cells + (int64_t)key * pitch; }
};

// columns [0, n) of the tile, from their planes into LDS
template <typename Source>
__device__ __forceinline__ void load_planes(uint32_t *tile, const Frame &F, const Tile &T, int n, const Source &S) {
    if (T.whole) {
        uint4 v[kLoads];
        int32_t m[kLoads];
        const int lane = threadIdx.x & 31, q_lo = lane & 7, g_lo = lane >> 3;
#pragma unroll
        for (int u = 0; u < kLoads; ++u) {
            const int grp = (u * kThreads + threadIdx.x) >> 5;  // 64 groups: 4 blocks of 8 quads x 16 blocks of 4 columns
            m[u] = S.key((grp >> 2) * 4 + g_lo, n);
        }
#pragma unroll
        for (int u = 0; u < kLoads; ++u) {
            const int grp = (u * kThreads + threadIdx.x) >> 5;
            const int q = (grp & 3) * 8 + q_lo;
            if (S.named(m[u], n)) v[u] = *reinterpret_cast<const uint4 *>(S.plane(m[u], F.pitch) + T.t0 + 4 * q);
        }
#pragma unroll
        for (int u = 0; u < kLoads; ++u) {
            const int grp = (u * kThreads + threadIdx.x) >> 5;
            const int q = (grp & 3) * 8 + q_lo, g = (grp >> 2) * 4 + g_lo;
            if (g < n) {
                const uint4 w = S.named(m[u], n) ? v[u] : make_uint4(0, 0, 0, 0);  // (no plane: nothing was loaded)
                uint32_t *d = tile + g * kStride + 4 * q;
                d[0] = w.x, d[1] = w.y, d[2] = w.z, d[3] = w.w;
            }
        }
    } else {
        for (int e = threadIdx.x; e < n * kTP; e += kThreads) {
            const int g = e / kTP, q = e % kTP;
            const int64_t p = T.t0 + q;
            __builtin_assume(g < n);  // (the key is read without a branch)
            if (p >= F.first && p < T.end) {
                const int32_t key = S.key(g, n);
                tile[g * kStride + q] = S.named(key, n) ? S.plane(key, F.pitch)[p] : 0u;
            }
        }
    }
}

// the tile out of LDS (after the barrier), clipped at the end of the record
__device__ __forceinline__ void store_rows(const uint32_t *tile, const Frame &F, const Tile &T) {
    const int di = kThreads / T.ng, dg = kThreads % T.ng;
    int i = threadIdx.x / T.ng, g = threadIdx.x % T.ng;
    while (i < kTP) {
        const int64_t at = T.t0 + i - F.first;  // the row of the matrix
        if (at >= 0 && at < F.positions) {
            const uint32_t room = (uint32_t)(F.remaining - at);  // (1 .. 2^31 - 1)
            F.dap[at * F.cols + T.c0 + g] = (int32_t)min(tile[g * kStride + i], room);
        }
        i += di, g += dg;
        if (g >= T.ng) g -= T.ng, ++i;
    }
}

// The refusals the three entry points share, after the limits of their own counts and before their NULL checks.  d_side, where a
// kernel has another device array (`side` names it), is held to 4 bytes between the cells and the output.
inline int refuse(const uint32_t *d_cells, int64_t pitch, int64_t first, int64_t positions, int64_t remaining, const int32_t *d_dap,
                  const void *d_side = nullptr, const char *side = nullptr) {
    if (pitch < 0 || first < 0 || positions < 0 || remaining < 0)
        return fail(MEMO_EINVAL, "a negative count: pitch %lld, first %lld, positions %lld, remaining %lld", (long long)pitch, (long long)first,
                    (long long)positions, (long long)remaining);
    if (pitch & 3) return fail(MEMO_EINVAL, "pitch %lld must be a multiple of 4", (long long)pitch);
    if (first > pitch || positions > pitch - first)
        return fail(MEMO_EINVAL, "positions [%lld, %lld + %lld) do not lie inside a plane of pitch %lld", (long long)first, (long long)first, (long long)positions,
                    (long long)pitch);
    if (remaining < positions) return fail(MEMO_EINVAL, "remaining %lld is less than the %lld positions", (long long)remaining, (long long)positions);
    if (remaining > kMaxRemaining) return fail(MEMO_EINVAL, "remaining %lld is above 2^31 - 1", (long long)remaining);
    if (reinterpret_cast<uintptr_t>(d_cells) & 15) return fail(MEMO_EINVAL, "d_cells must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_side) & 3) return fail(MEMO_EINVAL, "%s must be 4-byte aligned", side);
    if (reinterpret_cast<uintptr_t>(d_dap) & 3) return fail(MEMO_EINVAL, "d_dap must be 4-byte aligned");
    return MEMO_OK;
}

// the frame of a matrix of `cols` columns, and its launch: one workgroup per tile
inline Frame frame(int64_t pitch, int64_t first, int64_t positions, int64_t remaining, int cols, int32_t *d_dap) {
    return {d_dap, pitch, first, positions, remaining, cols, (cols + kTG - 1) / kTG};
}

template <typename Args>
int launch(void (*kernel)(Args), const Args &A, int32_t device, void *stream) {
    OnDevice on(device);
    if (on.rc) return on.rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const Frame &F = A.f;
    const int64_t ptiles = (F.first + F.positions - 1) / kTP - F.first / kTP + 1;  // (at most 2^24 + 1, times at most 32 column tiles: fits grid.x)
    hipLaunchKernelGGL(kernel, dim3((unsigned)(ptiles * F.ctiles)), dim3(kThreads), 0, st, A);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    return MEMO_OK;
}

}  // namespace planes_dap
}  // namespace memo

#endif  // MEMO_PLANES_DAP_H
