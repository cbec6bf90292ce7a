// memo_merge.hip -- `memo merge`: the row builder's matrix of chosen genomes, in a chosen order, from the planes of one or more membership
// indexes on one pivot.  The planes of all inputs lie stacked in one buffer with one pitch, genome-major uint32 as memo_lengths.hip leaves
// them (cell[plane][p]: how far that genome matches the pivot from position p); a column map names the plane of every column of the
// position-major int32 matrix (memo_dap.hip reads it), clipped at the end of the record:
//     dap[i][c] = min( cell[plane_of[c]][first + i], remaining - i )            0 <= i < positions, 0 <= c < cols
// A plane may be named by no column, by one or by several; an entry outside [0, planes) names none and its column is 0.  No counterpart in
// the reference.
//
// merge_dap_kernel is convert_dap_kernel (memo_convert.hip, whose header gives the bank argument) with the 64 plane bases of a tile taken
// from the map instead of c0 + g: a workgroup of 256 lanes takes a tile of kTP = 128 positions x kTG = 64 columns through one LDS tile.
// Position tiles lie at multiples of kTP of the PLANE (not of `first`).  The workgroup index is position tile * column tiles + column tile.
//   map    every lane reads ITS OWN entries straight from global memory.  In a whole tile a lane's eight 16-byte loads go to eight columns,
//          g = 8 u + 4 (t >> 7) + ((t & 31) >> 3): eight 4-byte loads, issued together in front of the plane loads, neighbouring lanes on
//          the same or neighbouring words of one 256-byte piece of the map (all of it stays in L2 and L1: at most 8 KiB, read by every
//          workgroup).  They cost one cache round trip in front of the plane loads, which is what the kernel is behind convert_dap_kernel
//          on the same planes: 0.083 against 0.077 ms at 2.2 M positions x 15 columns, identity and permuted map alike
//          (profiles/merge_timing.txt; four workgroups a CU leave a round trip per tile in the open).  The other way, staging the tile's
//          64 entries in LDS once, pays the same round trip (64 lanes load, all wait), then a barrier before the first plane load can
//          issue and eight LDS reads a lane, for 256 bytes of LDS: it saves 7 of 8 global loads that hit the cache anyway and puts the
//          whole load phase behind a workgroup barrier.  Not chosen, and not built.  Built and dropped: the wave's 32 entries by scalar
//          loads (a wave's columns are the same for all its lanes but two bits) -- the compiler waits for each before it issues the
//          next, 24 round trips instead of one.  An edge tile reads the entry of every element's column, one word for the 128 lanes and
//          steps that share the column.
//   load   a whole tile: every lane holds 8 uint4 (4 neighbouring positions of one plane each), all in flight before the first goes to
//          LDS.  A 32-lane group is 8 quads x 4 columns: 128 bytes in a row from each of four planes, wherever the map puts them.
//          a tile that crosses `first` or `first + positions`: element by element, 32 neighbouring lanes on 32 neighbouring positions of
//          one plane; nothing outside [first, first + positions) is read.  Columns past `cols` are skipped in both forms; a column whose
//          entry names no plane loads nothing and puts 0 into LDS.
//   LDS    uint32 tile[kTG][kStride], kStride = kTP + 1 = 129 words (33 024 bytes), exactly as in convert_dap_kernel: the bank argument
//          is about LDS addresses, which the map does not touch.
//   store  the tile's output laid end to end, element f = i * ng + g (ng columns in this tile): lane t takes f = t, t + 256 ...; plain
//          4-byte stores, one contiguous run a tile and position.
//
// Conditions the code holds:
//   - no workgroup waits for another: no look-back, no flag in memory, no cooperative launch
//   - a map entry is compared with [0, planes) as an unsigned number before it becomes an offset: whatever the map holds, nothing outside
//     the `planes` planes is read
//   - nothing is read outside [first, first + positions) of a named plane; nothing outside plane_of[0 .. cols)
//   - nothing is written outside positions * cols integers, and every one of them is written once
//   - a tile that crosses either edge is taken element by element
//   - MEMO_EINVAL before any launch: planes outside [1, 65 536], cols outside [1, 2047], pitch % 4 != 0, first + positions > pitch,
//     remaining < positions, remaining > 2^31 - 1, cells that are not 16-byte aligned, a map or an output that are not 4-byte aligned, a
//     negative count, a NULL pointer with positions > 0; positions == 0 launches nothing
//   - offsets into the planes and the matrix are 64-bit (65 536 planes of pitch 2^31 are 2^47 cells); a value is at most
//     remaining - i <= 2^31 - 1 and fits the int32 it becomes
//   - values are written with vector stores only; there is no inline assembly
#include <algorithm>

#include "memo_common.h"

using namespace memo;

namespace {

constexpr int kThreads = 256;
constexpr int kTP = 128;                  // positions per tile
constexpr int kTG = 64;                   // columns per tile
constexpr int kStride = kTP + 1;          // words per column in LDS: odd (see the header of memo_convert.hip)
constexpr int kQuads = kTP / 4;           // 16-byte loads per column and tile
constexpr int kLoads = kTG * kQuads / kThreads;  // 16-byte loads a lane has in flight: 8
constexpr int kMaxPlanes = 65536;
constexpr int kMaxCols = 2047;
constexpr int64_t kMaxRemaining = 0x7FFFFFFF;
static_assert(kStride % 2 == 1 && kTG * kQuads % kThreads == 0 && kTP % 32 == 0, "the lane layout of the load");

struct MergeArgs {
    const uint32_t *cells;    // plane 0 of the stack
    const int32_t *plane_of;  // cols entries
    int32_t *dap;
    int64_t pitch, first, positions, remaining;
    int planes;
    int cols;
    int ctiles;  // column tiles
};

__global__ __launch_bounds__(kThreads) void merge_dap_kernel(const MergeArgs A) {
    __shared__ uint32_t tile[kTG * kStride];
    const int64_t wg = blockIdx.x;
    const int ct = (int)(wg % A.ctiles);
    const int64_t t0 = (A.first / kTP + wg / A.ctiles) * kTP;  // the tile's first position in the plane
    const int c0 = ct * kTG, ng = min(kTG, A.cols - c0);       // its columns [c0, c0 + ng)
    const int64_t end = A.first + A.positions;
    const int32_t *map = A.plane_of + c0;
    if (t0 >= A.first && t0 + kTP <= end) {
        uint4 v[kLoads];
        int32_t m[kLoads];
        const int lane = threadIdx.x & 31, q_lo = lane & 7, g_lo = lane >> 3;
#pragma unroll
        for (int u = 0; u < kLoads; ++u) {
            const int grp = (u * kThreads + threadIdx.x) >> 5;  // 64 groups: 4 blocks of 8 quads x 16 blocks of 4 columns
            const int g = (grp >> 2) * 4 + g_lo;
            m[u] = g < ng ? map[g] : -1;
        }
#pragma unroll
        for (int u = 0; u < kLoads; ++u) {
            const int grp = (u * kThreads + threadIdx.x) >> 5;
            const int q = (grp & 3) * 8 + q_lo;
            if ((uint32_t)m[u] < (uint32_t)A.planes) v[u] = *reinterpret_cast<const uint4 *>(A.cells + (int64_t)m[u] * A.pitch + t0 + 4 * q);
        }
#pragma unroll
        for (int u = 0; u < kLoads; ++u) {
            const int grp = (u * kThreads + threadIdx.x) >> 5;
            const int q = (grp & 3) * 8 + q_lo, g = (grp >> 2) * 4 + g_lo;
            if (g < ng) {
                const uint4 w = (uint32_t)m[u] < (uint32_t)A.planes ? v[u] : make_uint4(0, 0, 0, 0);  // (no plane: nothing was loaded)
                uint32_t *d = tile + g * kStride + 4 * q;
                d[0] = w.x, d[1] = w.y, d[2] = w.z, d[3] = w.w;
            }
        }
    } else {
        for (int e = threadIdx.x; e < ng * kTP; e += kThreads) {
            const int g = e / kTP, q = e % kTP;
            const int64_t p = t0 + q;
            if (p >= A.first && p < end) {
                const int32_t plane = map[g];
                tile[g * kStride + q] = (uint32_t)plane < (uint32_t)A.planes ? A.cells[(int64_t)plane * A.pitch + p] : 0u;
            }
        }
    }
    __syncthreads();
    const int di = kThreads / ng, dg = kThreads % ng;
    int i = threadIdx.x / ng, g = threadIdx.x % ng;
    while (i < kTP) {
        const int64_t at = t0 + i - A.first;  // the row of the matrix
        if (at >= 0 && at < A.positions) {
            const uint32_t room = (uint32_t)(A.remaining - at);  // (1 .. 2^31 - 1)
            A.dap[at * A.cols + c0 + g] = (int32_t)min(tile[g * kStride + i], room);
        }
        i += di, g += dg;
        if (g >= ng) g -= ng, ++i;
    }
}

}  // namespace

extern "C" {

int32_t memo_merge_tile(void) { return kTP; }

int memo_merge_dap_dev(const uint32_t *d_cells, int64_t pitch, int32_t planes, const int32_t *d_plane_of, int32_t cols, int64_t first,
                       int64_t positions, int64_t remaining, int32_t *d_dap, int32_t device, void *stream) {
    if (planes < 1 || planes > kMaxPlanes) return fail(MEMO_EINVAL, "planes must be in [1, %d] (got %d)", kMaxPlanes, planes);
    if (cols < 1 || cols > kMaxCols) return fail(MEMO_EINVAL, "cols must be in [1, %d] (got %d)", kMaxCols, cols);
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
    if (reinterpret_cast<uintptr_t>(d_plane_of) & 3) return fail(MEMO_EINVAL, "d_plane_of must be 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_dap) & 3) return fail(MEMO_EINVAL, "d_dap must be 4-byte aligned");
    if (!positions) return MEMO_OK;
    if (!d_cells || !d_plane_of || !d_dap) return fail(MEMO_EINVAL, "d_cells, d_plane_of or d_dap is NULL");
    if (int rc = device_ok(device)) return rc;
    DeviceGuard guard(device);
    if (!guard.ok) return fail(MEMO_EHIP, "cannot select HIP device %d", device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    MergeArgs A = {};
    A.cells = d_cells, A.plane_of = d_plane_of, A.dap = d_dap;
    A.pitch = pitch, A.first = first, A.positions = positions, A.remaining = remaining;
    A.planes = planes, A.cols = cols;
    A.ctiles = (cols + kTG - 1) / kTG;
    const int64_t ptiles = (first + positions - 1) / kTP - first / kTP + 1;  // (at most 2^24 + 1, times at most 32 column tiles: fits grid.x)
    hipLaunchKernelGGL(merge_dap_kernel, dim3((unsigned)(ptiles * A.ctiles)), dim3(kThreads), 0, st, A);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    return MEMO_OK;
}

}  // extern "C"
