// memo_add.hip -- `memo add`: the row builder's matrix of N + m genomes from two sources.  The old genomes' columns are read back from the
// membership index as genome-major uint32 planes (memo_lengths.hip: cell[g][p]), as `memo convert` reads them; the new genomes' columns
// are matching statistics computed now, position-major int32 rows [positions][new_cols] (memo_ms.hip: memo_ms_rows_dev).  Both become
// ONE position-major int32 matrix of W = N - 1 + new_cols columns (memo_dap.hip reads it), clipped at the end of the record:
//     dap[i][c] = min( cell[c + 1][first + i], remaining - i )                  0 <= c < N - 1         0 <= i < positions
//     dap[i][c] = min( (uint32) new[i][c - (N - 1)], remaining - i )            N - 1 <= c < W
// Plane 0, the pivot, is not read: a DAP has no column for it.  No counterpart in the reference.
//
// add_dap_kernel is convert_dap_kernel (memo_convert.hip, whose header gives the bank argument) over the COMBINED column space [0, W):
// a workgroup of 256 lanes takes a tile of kTP = 128 positions x kTG = 64 columns, and a tile holds old columns, new columns or both,
// staged through one LDS tile, so that an output row segment is written in one contiguous run whatever (N - 1) mod 64 is.  Position
// tiles lie at multiples of kTP of the PLANE (not of `first`).  The workgroup index is position tile * column tiles + column tile.
//   load   old columns of a whole tile: every lane holds up to 8 uint4 (4 neighbouring positions of one genome each), all in flight
//          before the first goes to LDS; a 32-lane group is 8 quads x 4 genomes.
//          old columns of a tile that crosses `first` or `first + positions`: element by element, 32 neighbouring lanes on 32
//          neighbouring positions of one genome; nothing outside [first, first + positions) is read.
//          new columns (either kind of tile): the column index fastest across lanes, element e = q * nn + j (nn new columns in this tile):
//          lane t takes e = t, t + 256 ...; a row's nn values are one contiguous run of d_new, and with nn = new_cols (the whole of the
//          new columns in one tile) so is the tile's whole piece of d_new.  Rows outside [0, positions) are not read.  (q, j) advance by
//          (256 / nn, 256 % nn) with one carry: one division per lane and tile.
//   LDS    uint32 tile[kTG][kStride], kStride = kTP + 1 = 129 words (33 024 bytes), column-major as in convert_dap_kernel: the odd
//          stride spreads the old columns' quad stores and the read side over the banks as its header shows.  The new columns' store of
//          element (q, j) goes to word (no + j) * 129 + q: 32 neighbouring j per group are 32 banks (129 mod 32 = 1); where a group runs
//          over the end of one row's columns into the next row's it is 2-way at most.
//   store  the tile's output laid end to end, element f = i * ng + g (ng columns in this tile): lane t takes f = t, t + 256 ...; plain
//          4-byte stores.
//
// Conditions the code holds:
//   - no workgroup waits for another: no look-back, no flag in memory, no cooperative launch
//   - nothing is read outside [first, first + positions) of planes 1 .. N - 1; plane 0 and the cells outside that range are never read
//   - nothing is read outside d_new[0 .. positions * new_cols)
//   - nothing is written outside positions * W integers, and every one of them is written once
//   - an old column of a tile that crosses either edge is taken element by element
//   - MEMO_EINVAL before any launch: N outside [2, 2047], new_cols outside [1, 2047], W > 2047, pitch % 4 != 0, first + positions > pitch,
//     remaining < positions, remaining > 2^31 - 1, cells that are not 16-byte aligned, new rows or an output that are not 4-byte aligned,
//     a negative count, a NULL pointer with positions > 0; positions == 0 launches nothing
//   - offsets into the planes, the new rows and the matrix are 64-bit; a value is at most remaining - i <= 2^31 - 1 and fits the int32
//     it becomes
//   - values are written with vector stores only; there is no inline assembly
#include <algorithm>

#include "memo_common.h"

using namespace memo;

namespace {

constexpr int kThreads = 256;
constexpr int kTP = 128;                  // positions per tile
constexpr int kTG = 64;                   // columns per tile
constexpr int kStride = kTP + 1;          // words per column in LDS: odd (see the header of memo_convert.hip)
constexpr int kQuads = kTP / 4;           // 16-byte loads per genome and tile
constexpr int kLoads = kTG * kQuads / kThreads;  // 16-byte loads a lane has in flight: 8
constexpr int kMaxWidth = 2047;           // columns of the matrix, and each of its two parts
constexpr int64_t kMaxRemaining = 0x7FFFFFFF;
static_assert(kStride % 2 == 1 && kTG * kQuads % kThreads == 0 && kTP % 32 == 0, "the lane layout of the load");

struct AddArgs {
    const uint32_t *cells;  // plane 0
    const int32_t *fresh;   // the new columns' rows
    int32_t *dap;
    int64_t pitch, first, positions, remaining;
    int old_cols;  // N - 1
    int new_cols;
    int cols;      // W
    int ctiles;    // column tiles
};

__global__ __launch_bounds__(kThreads) void add_dap_kernel(const AddArgs A) {
    __shared__ uint32_t tile[kTG * kStride];
    const int64_t wg = blockIdx.x;
    const int ct = (int)(wg % A.ctiles);
    const int64_t t0 = (A.first / kTP + wg / A.ctiles) * kTP;  // the tile's first position in the plane
    const int c0 = ct * kTG, ng = min(kTG, A.cols - c0);       // its columns [c0, c0 + ng)
    const int no = max(0, min(ng, A.old_cols - c0));           // the first `no` of them are old, the other nn new
    const int nn = ng - no;
    const int64_t end = A.first + A.positions;
    if (no > 0) {
        const uint32_t *plane = A.cells + (int64_t)(1 + c0) * A.pitch;  // the plane of column c0
        if (t0 >= A.first && t0 + kTP <= end) {
            uint4 v[kLoads];
            const int lane = threadIdx.x & 31, q_lo = lane & 7, g_lo = lane >> 3;
#pragma unroll
            for (int u = 0; u < kLoads; ++u) {
                const int grp = (u * kThreads + threadIdx.x) >> 5;  // 64 groups: 4 blocks of 8 quads x 16 blocks of 4 genomes
                const int q = (grp & 3) * 8 + q_lo, g = (grp >> 2) * 4 + g_lo;
                if (g < no) v[u] = *reinterpret_cast<const uint4 *>(plane + (int64_t)g * A.pitch + t0 + 4 * q);
            }
#pragma unroll
            for (int u = 0; u < kLoads; ++u) {
                const int grp = (u * kThreads + threadIdx.x) >> 5;
                const int q = (grp & 3) * 8 + q_lo, g = (grp >> 2) * 4 + g_lo;
                if (g < no) {
                    uint32_t *d = tile + g * kStride + 4 * q;
                    d[0] = v[u].x, d[1] = v[u].y, d[2] = v[u].z, d[3] = v[u].w;
                }
            }
        } else {
            for (int e = threadIdx.x; e < no * kTP; e += kThreads) {
                const int g = e / kTP, q = e % kTP;
                const int64_t p = t0 + q;
                if (p >= A.first && p < end) tile[g * kStride + q] = plane[(int64_t)g * A.pitch + p];
            }
        }
    }
    if (nn > 0) {
        const int j0 = c0 + no - A.old_cols;  // the tile's first new column
        const int dq = kThreads / nn, dj = kThreads % nn;
        int q = threadIdx.x / nn, j = threadIdx.x % nn;
        while (q < kTP) {
            const int64_t at = t0 + q - A.first;  // the row of both matrices
            if (at >= 0 && at < A.positions) tile[(no + j) * kStride + q] = (uint32_t)A.fresh[at * A.new_cols + j0 + j];
            q += dq, j += dj;
            if (j >= nn) j -= nn, ++q;
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

int32_t memo_add_tile(void) { return kTP; }

int memo_add_dap_dev(const uint32_t *d_cells, int64_t pitch, int32_t num_docs, int64_t first, int64_t positions, int64_t remaining,
                     const int32_t *d_new, int32_t new_cols, int32_t *d_dap, int32_t device, void *stream) {
    if (num_docs < 2 || num_docs > kMaxWidth) return fail(MEMO_EINVAL, "num_docs must be in [2, %d] (got %d)", kMaxWidth, num_docs);
    if (new_cols < 1 || new_cols > kMaxWidth) return fail(MEMO_EINVAL, "new_cols must be in [1, %d] (got %d)", kMaxWidth, new_cols);
    if (num_docs - 1 + new_cols > kMaxWidth)
        return fail(MEMO_EINVAL, "num_docs - 1 + new_cols = %d columns: the limit is %d", num_docs - 1 + new_cols, kMaxWidth);
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
    if (reinterpret_cast<uintptr_t>(d_new) & 3) return fail(MEMO_EINVAL, "d_new must be 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_dap) & 3) return fail(MEMO_EINVAL, "d_dap must be 4-byte aligned");
    if (!positions) return MEMO_OK;
    if (!d_cells || !d_new || !d_dap) return fail(MEMO_EINVAL, "d_cells, d_new or d_dap is NULL");
    if (int rc = device_ok(device)) return rc;
    DeviceGuard guard(device);
    if (!guard.ok) return fail(MEMO_EHIP, "cannot select HIP device %d", device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    AddArgs A = {};
    A.cells = d_cells, A.fresh = d_new, A.dap = d_dap;
    A.pitch = pitch, A.first = first, A.positions = positions, A.remaining = remaining;
    A.old_cols = num_docs - 1, A.new_cols = new_cols;
    A.cols = A.old_cols + new_cols;
    A.ctiles = (A.cols + kTG - 1) / kTG;
    const int64_t ptiles = (first + positions - 1) / kTP - first / kTP + 1;  // (at most 2^24 + 1, times at most 32 column tiles: fits grid.x)
    hipLaunchKernelGGL(add_dap_kernel, dim3((unsigned)(ptiles * A.ctiles)), dim3(kThreads), 0, st, A);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    return MEMO_OK;
}

}  // extern "C"
