// memo_convert.hip -- `memo convert`: the step between the planes of `memo lengths` and the row builder of `memo index`.  A finished slice
// of genome-major uint32 planes (memo_lengths.hip: cell[g][p], how far genome g matches the pivot from position p) becomes the
// position-major int32 matrix the row builder reads (memo_dap.hip: one row per position, one column per non-pivot genome), clipped at
// the end of the record:
//     dap[i][g - 1] = min( cell[g][first + i], remaining - i )        0 <= i < positions, 1 <= g < N
// Plane 0, the pivot, is not read: a DAP has no column for it.  No counterpart in the reference.
//
// convert_dap_kernel is a transposition through LDS.  A workgroup of 256 lanes takes a tile of kTP = 128 positions x kTG = 64 genomes.
// Position tiles lie at multiples of kTP of the PLANE (not of `first`): the planes are 16-byte aligned and pitch % 4 == 0, so a whole
// tile loads with 16-byte loads whatever `first` is.  The workgroup index is position tile * genome tiles + genome tile: the workgroups
// that write the pieces of one output row run side by side.
//   load   a whole tile: every lane holds 8 uint4 (4 neighbouring positions of one genome each), all in flight before the first goes to
//          LDS.  A 32-lane group is 8 quads x 4 genomes: 128 bytes in a row from each of four planes.
//          a tile that crosses `first` or `first + positions`: element by element, 32 neighbouring lanes on 32 neighbouring positions of one
//          genome, nothing outside [first, first + positions) is read.  Genomes past N - 1 are skipped in both forms.
//   LDS    uint32 tile[kTG][kStride], kStride = kTP + 1 = 129 words (33 024 bytes).  The stride is odd, so both sides spread over the banks
//          (64 banks of 4 bytes; a ds_write_b32 and a ds_read_b32 are served in two groups of 32 lanes over (a / 4) mod 32):
//            the store of dword j of a quad: word = g * 129 + 4 q + j with 8 q and 4 g per group -- g * 129 mod 4 tells the four
//              genomes apart, 4 q the eight quads: 32 banks (four ds_write_b32 per uint4: a 16-byte store would need a stride that is a
//              multiple of 4 words, which puts the read side 4-way on a bank)
//            the read of a run of genomes at position i: word = g * 129 + i, 32 neighbouring g per group: 32 banks.  Where a group runs over
//              the end of one position's genomes into the next position's it is 2-way at most.
//   store  the tile's output laid end to end, element f = i * ng + g (ng genomes in this tile): lane t takes f = t, t + 256 ...  A full
//          genome tile writes 256 bytes in a row per position and wave; a matrix of fewer than 64 columns is written as one contiguous
//          run.  Plain 4-byte stores: an output row starts at 4 (N - 1) i bytes, 16-byte aligned for some N only.  (i, g) advance by
//          (256 / ng, 256 % ng) with one carry: one division per lane and tile.
//
// Conditions the code holds:
//   - no workgroup waits for another: no look-back, no flag in memory, no cooperative launch
//   - nothing is read outside [first, first + positions) of planes 1 .. N - 1; plane 0 and the cells outside that range are never read
//   - nothing is written outside positions * (N - 1) integers
//   - a tile that crosses either edge is taken element by element
//   - MEMO_EINVAL before any launch: N outside [2, 2048], pitch % 4 != 0, first + positions > pitch, remaining < positions,
//     remaining > 2^31 - 1, cells that are not 16-byte aligned, an output that is not 4-byte aligned, a negative count, a NULL pointer
//     with positions > 0; positions == 0 launches nothing
//   - offsets into the planes and the matrix are 64-bit; a value is at most remaining - i <= 2^31 - 1 and fits the int32 it becomes
//   - values are written with vector stores only; there is no inline assembly
#include <algorithm>

#include "memo_common.h"

using namespace memo;

namespace {

constexpr int kThreads = 256;
constexpr int kTP = 128;                  // positions per tile
constexpr int kTG = 64;                   // genomes per tile
constexpr int kStride = kTP + 1;          // words per genome in LDS: odd (see the header)
constexpr int kQuads = kTP / 4;           // 16-byte loads per genome and tile
constexpr int kLoads = kTG * kQuads / kThreads;  // 16-byte loads a lane has in flight: 8
constexpr int kMaxDocs = 2048;
constexpr int64_t kMaxRemaining = 0x7FFFFFFF;
static_assert(kStride % 2 == 1 && kTG * kQuads % kThreads == 0 && kTP % 32 == 0, "the lane layout of the load");

struct ConvertArgs {
    const uint32_t *cells;  // plane 0
    int32_t *dap;
    int64_t pitch, first, positions, remaining;
    int cols;    // N - 1
    int gtiles;  // genome tiles
};

__global__ __launch_bounds__(kThreads) void convert_dap_kernel(const ConvertArgs A) {
    __shared__ uint32_t tile[kTG * kStride];
    const int64_t wg = blockIdx.x;
    const int gt = (int)(wg % A.gtiles);
    const int64_t t0 = (A.first / kTP + wg / A.gtiles) * kTP;  // the tile's first position in the plane
    const int c0 = gt * kTG, ng = min(kTG, A.cols - c0);       // its columns [c0, c0 + ng)
    const int64_t end = A.first + A.positions;
    const uint32_t *plane = A.cells + (int64_t)(1 + c0) * A.pitch;  // the plane of column c0
    if (t0 >= A.first && t0 + kTP <= end) {
        uint4 v[kLoads];
        const int lane = threadIdx.x & 31, q_lo = lane & 7, g_lo = lane >> 3;
#pragma unroll
        for (int u = 0; u < kLoads; ++u) {
            const int grp = (u * kThreads + threadIdx.x) >> 5;  // 64 groups: 4 blocks of 8 quads x 16 blocks of 4 genomes
            const int q = (grp & 3) * 8 + q_lo, g = (grp >> 2) * 4 + g_lo;
            if (g < ng) v[u] = *reinterpret_cast<const uint4 *>(plane + (int64_t)g * A.pitch + t0 + 4 * q);
        }
#pragma unroll
        for (int u = 0; u < kLoads; ++u) {
            const int grp = (u * kThreads + threadIdx.x) >> 5;
            const int q = (grp & 3) * 8 + q_lo, g = (grp >> 2) * 4 + g_lo;
            if (g < ng) {
                uint32_t *d = tile + g * kStride + 4 * q;
                d[0] = v[u].x, d[1] = v[u].y, d[2] = v[u].z, d[3] = v[u].w;
            }
        }
    } else {
        for (int e = threadIdx.x; e < ng * kTP; e += kThreads) {
            const int g = e / kTP, q = e % kTP;
            const int64_t p = t0 + q;
            if (p >= A.first && p < end) tile[g * kStride + q] = plane[(int64_t)g * A.pitch + p];
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

int32_t memo_convert_tile(void) { return kTP; }

int memo_convert_dap_dev(const uint32_t *d_cells, int64_t pitch, int32_t num_docs, int64_t first, int64_t positions, int64_t remaining,
                         int32_t *d_dap, int32_t device, void *stream) {
    if (num_docs < 2 || num_docs > kMaxDocs) return fail(MEMO_EINVAL, "num_docs must be in [2, %d] (got %d)", kMaxDocs, num_docs);
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
    if (reinterpret_cast<uintptr_t>(d_dap) & 3) return fail(MEMO_EINVAL, "d_dap must be 4-byte aligned");
    if (!positions) return MEMO_OK;
    if (!d_cells || !d_dap) return fail(MEMO_EINVAL, "d_cells or d_dap is NULL");
    if (int rc = device_ok(device)) return rc;
    DeviceGuard guard(device);
    if (!guard.ok) return fail(MEMO_EHIP, "cannot select HIP device %d", device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    ConvertArgs A = {};
    A.cells = d_cells, A.dap = d_dap;
    A.pitch = pitch, A.first = first, A.positions = positions, A.remaining = remaining;
    A.cols = num_docs - 1;
    A.gtiles = (A.cols + kTG - 1) / kTG;
    const int64_t ptiles = (first + positions - 1) / kTP - first / kTP + 1;  // (at most 2^24 + 1, times at most 32 genome tiles: fits grid.x)
    hipLaunchKernelGGL(convert_dap_kernel, dim3((unsigned)(ptiles * A.gtiles)), dim3(kThreads), 0, st, A);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    return MEMO_OK;
}

}  // extern "C"
