// memo_cells.hip -- the passes over planes of cells (memo_cells.h has the layout) that `memo maxk` and `memo lengths` share: maxk's
// cells are the one-plane case.  The plane is blockIdx.y (the scan: one workgroup per plane, in blockIdx.x); a plane's offset is
// plane x pitch, so with one plane the pitch is never used and only lengths needs it to be a multiple of 4.
//   cells_fill      cells_fill_kernel: [0, L) of every plane = ident, 16-byte stores (the last L % 4 cells one by one)
//   cells_carry_in  cells_carry_in_kernel: cell[g][L - 1] = clamp(carry[g] - qs) where a carry (int64 [planes], INT64_MAX: none) exists
//   cells_finish    three launches ordered by the stream, in place:
//                     cells_tile_min_kernel  the minimum of every tile of kCellTile cells
//                     cells_scan_kernel      one workgroup per plane: mins[t] <- min(mins[t + 1 ..]) (ident for the last tile), kScanRound
//                                            tiles a round from the right, the rounds chained by a register
//                     cells_apply_kernel     per tile the reverse inclusive min-scan (in the lane, wave shuffles, LDS across the waves)
//                                            combined with the tile's carry, then out = cell > i ? min(cell - i, CAP) : 0 over the cell
//
// Conditions the code holds:
//   - no workgroup waits for another: no look-back, no flag in memory, no cooperative launch
//   - nothing is read or written outside [0, L) of a plane: a 16-byte access is of four cells below L, a tile that crosses L is taken
//     cell by cell
//   - the caller has refused cells that are not 16-byte aligned, L > 2^31 and, with more than one plane, a pitch that is no multiple of 4
//   - values are written with vector stores only; there is no inline assembly
#include "memo_cells.h"

using namespace memo;

namespace {

constexpr int kThreads = 256;
constexpr int kPerLane = 8;                 // cells a lane of the scan holds: two 16-byte loads
constexpr int kTile = kThreads * kPerLane;  // cells per tile of the scan
static_assert(kTile == kCellTile, "memo_common.h names the tile");
constexpr int kScanThreads = 1024, kScanPerLane = 4;
constexpr int kScanRound = kScanThreads * kScanPerLane;  // tile minima one round of the scan takes
constexpr int64_t kMaxL = (int64_t)1 << 31;
constexpr uint32_t kMaxCap = 0x7FFFFFFFu;

// grid (.., planes): [0, L) of plane blockIdx.y = ident
__global__ __launch_bounds__(kThreads) void cells_fill_kernel(uint32_t *cells, int64_t L, int64_t pitch, uint32_t ident) {
    uint32_t *cell = cells + (int64_t)blockIdx.y * pitch;
    const int64_t n4 = L >> 2;
    const uint4 v = make_uint4(ident, ident, ident, ident);
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n4; i += (int64_t)gridDim.x * kThreads)
        reinterpret_cast<uint4 *>(cell)[i] = v;
    if (blockIdx.x == 0 && threadIdx.x < (L & 3)) cell[4 * n4 + threadIdx.x] = ident;
}

// cell[g][L - 1] = clamp(carry[g] - qs), after the fill (its own launch: the fill's workgroups are not ordered among themselves)
__global__ __launch_bounds__(kThreads) void cells_carry_in_kernel(uint32_t *cells, int64_t L, int64_t pitch, int n, uint32_t ident,
                                                                  const int64_t *carry, int64_t qs) {
    const int g = blockIdx.x * kThreads + threadIdx.x;
    if (g >= n) return;
    const int64_t e = carry[g];
    if (e == INT64_MAX) return;
    cells[(int64_t)g * pitch + L - 1] = e <= qs ? 0u : e >= qs + (int64_t)ident ? ident : (uint32_t)(e - qs);  // (|qs| <= 2^61: the sum cannot overflow, e - qs could)
}

// the kPerLane cells of a lane of tile t, cells at or past L as kNone
__device__ __forceinline__ void load_cells(const uint32_t *cell, int64_t L, int64_t t, uint32_t (&c)[kPerLane]) {
    const int64_t i0 = t * kTile + (int64_t)threadIdx.x * kPerLane;
    if (i0 + kPerLane <= L) {
        const uint4 lo = *reinterpret_cast<const uint4 *>(cell + i0), hi = *reinterpret_cast<const uint4 *>(cell + i0 + 4);
        c[0] = lo.x, c[1] = lo.y, c[2] = lo.z, c[3] = lo.w, c[4] = hi.x, c[5] = hi.y, c[6] = hi.z, c[7] = hi.w;
    } else {
#pragma unroll
        for (int q = 0; q < kPerLane; ++q) c[q] = i0 + q < L ? cell[i0 + q] : kNone;
    }
}

// the minimum over the lanes RIGHT of this one in the workgroup (kNone: none), and the workgroup's minimum.  wave_min: LDS [WAVES];
// all lanes of the workgroup call it; two barriers
template <int WAVES>
__device__ __forceinline__ uint32_t min_right_of(uint32_t mine, uint32_t *wave_min, uint32_t &all) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = mine;  // over this lane and the lanes of the wave right of it
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_down(inc, d);
        if (lane + d < 64) inc = min(inc, o);
    }
    uint32_t right = __shfl_down(inc, 1);
    if (lane == 63) right = kNone;
    if (lane == 0) wave_min[wave] = inc;
    __syncthreads();
    all = kNone;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        const uint32_t m = wave_min[w];
        all = min(all, m);
        if (w > wave) right = min(right, m);
    }
    __syncthreads();  // (the next call writes wave_min again)
    return right;
}

// grid (ntiles, planes): the minimum of tile blockIdx.x of plane blockIdx.y
__global__ __launch_bounds__(kThreads) void cells_tile_min_kernel(const uint32_t *cells, int64_t L, int64_t pitch, uint32_t *mins) {
    __shared__ uint32_t wave_min[kThreads / 64];
    uint32_t c[kPerLane];
    load_cells(cells + (int64_t)blockIdx.y * pitch, L, blockIdx.x, c);
    uint32_t m = c[0];
#pragma unroll
    for (int q = 1; q < kPerLane; ++q) m = min(m, c[q]);
    uint32_t all;
    (void)min_right_of<kThreads / 64>(m, wave_min, all);
    if (threadIdx.x == 0) mins[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = all;
}

// grid (planes): plane blockIdx.x's mins[t] <- min(mins[t + 1 .. ntiles)), ident for the last tile; rounds of kScanRound tiles from the right
__global__ __launch_bounds__(kScanThreads) void cells_scan_kernel(uint32_t *all_mins, int64_t ntiles, uint32_t ident) {
    __shared__ uint32_t wave_min[kScanThreads / 64];
    uint32_t *mins = all_mins + (int64_t)blockIdx.x * ntiles;
    uint32_t carry = ident;  // the minimum of every tile right of this round
    for (int64_t hi = ntiles; hi > 0; hi -= kScanRound) {
        const int64_t i0 = hi - kScanRound + (int64_t)threadIdx.x * kScanPerLane;  // (may be negative in the last round)
        uint32_t m[kScanPerLane];
#pragma unroll
        for (int q = 0; q < kScanPerLane; ++q) m[q] = i0 + q >= 0 ? mins[i0 + q] : kNone;
        uint32_t mine = m[0];
#pragma unroll
        for (int q = 1; q < kScanPerLane; ++q) mine = min(mine, m[q]);
        uint32_t all;
        uint32_t right = min(min_right_of<kScanThreads / 64>(mine, wave_min, all), carry);
#pragma unroll
        for (int q = kScanPerLane - 1; q >= 0; --q) {
            if (i0 + q >= 0) mins[i0 + q] = right;
            right = min(right, m[q]);
        }
        carry = min(carry, all);
    }
}

// grid (ntiles, planes)
__global__ __launch_bounds__(kThreads) void cells_apply_kernel(uint32_t *cells, int64_t L, int64_t pitch, const uint32_t *carry, uint32_t cap) {
    __shared__ uint32_t wave_min[kThreads / 64];
    uint32_t *cell = cells + (int64_t)blockIdx.y * pitch;
    uint32_t c[kPerLane];
    load_cells(cell, L, blockIdx.x, c);
#pragma unroll
    for (int q = kPerLane - 2; q >= 0; --q) c[q] = min(c[q], c[q + 1]);
    uint32_t all;
    const uint32_t right = min(min_right_of<kThreads / 64>(c[0], wave_min, all), carry[(int64_t)blockIdx.y * gridDim.x + blockIdx.x]);
    const int64_t i0 = (int64_t)blockIdx.x * kTile + (int64_t)threadIdx.x * kPerLane;
    uint32_t out[kPerLane];
#pragma unroll
    for (int q = 0; q < kPerLane; ++q) {
        const uint32_t bound = min(c[q], right), i = (uint32_t)(i0 + q);  // (i < L <= 2^31)
        out[q] = bound > i ? min(bound - i, cap) : 0u;
    }
    if (i0 + kPerLane <= L) {
        *reinterpret_cast<uint4 *>(cell + i0) = make_uint4(out[0], out[1], out[2], out[3]);
        *reinterpret_cast<uint4 *>(cell + i0 + 4) = make_uint4(out[4], out[5], out[6], out[7]);
    } else {
#pragma unroll
        for (int q = 0; q < kPerLane; ++q)
            if (i0 + q < L) cell[i0 + q] = out[q];
    }
}

}  // namespace

int memo::check_window(int64_t L, uint32_t cap) {
    if (L < 0 || L > kMaxL) return fail(MEMO_EINVAL, "a window of %lld positions: L must be in [0, 2^31]", (long long)L);
    if (cap < 1 || cap > kMaxCap) return fail(MEMO_EINVAL, "cap must be in [1, 2^31 - 1] (got %u)", cap);
    return MEMO_OK;
}

int memo::check_cell_pointer(const uint32_t *d_cells, int64_t L) {
    if (reinterpret_cast<uintptr_t>(d_cells) & 15) return fail(MEMO_EINVAL, "d_cells must be 16-byte aligned");
    if (L && !d_cells) return fail(MEMO_EINVAL, "d_cells is NULL");
    return MEMO_OK;
}

hipError_t memo::cells_fill(const CellPlanes &P, int64_t most, hipStream_t st) {
    const int64_t wgs = std::max<int64_t>(1, std::min<int64_t>(((P.L >> 2) + kThreads - 1) / kThreads, most));
    hipLaunchKernelGGL(cells_fill_kernel, dim3((unsigned)wgs, (unsigned)P.planes), dim3(kThreads), 0, st, P.cells, P.L, P.pitch, P.ident());
    return hipGetLastError();
}

hipError_t memo::cells_carry_in(const CellPlanes &P, const int64_t *d_carry, int64_t qs, hipStream_t st) {
    hipLaunchKernelGGL(cells_carry_in_kernel, dim3((unsigned)((P.planes + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, P.cells, P.L, P.pitch,
                       P.planes, P.ident(), d_carry, qs);
    return hipGetLastError();
}

int memo::cells_finish(const CellPlanes &P, uint32_t *d_mins, hipStream_t st, Laps &laps, int slot) {
    const int64_t ntiles = cell_tiles(P.L);  // (at most 2^20: fits grid.x; the planes, at most 2048, fit grid.y)
    const dim3 tiles((unsigned)ntiles, (unsigned)P.planes);
    if (int rc = laps.start()) return rc;
    hipLaunchKernelGGL(cells_tile_min_kernel, tiles, dim3(kThreads), 0, st, P.cells, P.L, P.pitch, d_mins);
    HIP_TRY(hipGetLastError());
    if (int rc = laps.lap(slot)) return rc;
    hipLaunchKernelGGL(cells_scan_kernel, dim3((unsigned)P.planes), dim3(kScanThreads), 0, st, d_mins, ntiles, P.ident());
    HIP_TRY(hipGetLastError());
    if (int rc = laps.lap(slot + 1)) return rc;
    hipLaunchKernelGGL(cells_apply_kernel, tiles, dim3(kThreads), 0, st, P.cells, P.L, P.pitch, d_mins, P.cap);
    HIP_TRY(hipGetLastError());
    return laps.lap(slot + 2);
}
