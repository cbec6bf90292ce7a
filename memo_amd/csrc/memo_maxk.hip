// memo_maxk.hip -- `memo maxk`: for every position of a window the longest k at which the k-mer starting there is still shared,
//     out[p - qs] = min( CAP, max( 0, min{ e_i - p : pred(a_i), p < s_i, qs < s_i < qe + CAP } ) )        uint32, CAP where no row bounds p
// with pred = (0 <= a < T) on a conservation index ("at least T genomes share it") or (a == G) on a membership index ("genome G holds
// it"): every k in one pass instead of one sweep per k.  No counterpart in the reference.  A row (s, e, a) with e >= s makes the k-mer
// at p absent exactly when p < s and p + k - 1 >= e, so the answer is a suffix minimum of row ends over row starts,
// minus p.  Rows with e < s take the formula literally (the result can be 0).
//
// Cells.  uint32 cell[L], relative to qs: ONE plane of memo_cells.h's layout (the identity ident = L - 1 + CAP and the saturation to
// [0, ident] are described there), so L is arbitrary: a pitch is never used.
//   1. begin   memo::cells_fill (memo_cells.hip): cell[] = ident, 16-byte stores (the last L % 4 cells one by one)
//   2. rows    maxk_rows_kernel: memo_cells.h's stream_rows over the three int64 columns (16 bytes a lane and load, kLoads loads of each
//              column in flight), and for
//              every row that passes the predicate and qs < s < qe + CAP:  atomicMin(&cell[min(s - 1 - qs, L - 1)], clamp(e - qs)),
//              no return value, device scope (a row with s >= qe bounds every position: cell L - 1).  A row whose clamp is ident is
//              the identity and is skipped.  Min is idempotent and commutative: row order, repeated rows and the cut into calls
//              do not matter, so unsorted rows are legal and a caller streams chunks.  Two ways (memo_debug_maxk_rows of the AB library):
//                way 0 (the product's)  wave-aggregated: the two rows of a lane are merged where they hit one cell, then a segmented min
//                                       over the lanes that hit the same cell (wave shuffles) leaves one atomic per run of equal cells
//                                       and wave -- the files are start-sorted, so neighbouring lanes hit neighbouring or equal cells
//                way 1                  one atomic per row
//              (DESIGN.md 10.5 has both times: equal where few rows are selected, 4.7 times apart where every row of config 3 is.)
//   3. finish  memo::cells_finish (memo_cells.hip) on the one plane: the tile minima, their suffix-min scan by one workgroup, and the
//              apply launch that writes out = cell > i ? min(cell - i, CAP) : 0 over the cell
//
// Conditions the code holds:
//   - no workgroup waits for another: no look-back, no flag in memory, no cooperative launch
//   - nothing is read outside the `rows` elements of each column or outside cell[0 .. L): a 16-byte load is of two rows that both exist
//     (a first row that is not 16-byte aligned and a last odd row are read alone), a tile that crosses L is taken cell by cell
//   - columns that are not 8-byte aligned, cells that are not 16-byte aligned, L > 2^31, CAP outside [1, 2^31 - 1], a window start
//     beyond +-2^61 are MEMO_EINVAL before any launch; L == 0 or rows == 0 launches nothing
//   - the columns take 16-byte loads when all three have the same alignment mod 16, else 8-byte loads (same kernel, same result)
//   - positions and row counts are 64-bit; a cell index and a cell value fit 32 bits by the limits above
//   - scratch: the tile minima only (4 bytes per kTile cells), owned by DevPtr; an allocation that fails is MEMO_EHIP with the bytes
//     asked for, and nothing stays allocated
//   - values are written with vector stores and vector atomics only; there is no inline assembly
#include "memo_cells.h"

using namespace memo;

namespace memo {
thread_local int g_maxk_rows_way = 0;  // 0 = wave-aggregated atomics, 1 = one atomic per row (memo_debug_maxk_rows)
thread_local int g_maxk_timed = 0;     // 1 = event pairs around the launches (memo_debug_maxk_times)
thread_local float g_maxk_ms[5] = {0.f, 0.f, 0.f, 0.f, 0.f};  // ... of the last such calls: fill, rows, tile minima, scan of them, apply
}

namespace {

constexpr int kThreads = kRowThreads;

struct RowArgs {
    Columns c;
    RowWindow w;
    int64_t arg;
    int mode;
    uint32_t *cell;
};

__device__ __forceinline__ void cell_min(uint32_t *cell, uint32_t j, uint32_t v) {
    (void)__hip_atomic_fetch_min(cell + j, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// way 0: one atomic per run of lanes with the same cell.  A lane takes the value of the lane d below it where both hit the same cell
// (d = 1, 2 .. 32): over a run of equal cells that is an inclusive min-scan, and the run's last lane holds the run's minimum.  Every
// value a lane takes belongs to its own cell, and a lane that is not its run's last has handed its value to the next one: right for
// any order of rows, fewest atomics for sorted ones.
__device__ __forceinline__ void cell_min_wave(uint32_t *cell, uint32_t j, uint32_t v) {
    if (!__ballot(j != kNone)) return;
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t oj = __shfl_up(j, d), ov = __shfl_up(v, d);
        if (lane >= d && oj == j) v = min(v, ov);
    }
    const uint32_t nj = __shfl_down(j, 1);
    if (j != kNone && (lane == 63 || nj != j)) cell_min(cell, j, v);
}

template <bool AGG>
struct RowMin {  // what stream_rows hands its rows to
    const RowArgs &A;
    __device__ __forceinline__ void bound(int64_t s, int64_t e, int64_t a, uint32_t &j, uint32_t &v) const {
        row_bound(A.w, A.mode ? a == A.arg : (a >= 0 && a < A.arg), s, e, j, v);
    }
    __device__ __forceinline__ void pair(const longlong2 &s, const longlong2 &e, const longlong2 &a) const {
        uint32_t jx, vx, jy, vy;
        bound(s.x, e.x, a.x, jx, vx);
        bound(s.y, e.y, a.y, jy, vy);
        if (AGG) {
            if (jx == jy) vy = min(vx, vy), jx = kNone;  // (both ignored: still ignored)
            cell_min_wave(A.cell, jx, vx);
            cell_min_wave(A.cell, jy, vy);
        } else {
            if (jx != kNone) cell_min(A.cell, jx, vx);
            if (jy != kNone) cell_min(A.cell, jy, vy);
        }
    }
    __device__ __forceinline__ void one(int64_t s, int64_t e, int64_t a) const {
        uint32_t j, v;
        bound(s, e, a, j, v);
        if (j != kNone) cell_min(A.cell, j, v);
    }
};

template <bool VEC, bool AGG>
__global__ __launch_bounds__(kThreads) void maxk_rows_kernel(const RowArgs A) {
    stream_rows<VEC>(A.c, RowMin<AGG>{A});
}

// what every entry point refuses before it looks at anything else
int check_cells(const uint32_t *d_cells, int64_t L, uint32_t cap) {
    if (int rc = check_window(L, cap)) return rc;
    return check_cell_pointer(d_cells, L);
}

template <bool VEC>
void launch_rows(const RowArgs &A, unsigned grid, hipStream_t st) {
    if (g_maxk_rows_way) hipLaunchKernelGGL((maxk_rows_kernel<VEC, false>), dim3(grid), dim3(kThreads), 0, st, A);
    else hipLaunchKernelGGL((maxk_rows_kernel<VEC, true>), dim3(grid), dim3(kThreads), 0, st, A);
}

}  // namespace

extern "C" {

int32_t memo_maxk_tile(void) { return kCellTile; }

int memo_maxk_begin_dev(uint32_t *d_cells, int64_t L, uint32_t cap, int32_t device, void *stream) {
    if (int rc = check_cells(d_cells, L, cap)) return rc;
    if (!L) return MEMO_OK;
    OnDevice on(device);
    if (on.rc) return on.rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    Laps laps(st, g_maxk_timed, g_maxk_ms);
    if (int rc = laps.start()) return rc;
    HIP_TRY(cells_fill(CellPlanes{d_cells, L, 0, 1, cap}, 1 << 16, st));
    if (int rc = laps.lap(0)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return MEMO_OK;
}

int memo_maxk_rows_dev(const int64_t *d_start, const int64_t *d_end, const int64_t *d_annot, uint64_t rows, int64_t qs, int64_t L,
                       uint32_t cap, int32_t mode, int64_t arg, uint32_t *d_cells, int32_t device, void *stream) {
    if (int rc = check_cells(d_cells, L, cap)) return rc;
    if (mode != 0 && mode != 1) return fail(MEMO_EINVAL, "mode must be 0 (0 <= annot < arg) or 1 (annot == arg)");
    if (qs < -kCoordLimit || qs > kCoordLimit) return fail(MEMO_EINVAL, "window start %lld is beyond +-2^61", (long long)qs);
    if (int rc = check_columns(d_start, d_end, d_annot, rows)) return rc;
    if (!L || !rows) return MEMO_OK;
    OnDevice on(device);
    if (on.rc) return on.rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    RowArgs A = {};
    bool vec;
    const unsigned grid = set_columns(A.c, d_start, d_end, d_annot, rows, vec, 1 << 16);
    A.w.set(qs, L, cap);
    A.mode = mode;
    A.arg = arg;
    A.cell = d_cells;
    Laps laps(st, g_maxk_timed, g_maxk_ms);
    if (int rc = laps.start()) return rc;
    if (vec) launch_rows<true>(A, grid, st);
    else launch_rows<false>(A, grid, st);
    HIP_TRY(hipGetLastError());
    if (int rc = laps.lap(1)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return MEMO_OK;
}

int memo_maxk_finish_dev(uint32_t *d_cells, int64_t L, uint32_t cap, int32_t device, void *stream) {
    if (int rc = check_cells(d_cells, L, cap)) return rc;
    if (!L) return MEMO_OK;
    OnDevice on(device);
    if (on.rc) return on.rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t ntiles = cell_tiles(L);
    DevPtr<uint32_t> mins;
    if (hipError_t err = mins.alloc((size_t)ntiles); err != hipSuccess)
        return fail(MEMO_EHIP, "hipMalloc(%zu bytes) for the tile minima of %lld positions: %s", (size_t)ntiles * sizeof(uint32_t), (long long)L,
                    hipGetErrorString(err));
    Laps laps(st, g_maxk_timed, g_maxk_ms);
    if (int rc = cells_finish(CellPlanes{d_cells, L, 0, 1, cap}, mins, st, laps, 2)) return rc;
    HIP_TRY(hipStreamSynchronize(st));  // (the tile minima go with this call)
    return MEMO_OK;
}

}  // extern "C"
