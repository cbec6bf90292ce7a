// memo_maxk.hip -- `memo maxk`: for every position of a window the longest k at which the k-mer starting there is still shared,
//     out[p - qs] = min( CAP, max( 0, min{ e_i - p : pred(a_i), p < s_i, qs < s_i < qe + CAP } ) )        uint32, CAP where no row bounds p
// with pred = (0 <= a < T) on a conservation index ("at least T genomes share it") or (a == G) on a membership index ("genome G holds
// it"): every k in one pass instead of one sweep per k.  No counterpart in the reference.  A row (s, e, a) with e >= s makes the k-mer
// at p absent exactly when p < s and p + k - 1 >= e, so the answer is a suffix minimum of row ends over row starts,
// minus p.  Rows with e < s take the formula literally (the result can be 0).
//
// Cells.  uint32 cell[L], relative to qs.  The identity is ident = L - 1 + CAP (L <= 2^31 and CAP < 2^31: below 2^32); every value is
// saturated to [0, ident], which is exact: a bound at or above ident yields CAP at every position.
//   1. begin   maxk_fill_kernel: cell[] = ident, 16-byte stores (the last L % 4 cells one by one)
//   2. rows    maxk_rows_kernel: streams the three int64 columns, 16 bytes a lane and load, kLoads loads of each column in flight, and for
//              every row that passes the predicate and qs < s < qe + CAP:  atomicMin(&cell[min(s - 1 - qs, L - 1)], clamp(e - qs)),
//              no return value, device scope (a row with s >= qe bounds every position: cell L - 1).  A row whose clamp is ident is
//              the identity and is skipped.  Min is idempotent and commutative: row order, repeated rows and the cut into calls
//              do not matter, so unsorted rows are legal and a caller streams chunks.  Two ways (memo_debug_maxk_rows of the AB library):
//                way 0 (the product's)  wave-aggregated: the two rows of a lane are merged where they hit one cell, then a segmented min
//                                       over the lanes that hit the same cell (wave shuffles) leaves one atomic per run of equal cells
//                                       and wave -- the files are start-sorted, so neighbouring lanes hit neighbouring or equal cells
//                way 1                  one atomic per row
//              (DESIGN.md 10.5 has both times: equal where few rows are selected, 4.7 times apart where every row of config 3 is.)
//   3. finish  three launches ordered by the stream, in place:
//                maxk_tile_min_kernel   the minimum of every tile of kTile cells
//                scan_tile_mins         ONE workgroup: mins[t] <- min(mins[t + 1 ..]) (ident for the last tile), kScanRound tiles a round
//                                       from the right, the rounds chained by a register
//                maxk_apply_kernel      per tile the reverse inclusive min-scan (in the lane, wave shuffles, LDS across the waves) combined
//                                       with the tile's carry, then out = cell > i ? min(cell - i, CAP) : 0 written over the cell
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
#include <algorithm>

#include "memo_common.h"

using namespace memo;

namespace memo {
thread_local int g_maxk_rows_way = 0;  // 0 = wave-aggregated atomics, 1 = one atomic per row (memo_debug_maxk_rows)
thread_local int g_maxk_timed = 0;     // 1 = event pairs around the launches (memo_debug_maxk_times)
thread_local float g_maxk_ms[5] = {0.f, 0.f, 0.f, 0.f, 0.f};  // ... of the last such calls: fill, rows, tile minima, scan of them, apply
}

namespace {

constexpr int kThreads = 256;
constexpr int kPerLane = 8;                   // cells a lane of the scan holds: two 16-byte loads
constexpr int kTile = kThreads * kPerLane;    // cells per tile of the scan
constexpr int kScanThreads = 1024, kScanPerLane = 4;
constexpr int kScanRound = kScanThreads * kScanPerLane;  // tile minima one round of scan_tile_mins takes
constexpr int kLoads = 4;                     // 16-byte loads of each column a lane has in flight
constexpr int64_t kPairsPerWg = (int64_t)kThreads * kLoads;  // row pairs a workgroup takes at a time
constexpr uint32_t kNone = 0xFFFFFFFFu;       // above every cell value; as a cell index: no cell
constexpr int64_t kMaxL = (int64_t)1 << 31;
constexpr uint32_t kMaxCap = 0x7FFFFFFFu;

struct RowArgs {
    const int64_t *s, *e, *a;
    uint64_t rows;
    int64_t head;    // rows before the first 16-byte pair (0 or 1)
    int64_t npairs;  // 16-byte pairs behind them
    int64_t qs, s_end, e_hi;  // s_end = qs + L + CAP (a start at or past it is ignored), e_hi = qs + ident (an end at or past it is ident)
    int64_t arg;
    uint32_t last, ident;  // last = L - 1
    int mode;
    uint32_t *cell;
};

// the cell and value of a row; cell kNone: the row is ignored
__device__ __forceinline__ void row_bound(const RowArgs &A, int64_t s, int64_t e, int64_t a, uint32_t &j, uint32_t &v) {
    const bool pred = A.mode ? a == A.arg : (a >= 0 && a < A.arg);
    j = kNone, v = kNone;
    if (!pred || s <= A.qs || s >= A.s_end) return;
    v = e <= A.qs ? 0u : e >= A.e_hi ? A.ident : (uint32_t)(e - A.qs);
    if (v >= A.ident) return;  // the identity
    const uint64_t d = (uint64_t)(s - A.qs - 1);
    j = d < A.last ? (uint32_t)d : A.last;
}

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

template <bool VEC, bool AGG>
__global__ __launch_bounds__(kThreads) void maxk_rows_kernel(const RowArgs A) {
    const int64_t nchunks = (A.npairs + kPairsPerWg - 1) / kPairsPerWg;
    for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const int64_t p0 = c * kPairsPerWg + threadIdx.x;
        longlong2 s[kLoads], e[kLoads], a[kLoads];
#pragma unroll
        for (int u = 0; u < kLoads; ++u) {
            const int64_t p = p0 + (int64_t)u * kThreads, r = A.head + 2 * p;
            // (a pair past the end: a start that no window takes)
            s[u] = e[u] = a[u] = make_longlong2(INT64_MIN, INT64_MIN);
            if (p < A.npairs) {
                if (VEC) {
                    s[u] = *reinterpret_cast<const longlong2 *>(A.s + r);
                    e[u] = *reinterpret_cast<const longlong2 *>(A.e + r);
                    a[u] = *reinterpret_cast<const longlong2 *>(A.a + r);
                } else {
                    s[u] = make_longlong2(A.s[r], A.s[r + 1]);
                    e[u] = make_longlong2(A.e[r], A.e[r + 1]);
                    a[u] = make_longlong2(A.a[r], A.a[r + 1]);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kLoads; ++u) {
            uint32_t jx, vx, jy, vy;
            row_bound(A, s[u].x, e[u].x, a[u].x, jx, vx);
            row_bound(A, s[u].y, e[u].y, a[u].y, jy, vy);
            if (AGG) {
                if (jx == jy) vy = min(vx, vy), jx = kNone;  // (both ignored: still ignored)
                cell_min_wave(A.cell, jx, vx);
                cell_min_wave(A.cell, jy, vy);
            } else {
                if (jx != kNone) cell_min(A.cell, jx, vx);
                if (jy != kNone) cell_min(A.cell, jy, vy);
            }
        }
    }
    // the rows outside the pairs, one lane each: the first row of columns that start 8 bytes off a 16-byte line, the last odd row
    if (blockIdx.x == 0 && threadIdx.x < 2) {
        const uint64_t behind = (uint64_t)(A.head + 2 * A.npairs);
        const bool first = threadIdx.x == 0;
        if (first ? A.head == 1 : behind < A.rows) {
            const uint64_t r = first ? 0 : behind;
            uint32_t j, v;
            row_bound(A, A.s[r], A.e[r], A.a[r], j, v);
            if (j != kNone) cell_min(A.cell, j, v);
        }
    }
}

__global__ __launch_bounds__(kThreads) void maxk_fill_kernel(uint32_t *cell, int64_t L, uint32_t ident) {
    const int64_t n4 = L >> 2;
    const uint4 v = make_uint4(ident, ident, ident, ident);
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n4; i += (int64_t)gridDim.x * kThreads)
        reinterpret_cast<uint4 *>(cell)[i] = v;
    if (blockIdx.x == 0 && threadIdx.x < (L & 3)) cell[4 * n4 + threadIdx.x] = ident;
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

__global__ __launch_bounds__(kThreads) void maxk_tile_min_kernel(const uint32_t *cell, int64_t L, uint32_t *mins) {
    __shared__ uint32_t wave_min[kThreads / 64];
    uint32_t c[kPerLane];
    load_cells(cell, L, blockIdx.x, c);
    uint32_t m = c[0];
#pragma unroll
    for (int q = 1; q < kPerLane; ++q) m = min(m, c[q]);
    uint32_t all;
    (void)min_right_of<kThreads / 64>(m, wave_min, all);
    if (threadIdx.x == 0) mins[blockIdx.x] = all;
}

// mins[t] <- min(mins[t + 1 .. ntiles)), ident for the last tile: one workgroup, rounds of kScanRound tiles from the right
__global__ __launch_bounds__(kScanThreads) void scan_tile_mins(uint32_t *mins, int64_t ntiles, uint32_t ident) {
    __shared__ uint32_t wave_min[kScanThreads / 64];
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

__global__ __launch_bounds__(kThreads) void maxk_apply_kernel(uint32_t *cell, int64_t L, const uint32_t *carry, uint32_t cap) {
    __shared__ uint32_t wave_min[kThreads / 64];
    uint32_t c[kPerLane];
    load_cells(cell, L, blockIdx.x, c);
#pragma unroll
    for (int q = kPerLane - 2; q >= 0; --q) c[q] = min(c[q], c[q + 1]);
    uint32_t all;
    const uint32_t right = min(min_right_of<kThreads / 64>(c[0], wave_min, all), carry[blockIdx.x]);
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

// what every entry point refuses before it looks at anything else
int check_cells(const uint32_t *d_cells, int64_t L, uint32_t cap) {
    if (L < 0 || L > kMaxL) return fail(MEMO_EINVAL, "a window of %lld positions: L must be in [0, 2^31]", (long long)L);
    if (cap < 1 || cap > kMaxCap) return fail(MEMO_EINVAL, "cap must be in [1, 2^31 - 1] (got %u)", cap);
    if (reinterpret_cast<uintptr_t>(d_cells) & 15) return fail(MEMO_EINVAL, "d_cells must be 16-byte aligned");
    if (L && !d_cells) return fail(MEMO_EINVAL, "d_cells is NULL");
    return MEMO_OK;
}

// event pairs around the launches of a timed call (memo_debug_maxk_times): lap(i) waits for the launches since the last lap
// and adds their device time to g_maxk_ms[i]
struct Laps {
    hipEvent_t e[2] = {};
    hipStream_t st;
    explicit Laps(hipStream_t s) : st(s) {}
    ~Laps() {
        for (hipEvent_t x : e)
            if (x) (void)hipEventDestroy(x);
    }
    int start() {
        if (!g_maxk_timed) return MEMO_OK;
        for (hipEvent_t &x : e)
            if (!x) HIP_TRY(hipEventCreate(&x));
        HIP_TRY(hipEventRecord(e[0], st));
        return MEMO_OK;
    }
    int lap(int i) {
        if (!g_maxk_timed) return MEMO_OK;
        float ms = 0.f;
        HIP_TRY(hipEventRecord(e[1], st));
        HIP_TRY(hipEventSynchronize(e[1]));
        HIP_TRY(hipEventElapsedTime(&ms, e[0], e[1]));
        g_maxk_ms[i] = ms;
        HIP_TRY(hipEventRecord(e[0], st));
        return MEMO_OK;
    }
};

template <bool VEC>
void launch_rows(const RowArgs &A, unsigned grid, hipStream_t st) {
    if (g_maxk_rows_way) hipLaunchKernelGGL((maxk_rows_kernel<VEC, false>), dim3(grid), dim3(kThreads), 0, st, A);
    else hipLaunchKernelGGL((maxk_rows_kernel<VEC, true>), dim3(grid), dim3(kThreads), 0, st, A);
}

}  // namespace

extern "C" {

int32_t memo_maxk_tile(void) { return kTile; }

int memo_maxk_begin_dev(uint32_t *d_cells, int64_t L, uint32_t cap, int32_t device, void *stream) {
    if (int rc = check_cells(d_cells, L, cap)) return rc;
    if (!L) return MEMO_OK;
    if (int rc = device_ok(device)) return rc;
    DeviceGuard guard(device);
    if (!guard.ok) return fail(MEMO_EHIP, "cannot select HIP device %d", device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    Laps laps(st);
    if (int rc = laps.start()) return rc;
    const int64_t wgs = std::max<int64_t>(1, std::min<int64_t>(((L >> 2) + kThreads - 1) / kThreads, 1 << 16));
    hipLaunchKernelGGL(maxk_fill_kernel, dim3((unsigned)wgs), dim3(kThreads), 0, st, d_cells, L, (uint32_t)(L - 1 + cap));
    HIP_TRY(hipGetLastError());
    if (int rc = laps.lap(0)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return MEMO_OK;
}

int memo_maxk_rows_dev(const int64_t *d_start, const int64_t *d_end, const int64_t *d_annot, uint64_t rows, int64_t qs, int64_t L,
                       uint32_t cap, int32_t mode, int64_t arg, uint32_t *d_cells, int32_t device, void *stream) {
    if (int rc = check_cells(d_cells, L, cap)) return rc;
    if (mode != 0 && mode != 1) return fail(MEMO_EINVAL, "mode must be 0 (0 <= annot < arg) or 1 (annot == arg)");
    if (qs < -kCoordLimit || qs > kCoordLimit) return fail(MEMO_EINVAL, "window start %lld is beyond +-2^61", (long long)qs);
    if ((reinterpret_cast<uintptr_t>(d_start) | reinterpret_cast<uintptr_t>(d_end) | reinterpret_cast<uintptr_t>(d_annot)) & 7)
        return fail(MEMO_EINVAL, "the row columns must be 8-byte aligned");
    if (rows && (!d_start || !d_end || !d_annot)) return fail(MEMO_EINVAL, "a row column is NULL");
    if (!L || !rows) return MEMO_OK;
    if (int rc = device_ok(device)) return rc;
    DeviceGuard guard(device);
    if (!guard.ok) return fail(MEMO_EHIP, "cannot select HIP device %d", device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    RowArgs A = {};
    A.s = d_start, A.e = d_end, A.a = d_annot;
    A.rows = rows;
    const uintptr_t off = reinterpret_cast<uintptr_t>(d_start) & 15;
    const bool vec = (reinterpret_cast<uintptr_t>(d_end) & 15) == off && (reinterpret_cast<uintptr_t>(d_annot) & 15) == off;
    A.head = vec && off ? 1 : 0;
    A.npairs = (int64_t)((rows - (uint64_t)A.head) / 2);
    A.ident = (uint32_t)(L - 1 + cap);
    A.last = (uint32_t)(L - 1);
    A.qs = qs;
    A.s_end = qs + L + (int64_t)cap;
    A.e_hi = qs + (int64_t)A.ident;
    A.mode = mode;
    A.arg = arg;
    A.cell = d_cells;
    const int64_t nchunks = (A.npairs + kPairsPerWg - 1) / kPairsPerWg;
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(nchunks, 1 << 16));
    Laps laps(st);
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
    if (int rc = device_ok(device)) return rc;
    DeviceGuard guard(device);
    if (!guard.ok) return fail(MEMO_EHIP, "cannot select HIP device %d", device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t ntiles = (L + kTile - 1) / kTile;
    DevPtr<uint32_t> mins;
    if (hipError_t err = mins.alloc((size_t)ntiles); err != hipSuccess)
        return fail(MEMO_EHIP, "hipMalloc(%zu bytes) for the tile minima of %lld positions: %s", (size_t)ntiles * sizeof(uint32_t), (long long)L,
                    hipGetErrorString(err));
    Laps laps(st);
    if (int rc = laps.start()) return rc;
    hipLaunchKernelGGL(maxk_tile_min_kernel, dim3((unsigned)ntiles), dim3(kThreads), 0, st, d_cells, L, mins.p);
    HIP_TRY(hipGetLastError());
    if (int rc = laps.lap(2)) return rc;
    hipLaunchKernelGGL(scan_tile_mins, dim3(1), dim3(kScanThreads), 0, st, mins.p, ntiles, (uint32_t)(L - 1 + cap));
    HIP_TRY(hipGetLastError());
    if (int rc = laps.lap(3)) return rc;
    hipLaunchKernelGGL(maxk_apply_kernel, dim3((unsigned)ntiles), dim3(kThreads), 0, st, d_cells, L, mins.p, cap);
    HIP_TRY(hipGetLastError());
    if (int rc = laps.lap(4)) return rc;
    HIP_TRY(hipStreamSynchronize(st));  // (the tile minima go with this call)
    return MEMO_OK;
}

}  // extern "C"
