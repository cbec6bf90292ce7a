// memo_lengths.hip -- `memo lengths`: from a MEMBERSHIP index, for every position of a window, how far every genome matches the pivot,
//     len[g][p - qs] = min( CAP, max( 0, min{ e_i - p : a_i = g, p < s_i, qs < s_i < qe + CAP } ) )        uint32, CAP where no row bounds p
// for all genomes 0 <= g < N in ONE pass over the rows, and the T-th largest of them per position,
//     sel_T[p - qs] = the T-th largest of { len[g][p - qs] : 0 <= g < N }                                     1 <= T <= N
// ("up to which k do at least T genomes hold this k-mer").  len[g] is `memo maxk -m -d g` (memo_maxk.hip); the planes,
// the carry between slices and the selection are new.  No counterpart in the reference.
//
// Cells.  uint32 cell[N][pitch], genome-major, relative to qs; pitch >= L, a multiple of 4; the base 16-byte aligned, so every plane
// is.  The identity is ident = L - 1 + CAP (L <= 2^31 and CAP < 2^31: below 2^32); every value is saturated to [0, ident], which is
// exact: a bound at or above ident yields CAP at every position.  The cells [L, pitch) of a plane are never read or written.
//   1. begin   lengths_fill_kernel: [0, L) of every plane = ident, 16-byte stores (pitch % 4 == 0 keeps the planes aligned); with a
//              carry (int64 [N], INT64_MAX: none) cell[g][L - 1] = clamp(carry[g] - qs)
//   2. rows    lengths_rows_kernel: streams the three int64 columns as maxk_rows_kernel does (16 bytes a lane and load, kLoads loads of
//              each column in flight) and for every row with 0 <= a < N and qs < s < qe + CAP:
//              atomicMin(&cell[a][min(s - 1 - qs, L - 1)], clamp(e - qs)), no return value, device scope; a row whose clamp is ident is
//              the identity and is skipped.  ONE atomic per row: a membership index sorted by start has neighbouring rows in different
//              planes, the wave aggregation of memo_maxk.hip would find nothing to merge.  Min is idempotent and commutative: any
//              order, any cut into calls, repeated rows -- the same cells.
//   3. carry   lengths_carry_kernel: carry[a] = min(carry[a], e) in int64 over the rows with lo < s < hi and 0 <= a < N: per-workgroup
//              minima in LDS (N <= 2048: 16 KiB), then one global 64-bit atomic min per genome the workgroup saw and workgroup.  With
//              it a long window runs in slices from the right, every row read once: before the slice [a, b) the carry holds the rows
//              with b < s < qe + CAP and enters cell L - 1 of every plane (begin); it stays int64, because a carry clamped into one
//              slice's cells would be wrong for rows with e < s that reach across slices.
//   4. finish  the three launches of memo_maxk.hip with the plane in blockIdx.y (the scan: one workgroup per plane, in blockIdx.x):
//              lengths_tile_min_kernel, lengths_scan_kernel (mins[g][t] <- min(mins[g][t + 1 ..]), ident for the last tile),
//              lengths_apply_kernel (reverse inclusive min-scan per tile, then cell > i ? min(cell - i, CAP) : 0 over the cell)
//   5. select  lengths_select_kernel<P>: out[p] = the T-th largest over g of min(cell[g][p], CAP).  A workgroup of 256 lanes takes a tile
//              of P positions (256, 128 ... 8: the largest whose N rows, with the kernel's 16 static bytes, fit 120 KiB of LDS) and
//              stages them as [g][stride] (a whole tile with 16-byte loads, eight in flight per lane; the window's last tile cell by
//              cell).  S = 256 / P
//              NEIGHBOURING lanes share a position and take the genomes part, part + S ...; stride = P for S = 1 and 5 P / 4 else, which
//              puts the 64 addresses of a wave's read on 64 different banks.  The answer is searched bit by bit from the top
//              (c = ans | bit; count the genomes with value >= c, the S partial counts added by wave shuffles; keep the bit if the count
//              is at least T) -- after a first pass that counts the values equal to CAP (at least T of them: the answer is CAP) and
//              finds the tile's largest value under CAP, whose bit width is the number of rounds.
//
// Conditions the code holds:
//   - no workgroup waits for another: no look-back, no flag in memory, no cooperative launch
//   - nothing is read outside the `rows` elements of each column or outside [0, L) of a plane: a 16-byte load is of two rows that both
//     exist or of four cells below L, a tile that crosses L is taken cell by cell
//   - MEMO_EINVAL before any launch: N outside [1, 2048], T outside [1, N], L > 2^31, CAP outside [1, 2^31 - 1], |qs| > 2^61, columns or a
//     carry that are not 8-byte aligned, cells that are not 16-byte aligned, a result that is not 4-byte aligned, pitch < L,
//     pitch % 4 != 0, N pitch >= 2^32; L == 0 or rows == 0 launches nothing
//   - positions, row counts and cell offsets are 64-bit; a cell index inside a plane and a cell value fit 32 bits by the limits above
//   - scratch: the tile minima only (4 bytes per kTile cells and plane), owned by DevPtr; an allocation that fails is MEMO_EHIP with the
//     bytes asked for, and nothing stays allocated
//   - LDS above 64 KiB is opted into with hipFuncSetAttribute before the launch that needs it
//   - values are written with vector stores and vector atomics only; there is no inline assembly
#include <algorithm>

#include "memo_common.h"

using namespace memo;

namespace memo {
thread_local int g_lengths_timed = 0;  // 1 = event pairs around the launches (memo_debug_lengths_times)
thread_local float g_lengths_ms[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // fill, rows, carry, tile minima, scan of them, apply, select
}

namespace {

constexpr int kThreads = 256;
constexpr int kPerLane = 8;                   // cells a lane of the scan holds: two 16-byte loads
constexpr int kTile = kThreads * kPerLane;    // cells per tile of the scan
constexpr int kScanThreads = 1024, kScanPerLane = 4;
constexpr int kScanRound = kScanThreads * kScanPerLane;  // tile minima one round of the scan takes
constexpr int kLoads = 4;                     // 16-byte loads of each column a lane has in flight
constexpr int64_t kPairsPerWg = (int64_t)kThreads * kLoads;  // row pairs a workgroup takes at a time
constexpr uint32_t kNone = 0xFFFFFFFFu;       // above every cell value; as a cell index: no cell
constexpr int64_t kMaxL = (int64_t)1 << 31;
constexpr uint32_t kMaxCap = 0x7FFFFFFFu;
constexpr int kMaxDocs = 2048;
constexpr size_t kSelectLds = 120 << 10;      // of the CU's 160 KiB: the staged values and the kernel's static words together
constexpr size_t kSelectStatic = (kThreads / 64) * sizeof(uint32_t);  // lengths_select_kernel's wave_max
constexpr int kCarryWgs = 1024;               // workgroups of the carry pass at most: each ends with up to N global atomics

struct RowArgs {
    const int64_t *s, *e, *a;
    uint64_t rows;
    int64_t head;    // rows before the first 16-byte pair (0 or 1)
    int64_t npairs;  // 16-byte pairs behind them
    int64_t qs, s_end, e_hi;  // rows: s_end = qs + L + CAP (a start at or past it is ignored), e_hi = qs + ident; carry: qs = lo, s_end = hi
    int64_t n, pitch;
    uint32_t last, ident;  // last = L - 1
    uint32_t *cell;
    int64_t *carry;
};

// the cell (inside its plane) and value of a row; cell kNone: the row is ignored
__device__ __forceinline__ void row_bound(const RowArgs &A, int64_t s, int64_t e, int64_t a, uint32_t &j, uint32_t &v) {
    j = kNone, v = kNone;
    if (a < 0 || a >= A.n || s <= A.qs || s >= A.s_end) return;
    v = e <= A.qs ? 0u : e >= A.e_hi ? A.ident : (uint32_t)(e - A.qs);
    if (v >= A.ident) return;  // the identity
    const uint64_t d = (uint64_t)(s - A.qs - 1);
    j = d < A.last ? (uint32_t)d : A.last;
}

struct CellMin {  // rows: one atomic min per row into its genome's plane
    __device__ __forceinline__ void operator()(const RowArgs &A, int64_t s, int64_t e, int64_t a) const {
        uint32_t j, v;
        row_bound(A, s, e, a, j, v);
        if (j != kNone) (void)__hip_atomic_fetch_min(A.cell + a * A.pitch + j, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

struct CarryMin {  // carry: the workgroup's minima in LDS
    long long *lds;
    __device__ __forceinline__ void operator()(const RowArgs &A, int64_t s, int64_t e, int64_t a) const {
        if (a < 0 || a >= A.n || s <= A.qs || s >= A.s_end) return;
        (void)__hip_atomic_fetch_min(lds + a, (long long)e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
};

// every row of the columns to f, once: the pairs grid-strided in chunks of kPairsPerWg, the rows outside the pairs (the first row of
// columns that start 8 bytes off a 16-byte line, the last odd row) by two lanes of workgroup 0
template <bool VEC, typename F>
__device__ __forceinline__ void stream_rows(const RowArgs &A, const F &f) {
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
            f(A, s[u].x, e[u].x, a[u].x);
            f(A, s[u].y, e[u].y, a[u].y);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < 2) {
        const uint64_t behind = (uint64_t)(A.head + 2 * A.npairs);
        const bool first = threadIdx.x == 0;
        if (first ? A.head == 1 : behind < A.rows) {
            const uint64_t r = first ? 0 : behind;
            f(A, A.s[r], A.e[r], A.a[r]);
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void lengths_rows_kernel(const RowArgs A) {
    stream_rows<VEC>(A, CellMin{});
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void lengths_carry_kernel(const RowArgs A) {
    __shared__ long long lo[kMaxDocs];
    for (int g = threadIdx.x; g < A.n; g += kThreads) lo[g] = INT64_MAX;
    __syncthreads();
    stream_rows<VEC>(A, CarryMin{lo});
    __syncthreads();
    for (int g = threadIdx.x; g < A.n; g += kThreads)
        if (lo[g] != INT64_MAX) (void)__hip_atomic_fetch_min((long long *)A.carry + g, lo[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// grid (.., N): [0, L) of plane blockIdx.y = ident
__global__ __launch_bounds__(kThreads) void lengths_fill_kernel(uint32_t *cells, int64_t L, int64_t pitch, uint32_t ident) {
    uint32_t *cell = cells + (int64_t)blockIdx.y * pitch;
    const int64_t n4 = L >> 2;
    const uint4 v = make_uint4(ident, ident, ident, ident);
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n4; i += (int64_t)gridDim.x * kThreads)
        reinterpret_cast<uint4 *>(cell)[i] = v;
    if (blockIdx.x == 0 && threadIdx.x < (L & 3)) cell[4 * n4 + threadIdx.x] = ident;
}

// cell[g][L - 1] = clamp(carry[g] - qs), after the fill (its own launch: the fill's workgroups are not ordered among themselves)
__global__ __launch_bounds__(kThreads) void lengths_carry_in_kernel(uint32_t *cells, int64_t L, int64_t pitch, int n, uint32_t ident,
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

// grid (ntiles, N): the minimum of tile blockIdx.x of plane blockIdx.y
__global__ __launch_bounds__(kThreads) void lengths_tile_min_kernel(const uint32_t *cells, int64_t L, int64_t pitch, uint32_t *mins) {
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

// grid (N): plane blockIdx.x's mins[t] <- min(mins[t + 1 .. ntiles)), ident for the last tile; rounds of kScanRound tiles from the right
__global__ __launch_bounds__(kScanThreads) void lengths_scan_kernel(uint32_t *all_mins, int64_t ntiles, uint32_t ident) {
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

// grid (ntiles, N)
__global__ __launch_bounds__(kThreads) void lengths_apply_kernel(uint32_t *cells, int64_t L, int64_t pitch, const uint32_t *carry, uint32_t cap) {
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

// ---- select -------------------------------------------------------------------------------------------------------------
// positions per tile: the largest of 256, 128 ... 8 whose N rows of `stride` words fit kSelectLds
constexpr int select_stride(int P) { return P == kThreads ? P : P + P / 4; }
int select_tile(int n) {
    for (int P = kThreads; P > 8; P >>= 1)
        if ((size_t)n * select_stride(P) * sizeof(uint32_t) + kSelectStatic <= kSelectLds) return P;
    return 8;  // (2048 rows of 10 words: 80 KiB)
}

struct SelectArgs {
    const uint32_t *cells;
    uint32_t *out;
    int64_t L, pitch;
    int n, t;
    uint32_t cap;
};

template <int P>
__global__ __launch_bounds__(kThreads) void lengths_select_kernel(const SelectArgs A) {
    extern __shared__ __attribute__((aligned(16))) uint32_t vals[];  // [n][STRIDE]: min(cell, CAP); positions at or past L: 0
    __shared__ uint32_t wave_max[kThreads / 64];
    static_assert(sizeof(wave_max) == kSelectStatic, "the LDS budget counts the static words");
    constexpr int S = kThreads / P, STRIDE = select_stride(P);  // S lanes a position: lane = pos * S + part
    const int64_t p0 = (int64_t)blockIdx.x * P;
    if (p0 + P <= A.L) {
        // stage a whole tile: 16-byte loads (the planes and p0 are 16-byte aligned), kStage of them in flight per lane -- one load
        // a lane at a time left the kernel waiting for memory a hundred times a tile
        constexpr int Q = P / 4, kStage = 8;  // quads per row of the tile
        const int nquads = A.n * Q;
        for (int i0 = threadIdx.x; i0 < nquads; i0 += kThreads * kStage) {
            uint4 v[kStage];
#pragma unroll
            for (int u = 0; u < kStage; ++u) {
                const int i = i0 + u * kThreads;
                if (i < nquads) v[u] = *reinterpret_cast<const uint4 *>(A.cells + (int64_t)(i / Q) * A.pitch + p0 + 4 * (i % Q));
            }
#pragma unroll
            for (int u = 0; u < kStage; ++u) {
                const int i = i0 + u * kThreads;
                if (i < nquads) {
                    uint32_t *d = vals + (i / Q) * STRIDE + 4 * (i % Q);
                    d[0] = min(v[u].x, A.cap), d[1] = min(v[u].y, A.cap), d[2] = min(v[u].z, A.cap), d[3] = min(v[u].w, A.cap);
                }
            }
        }
    } else {
        // the window's last tile, cell by cell: P neighbouring lanes read P neighbouring positions of one genome
        for (int i = threadIdx.x; i < A.n * P; i += kThreads) {
            const int g = i / P, q = i % P;
            const int64_t p = p0 + q;
            vals[g * STRIDE + q] = p < A.L ? min(A.cells[(int64_t)g * A.pitch + p], A.cap) : 0u;
        }
    }
    __syncthreads();
    const int pos = threadIdx.x / S, part = threadIdx.x % S;
    const uint32_t *mine = vals + pos;
    // the values equal to CAP, and the largest value under it
    int at_cap = 0;
    uint32_t top = 0;
#pragma unroll 8
    for (int g = part; g < A.n; g += S) {
        const uint32_t v = mine[g * STRIDE];
        at_cap += v == A.cap;
        top = max(top, v == A.cap ? 0u : v);
    }
#pragma unroll
    for (int d = 1; d < S; d <<= 1) at_cap += __shfl_xor(at_cap, d);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) top = max(top, __shfl_xor(top, d));
    if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x >> 6] = top;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) top = max(top, wave_max[w]);
    // the T-th largest is CAP where at least T values are; else it is at most `top`, and the largest c with #{v >= c} >= T
    uint32_t ans = 0;
    for (int b = 31 - __clz((int)(top | 1u)); b >= 0; --b) {  // (top < CAP < 2^31; uniform over the workgroup)
        const uint32_t c = ans | (1u << b);
        int ge = 0;
#pragma unroll 8
        for (int g = part; g < A.n; g += S) ge += mine[g * STRIDE] >= c;
#pragma unroll
        for (int d = 1; d < S; d <<= 1) ge += __shfl_xor(ge, d);
        if (ge >= A.t) ans = c;
    }
    if (part == 0 && p0 + pos < A.L) A.out[p0 + pos] = at_cap >= A.t ? A.cap : ans;
}

template <int P>
int launch_select(const SelectArgs &A, hipStream_t st) {
    const size_t lds = (size_t)A.n * select_stride(P) * sizeof(uint32_t);
    if (lds > (64 << 10))  // above the default limit: opt in (per kernel and device; the call is cheap beside a launch that stages this much)
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(lengths_select_kernel<P>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(lengths_select_kernel<P>, dim3((unsigned)((A.L + P - 1) / P)), dim3(kThreads), lds, st, A);
    return MEMO_OK;
}

// what every entry point that takes the cells refuses before it looks at anything else
int check_cells(const uint32_t *d_cells, int64_t L, int64_t pitch, int32_t n, uint32_t cap) {
    if (n < 1 || n > kMaxDocs) return fail(MEMO_EINVAL, "num_docs must be in [1, %d] (got %d)", kMaxDocs, n);
    if (L < 0 || L > kMaxL) return fail(MEMO_EINVAL, "a window of %lld positions: L must be in [0, 2^31]", (long long)L);
    if (cap < 1 || cap > kMaxCap) return fail(MEMO_EINVAL, "cap must be in [1, 2^31 - 1] (got %u)", cap);
    if (pitch < L || (pitch & 3)) return fail(MEMO_EINVAL, "pitch %lld: it must be a multiple of 4 and at least L = %lld", (long long)pitch, (long long)L);
    if ((int64_t)n * pitch >= ((int64_t)1 << 32)) return fail(MEMO_EINVAL, "%d planes of pitch %lld: 2^32 cells or more (take the window in slices)", n, (long long)pitch);
    if (reinterpret_cast<uintptr_t>(d_cells) & 15) return fail(MEMO_EINVAL, "d_cells must be 16-byte aligned");
    if (L && !d_cells) return fail(MEMO_EINVAL, "d_cells is NULL");
    return MEMO_OK;
}

int check_columns(const int64_t *d_start, const int64_t *d_end, const int64_t *d_annot, uint64_t rows) {
    if ((reinterpret_cast<uintptr_t>(d_start) | reinterpret_cast<uintptr_t>(d_end) | reinterpret_cast<uintptr_t>(d_annot)) & 7)
        return fail(MEMO_EINVAL, "the row columns must be 8-byte aligned");
    if (rows && (!d_start || !d_end || !d_annot)) return fail(MEMO_EINVAL, "a row column is NULL");
    return MEMO_OK;
}

// the columns of a row pass: 16-byte loads when all three have the same alignment mod 16, else 8-byte loads.  Returns the grid.
unsigned set_columns(RowArgs &A, const int64_t *d_start, const int64_t *d_end, const int64_t *d_annot, uint64_t rows, bool &vec, int64_t most) {
    A.s = d_start, A.e = d_end, A.a = d_annot;
    A.rows = rows;
    const uintptr_t off = reinterpret_cast<uintptr_t>(d_start) & 15;
    vec = (reinterpret_cast<uintptr_t>(d_end) & 15) == off && (reinterpret_cast<uintptr_t>(d_annot) & 15) == off;
    A.head = vec && off ? 1 : 0;
    A.npairs = (int64_t)((rows - (uint64_t)A.head) / 2);
    const int64_t nchunks = (A.npairs + kPairsPerWg - 1) / kPairsPerWg;
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(nchunks, most));
}

// event pairs around the launches of a timed call (memo_debug_lengths_times): lap(i) waits for the launches since the last lap
// and puts their device time into g_lengths_ms[i]
struct Laps {
    hipEvent_t e[2] = {};
    hipStream_t st;
    explicit Laps(hipStream_t s) : st(s) {}
    ~Laps() {
        for (hipEvent_t x : e)
            if (x) (void)hipEventDestroy(x);
    }
    int start() {
        if (!g_lengths_timed) return MEMO_OK;
        for (hipEvent_t &x : e)
            if (!x) HIP_TRY(hipEventCreate(&x));
        HIP_TRY(hipEventRecord(e[0], st));
        return MEMO_OK;
    }
    int lap(int i) {
        if (!g_lengths_timed) return MEMO_OK;
        float ms = 0.f;
        HIP_TRY(hipEventRecord(e[1], st));
        HIP_TRY(hipEventSynchronize(e[1]));
        HIP_TRY(hipEventElapsedTime(&ms, e[0], e[1]));
        g_lengths_ms[i] = ms;
        HIP_TRY(hipEventRecord(e[0], st));
        return MEMO_OK;
    }
};

}  // namespace

extern "C" {

int32_t memo_lengths_tile(void) { return kTile; }

int32_t memo_lengths_select_tile(int32_t num_docs) { return num_docs < 1 || num_docs > kMaxDocs ? 0 : select_tile(num_docs); }

int memo_lengths_begin_dev(uint32_t *d_cells, int64_t L, int64_t pitch, int32_t num_docs, uint32_t cap, int64_t qs, const int64_t *d_carry,
                           int32_t device, void *stream) {
    if (int rc = check_cells(d_cells, L, pitch, num_docs, cap)) return rc;
    if (qs < -kCoordLimit || qs > kCoordLimit) return fail(MEMO_EINVAL, "window start %lld is beyond +-2^61", (long long)qs);
    if (reinterpret_cast<uintptr_t>(d_carry) & 7) return fail(MEMO_EINVAL, "d_carry must be 8-byte aligned");
    if (!L) return MEMO_OK;
    if (int rc = device_ok(device)) return rc;
    DeviceGuard guard(device);
    if (!guard.ok) return fail(MEMO_EHIP, "cannot select HIP device %d", device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    Laps laps(st);
    if (int rc = laps.start()) return rc;
    const uint32_t ident = (uint32_t)(L - 1 + cap);
    const int64_t wgs = std::max<int64_t>(1, std::min<int64_t>(((L >> 2) + kThreads - 1) / kThreads, 1 << 12));
    hipLaunchKernelGGL(lengths_fill_kernel, dim3((unsigned)wgs, (unsigned)num_docs), dim3(kThreads), 0, st, d_cells, L, pitch, ident);
    HIP_TRY(hipGetLastError());
    if (d_carry) {
        hipLaunchKernelGGL(lengths_carry_in_kernel, dim3((unsigned)((num_docs + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, d_cells, L, pitch,
                           (int)num_docs, ident, d_carry, qs);
        HIP_TRY(hipGetLastError());
    }
    if (int rc = laps.lap(0)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return MEMO_OK;
}

int memo_lengths_rows_dev(const int64_t *d_start, const int64_t *d_end, const int64_t *d_annot, uint64_t rows, int64_t qs, int64_t L,
                          int64_t pitch, int32_t num_docs, uint32_t cap, uint32_t *d_cells, int32_t device, void *stream) {
    if (int rc = check_cells(d_cells, L, pitch, num_docs, cap)) return rc;
    if (qs < -kCoordLimit || qs > kCoordLimit) return fail(MEMO_EINVAL, "window start %lld is beyond +-2^61", (long long)qs);
    if (int rc = check_columns(d_start, d_end, d_annot, rows)) return rc;
    if (!L || !rows) return MEMO_OK;
    if (int rc = device_ok(device)) return rc;
    DeviceGuard guard(device);
    if (!guard.ok) return fail(MEMO_EHIP, "cannot select HIP device %d", device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    RowArgs A = {};
    bool vec;
    const unsigned grid = set_columns(A, d_start, d_end, d_annot, rows, vec, 1 << 16);
    A.ident = (uint32_t)(L - 1 + cap);
    A.last = (uint32_t)(L - 1);
    A.qs = qs;
    A.s_end = qs + L + (int64_t)cap;
    A.e_hi = qs + (int64_t)A.ident;
    A.n = num_docs;
    A.pitch = pitch;
    A.cell = d_cells;
    Laps laps(st);
    if (int rc = laps.start()) return rc;
    if (vec) hipLaunchKernelGGL(lengths_rows_kernel<true>, dim3(grid), dim3(kThreads), 0, st, A);
    else hipLaunchKernelGGL(lengths_rows_kernel<false>, dim3(grid), dim3(kThreads), 0, st, A);
    HIP_TRY(hipGetLastError());
    if (int rc = laps.lap(1)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return MEMO_OK;
}

int memo_lengths_carry_dev(const int64_t *d_start, const int64_t *d_end, const int64_t *d_annot, uint64_t rows, int64_t lo, int64_t hi,
                           int32_t num_docs, int64_t *d_carry, int32_t device, void *stream) {
    if (num_docs < 1 || num_docs > kMaxDocs) return fail(MEMO_EINVAL, "num_docs must be in [1, %d] (got %d)", kMaxDocs, num_docs);
    if (int rc = check_columns(d_start, d_end, d_annot, rows)) return rc;
    if (!d_carry || (reinterpret_cast<uintptr_t>(d_carry) & 7)) return fail(MEMO_EINVAL, "d_carry must be 8-byte aligned and not NULL");
    if (!rows || hi <= lo) return MEMO_OK;
    if (int rc = device_ok(device)) return rc;
    DeviceGuard guard(device);
    if (!guard.ok) return fail(MEMO_EHIP, "cannot select HIP device %d", device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    RowArgs A = {};
    bool vec;
    const unsigned grid = set_columns(A, d_start, d_end, d_annot, rows, vec, kCarryWgs);
    A.qs = lo;
    A.s_end = hi;
    A.n = num_docs;
    A.carry = d_carry;
    Laps laps(st);
    if (int rc = laps.start()) return rc;
    if (vec) hipLaunchKernelGGL(lengths_carry_kernel<true>, dim3(grid), dim3(kThreads), 0, st, A);
    else hipLaunchKernelGGL(lengths_carry_kernel<false>, dim3(grid), dim3(kThreads), 0, st, A);
    HIP_TRY(hipGetLastError());
    if (int rc = laps.lap(2)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return MEMO_OK;
}

int memo_lengths_finish_dev(uint32_t *d_cells, int64_t L, int64_t pitch, int32_t num_docs, uint32_t cap, int32_t device, void *stream) {
    if (int rc = check_cells(d_cells, L, pitch, num_docs, cap)) return rc;
    if (!L) return MEMO_OK;
    if (int rc = device_ok(device)) return rc;
    DeviceGuard guard(device);
    if (!guard.ok) return fail(MEMO_EHIP, "cannot select HIP device %d", device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t ntiles = (L + kTile - 1) / kTile;  // (at most 2^20: fits grid.x; num_docs <= 2048 fits grid.y)
    DevPtr<uint32_t> mins;
    if (hipError_t err = mins.alloc((size_t)ntiles * num_docs); err != hipSuccess)
        return fail(MEMO_EHIP, "hipMalloc(%zu bytes) for the tile minima of %d planes of %lld positions: %s", (size_t)ntiles * num_docs * sizeof(uint32_t),
                    num_docs, (long long)L, hipGetErrorString(err));
    const dim3 tiles((unsigned)ntiles, (unsigned)num_docs);
    Laps laps(st);
    if (int rc = laps.start()) return rc;
    hipLaunchKernelGGL(lengths_tile_min_kernel, tiles, dim3(kThreads), 0, st, d_cells, L, pitch, mins.p);
    HIP_TRY(hipGetLastError());
    if (int rc = laps.lap(3)) return rc;
    hipLaunchKernelGGL(lengths_scan_kernel, dim3((unsigned)num_docs), dim3(kScanThreads), 0, st, mins.p, ntiles, (uint32_t)(L - 1 + cap));
    HIP_TRY(hipGetLastError());
    if (int rc = laps.lap(4)) return rc;
    hipLaunchKernelGGL(lengths_apply_kernel, tiles, dim3(kThreads), 0, st, d_cells, L, pitch, mins.p, cap);
    HIP_TRY(hipGetLastError());
    if (int rc = laps.lap(5)) return rc;
    HIP_TRY(hipStreamSynchronize(st));  // (the tile minima go with this call)
    return MEMO_OK;
}

int memo_lengths_select_dev(const uint32_t *d_cells, int64_t L, int64_t pitch, int32_t num_docs, uint32_t cap, int32_t threshold,
                            uint32_t *d_out, int32_t device, void *stream) {
    if (int rc = check_cells(d_cells, L, pitch, num_docs, cap)) return rc;
    if (threshold < 1 || threshold > num_docs) return fail(MEMO_EINVAL, "threshold must be in [1, %d] (got %d)", num_docs, threshold);
    if (reinterpret_cast<uintptr_t>(d_out) & 3) return fail(MEMO_EINVAL, "d_out must be 4-byte aligned");
    if (L && !d_out) return fail(MEMO_EINVAL, "d_out is NULL");
    if (!L) return MEMO_OK;
    if (int rc = device_ok(device)) return rc;
    DeviceGuard guard(device);
    if (!guard.ok) return fail(MEMO_EHIP, "cannot select HIP device %d", device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    SelectArgs A = {d_cells, d_out, L, pitch, num_docs, threshold, cap};
    Laps laps(st);
    if (int rc = laps.start()) return rc;
    int rc = MEMO_OK;
    switch (select_tile(num_docs)) {
        case 256: rc = launch_select<256>(A, st); break;
        case 128: rc = launch_select<128>(A, st); break;
        case 64: rc = launch_select<64>(A, st); break;
        case 32: rc = launch_select<32>(A, st); break;
        case 16: rc = launch_select<16>(A, st); break;
        default: rc = launch_select<8>(A, st); break;
    }
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    if (int rc2 = laps.lap(6)) return rc2;
    HIP_TRY(hipStreamSynchronize(st));
    return MEMO_OK;
}

}  // extern "C"
