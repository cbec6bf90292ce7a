// memo_lengths.hip -- `memo lengths`: from a MEMBERSHIP index, for every position of a window, how far every genome matches the pivot,
//     len[g][p - qs] = min( CAP, max( 0, min{ e_i - p : a_i = g, p < s_i, qs < s_i < qe + CAP } ) )        uint32, CAP where no row bounds p
// for all genomes 0 <= g < N in ONE pass over the rows, and the T-th largest of them per position,
//     sel_T[p - qs] = the T-th largest of { len[g][p - qs] : 0 <= g < N }                                     1 <= T <= N
// ("up to which k do at least T genomes hold this k-mer").  len[g] is `memo maxk -m -d g` (memo_maxk.hip); the planes,
// the carry between slices and the selection are new.  No counterpart in the reference.
//
// Cells.  uint32 cell[N][pitch], genome-major, relative to qs (memo_cells.h's layout, with its identity ident = L - 1 + CAP); pitch >= L,
// a multiple of 4; the base 16-byte aligned, so every plane is.  The cells [L, pitch) of a plane are never read or written.
//   1. begin   memo::cells_fill (memo_cells.hip): [0, L) of every plane = ident, 16-byte stores (pitch % 4 == 0 keeps the planes
//              aligned); with a carry (int64 [N], INT64_MAX: none) memo::cells_carry_in: cell[g][L - 1] = clamp(carry[g] - qs)
//   2. rows    lengths_rows_kernel: memo_cells.h's stream_rows over the three int64 columns (16 bytes a lane and load, kLoads loads of
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
//   4. finish  memo::cells_finish (memo_cells.hip) on the N planes: the tile minima, their suffix-min scan (one workgroup per plane),
//              and the apply launch (reverse inclusive min-scan per tile, then cell > i ? min(cell - i, CAP) : 0 over the cell)
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
#include "memo_cells.h"

using namespace memo;

namespace memo {
thread_local int g_lengths_timed = 0;  // 1 = event pairs around the launches (memo_debug_lengths_times)
thread_local float g_lengths_ms[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // fill, rows, carry, tile minima, scan of them, apply, select
}

namespace {

constexpr int kThreads = kRowThreads;
constexpr int kMaxDocs = 2048;
constexpr size_t kSelectLds = 120 << 10;      // of the CU's 160 KiB: the staged values and the kernel's static words together
constexpr size_t kSelectStatic = (kThreads / 64) * sizeof(uint32_t);  // lengths_select_kernel's wave_max
constexpr int kCarryWgs = 1024;               // workgroups of the carry pass at most: each ends with up to N global atomics

struct RowArgs {
    Columns c;
    RowWindow w;  // carry: qs = lo, s_end = hi
    int64_t n, pitch;
    uint32_t *cell;
    int64_t *carry;
};

struct CellMin {  // rows: one atomic min per row into its genome's plane
    const RowArgs &A;
    __device__ __forceinline__ void one(int64_t s, int64_t e, int64_t a) const {
        uint32_t j, v;
        row_bound(A.w, a >= 0 && a < A.n, s, e, j, v);
        if (j != kNone) (void)__hip_atomic_fetch_min(A.cell + a * A.pitch + j, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __device__ __forceinline__ void pair(const longlong2 &s, const longlong2 &e, const longlong2 &a) const { one(s.x, e.x, a.x), one(s.y, e.y, a.y); }
};

struct CarryMin {  // carry: the workgroup's minima in LDS
    const RowArgs &A;
    long long *lds;
    __device__ __forceinline__ void one(int64_t s, int64_t e, int64_t a) const {
        if (a < 0 || a >= A.n || s <= A.w.qs || s >= A.w.s_end) return;
        (void)__hip_atomic_fetch_min(lds + a, (long long)e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __device__ __forceinline__ void pair(const longlong2 &s, const longlong2 &e, const longlong2 &a) const { one(s.x, e.x, a.x), one(s.y, e.y, a.y); }
};

template <bool VEC>
__global__ __launch_bounds__(kThreads) void lengths_rows_kernel(const RowArgs A) {
    stream_rows<VEC>(A.c, CellMin{A});
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void lengths_carry_kernel(const RowArgs A) {
    __shared__ long long lo[kMaxDocs];
    for (int g = threadIdx.x; g < A.n; g += kThreads) lo[g] = INT64_MAX;
    __syncthreads();
    stream_rows<VEC>(A.c, CarryMin{A, lo});
    __syncthreads();
    for (int g = threadIdx.x; g < A.n; g += kThreads)
        if (lo[g] != INT64_MAX) (void)__hip_atomic_fetch_min((long long *)A.carry + g, lo[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
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
    if (int rc = check_window(L, cap)) return rc;
    if (pitch < L || (pitch & 3)) return fail(MEMO_EINVAL, "pitch %lld: it must be a multiple of 4 and at least L = %lld", (long long)pitch, (long long)L);
    if ((int64_t)n * pitch >= ((int64_t)1 << 32)) return fail(MEMO_EINVAL, "%d planes of pitch %lld: 2^32 cells or more (take the window in slices)", n, (long long)pitch);
    return check_cell_pointer(d_cells, L);
}

}  // namespace

extern "C" {

int32_t memo_lengths_tile(void) { return kCellTile; }

int32_t memo_lengths_select_tile(int32_t num_docs) { return num_docs < 1 || num_docs > kMaxDocs ? 0 : select_tile(num_docs); }

int memo_lengths_begin_dev(uint32_t *d_cells, int64_t L, int64_t pitch, int32_t num_docs, uint32_t cap, int64_t qs, const int64_t *d_carry,
                           int32_t device, void *stream) {
    if (int rc = check_cells(d_cells, L, pitch, num_docs, cap)) return rc;
    if (qs < -kCoordLimit || qs > kCoordLimit) return fail(MEMO_EINVAL, "window start %lld is beyond +-2^61", (long long)qs);
    if (reinterpret_cast<uintptr_t>(d_carry) & 7) return fail(MEMO_EINVAL, "d_carry must be 8-byte aligned");
    if (!L) return MEMO_OK;
    OnDevice on(device);
    if (on.rc) return on.rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    Laps laps(st, g_lengths_timed, g_lengths_ms);
    if (int rc = laps.start()) return rc;
    const CellPlanes P = {d_cells, L, pitch, num_docs, cap};
    HIP_TRY(cells_fill(P, 1 << 12, st));
    if (d_carry) HIP_TRY(cells_carry_in(P, d_carry, qs, st));
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
    OnDevice on(device);
    if (on.rc) return on.rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    RowArgs A = {};
    bool vec;
    const unsigned grid = set_columns(A.c, d_start, d_end, d_annot, rows, vec, 1 << 16);
    A.w.set(qs, L, cap);
    A.n = num_docs;
    A.pitch = pitch;
    A.cell = d_cells;
    Laps laps(st, g_lengths_timed, g_lengths_ms);
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
    OnDevice on(device);
    if (on.rc) return on.rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    RowArgs A = {};
    bool vec;
    const unsigned grid = set_columns(A.c, d_start, d_end, d_annot, rows, vec, kCarryWgs);
    A.w.qs = lo;
    A.w.s_end = hi;
    A.n = num_docs;
    A.carry = d_carry;
    Laps laps(st, g_lengths_timed, g_lengths_ms);
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
    OnDevice on(device);
    if (on.rc) return on.rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t ntiles = cell_tiles(L);
    DevPtr<uint32_t> mins;
    if (hipError_t err = mins.alloc((size_t)ntiles * num_docs); err != hipSuccess)
        return fail(MEMO_EHIP, "hipMalloc(%zu bytes) for the tile minima of %d planes of %lld positions: %s", (size_t)ntiles * num_docs * sizeof(uint32_t),
                    num_docs, (long long)L, hipGetErrorString(err));
    Laps laps(st, g_lengths_timed, g_lengths_ms);
    if (int rc = cells_finish(CellPlanes{d_cells, L, pitch, num_docs, cap}, mins, st, laps, 3)) return rc;
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
    OnDevice on(device);
    if (on.rc) return on.rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    SelectArgs A = {d_cells, d_out, L, pitch, num_docs, threshold, cap};
    Laps laps(st, g_lengths_timed, g_lengths_ms);
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
