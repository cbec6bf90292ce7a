// memo_spectrum.hip -- `memo spectrum`: the conservation histogram of a window at EVERY k-mer size from 1 to KMAX, from the finished
// planes of the memo_lengths_*_dev calls (uint32 cell[N][pitch], genome-major; a cell above KMAX is taken as KMAX), one pass:
//     sel_T[p]    = the T-th largest of cell[0 .. N)[p]                  mode 1: a membership index  (`memo lengths -t T`)
//     sel_T[p]    = min{ cell[a][p] : 0 <= a < T }                       mode 0: a conservation index (`memo maxk -t T`)
//     cons(p, k)  = max({ T : sel_T[p] >= k } + {0})                     1 <= k <= KMAX, in [0, N]
//     exact[k][v] = #{ p : cons(p, k) = v }                              uint64 [KMAX][N + 1]
// (DESIGN.md 10.11).  No counterpart in the reference.
//
// cons(p, .) is a non-increasing step function of k.  The kernels never touch exact[][]: they add every position's steps into a
// DIFFERENCE table D, uint64 [KMAX + 1][N + 1] in the caller's scratch (row k - 1 is k; the counters wrap): a maximal run lo <= k <= hi
// of cons(p, k) = v is D[lo][v] += 1, D[hi + 1][v] -= 1 -- two updates per step and position, whatever N is -- and the finish kernel
// takes the prefix sums over k.
//   begin   the table = 0
//   add     spectrum_kernel<MODE, PRIVATE>, workgroups of 256 lanes, tiles of P positions grid-strided:
//           mode 0  P = 256, one lane per position: a running minimum down the planes (a wave reads 256 contiguous bytes of a plane,
//                   eight planes in flight); where the minimum falls from m to m' at plane g the run m' < k <= m of value g closes; what
//                   is left after the last plane, 1 <= k <= m, has value N
//           mode 1  the multiset of a column, as a counting array per position in LDS: KMAX + 1 counters of 16 bits, two to a word (N <=
//                   2048 cannot overflow one, nor carry into its neighbour), rows of an odd number of words so that the lanes of a wave
//                   fall on different banks; P = the largest of 256, 128, 64, 32 whose rows fit kHistBytes.  N increments per position
//                   (one 32-bit LDS atomic each; a whole tile is read with 16-byte loads, four positions of a plane per lane, eight
//                   loads in flight, the window's last tile cell by cell),
//                   then 256 / P lanes per position walk the counters from KMAX down, each its own stretch of words: cons(p, k) is the
//                   number of values >= k, so a lane needs the sum of the stretches above its own (LDS, one barrier) and closes a run
//                   wherever a counter is not 0
//           PRIVATE the updates go to a workgroup-private copy of the table in LDS, 32-bit counters that wrap (a workgroup sees fewer
//                   than 2^31 positions), one LDS atomic each; when the workgroup has done its tiles every cell that is not 0 is added
//                   to D, sign-extended, with ONE 64-bit atomic add, no return value, device scope, neighbouring lanes on neighbouring
//                   cells.  Taken where (N + 1)(KMAX + 1) words fit beside the staging: staging + table <= kLdsBytes.
//           else    equal (k, v) updates of a wave are merged first: the lanes with the first unserved lane's cell are counted by a
//                   ballot and that lane adds the count with one global atomic; in a conserved stretch a wave's 64 positions are two
//                   atomics.
//   finish  spectrum_finish_kernel: exact[k][v] = sum of D[1 .. k][v]; 32 neighbouring v by 8 stretches of k per workgroup, the
//           stretches' sums through LDS
//
// Conditions the code holds:
//   - no workgroup waits for another: no look-back, no flag in memory, no cooperative launch
//   - nothing is read outside [0, L) of a plane: a lane whose position is at or past L loads nothing and adds nothing; nothing is written
//     outside the (KMAX + 1)(N + 1) counters of the table or the KMAX (N + 1) of the result: every value is clamped to KMAX first, so
//     k + 1 <= KMAX + 1, and a value v is a count of at most N planes
//   - MEMO_EINVAL before any launch: N outside [1, 2048], KMAX outside [1, 1024], a mode other than 0 or 1, L > 2^31, pitch < L,
//     pitch % 4 != 0, N pitch >= 2^32, cells that are not 16-byte aligned, a scratch or a result that is NULL or not 8-byte aligned;
//     L == 0 launches nothing
//   - positions and cell offsets are 64-bit; a cell index inside the table fits 32 bits by the limits above
//   - LDS above 64 KiB is opted into with hipFuncSetAttribute before the launch that needs it
//   - values are written with vector stores and vector atomics only; there is no inline assembly
#include <algorithm>

#include "memo_common.h"

using namespace memo;

namespace memo {
thread_local int g_spectrum_timed = 0;  // 1 = event pairs around the launches, 2 = and the global atomics counted (memo_debug_spectrum_times)
thread_local float g_spectrum_ms[2] = {0.f, 0.f};  // add, finish
thread_local int g_spectrum_private = -1;          // the last add: 1 = the private table in LDS, 0 = wave-merged global atomics
thread_local uint64_t g_spectrum_atomics = 0;      // the last add's global atomics, when they were counted
}

namespace {

constexpr int kThreads = 256;
constexpr int kLoads = 8;                      // cells a lane has in flight
constexpr int kMaxDocs = 2048, kMaxK = 1024;
constexpr int64_t kMaxL = (int64_t)1 << 31;
constexpr size_t kHistBytes = 72 << 10;        // mode 1: the counting arrays of a tile at most
constexpr size_t kLdsBytes = 128 << 10;        // of the CU's 160 KiB: staging and private table together
constexpr int kMaxGrid = 2048;                 // workgroups of an add at most: each ends with a flush of its table
constexpr int kFinishV = 32, kFinishParts = 8; // finish: values by stretches of k per workgroup

constexpr int hist_words(int kmax) { return ((kmax >> 1) + 1) | 1; }  // per position: values 0 .. kmax, two to a word, an odd stride

// positions per tile
int tile_of(int kmax, int mode) {
    if (mode == 0) return kThreads;
    for (int P = kThreads; P > 32; P >>= 1)
        if ((size_t)P * hist_words(kmax) * sizeof(uint32_t) <= kHistBytes) return P;
    return 32;  // (kmax = 1024: 32 rows of 513 words, 65 664 bytes)
}

// LDS words of the staging: the counting arrays and one partial sum per lane
size_t staging_words(int kmax, int mode) { return mode == 0 ? 0 : (size_t)tile_of(kmax, mode) * hist_words(kmax) + kThreads; }
size_t table_cells(int n, int kmax) { return (size_t)(n + 1) * (kmax + 1); }
bool table_fits(int n, int kmax, int mode) { return (staging_words(kmax, mode) + table_cells(n, kmax)) * sizeof(uint32_t) <= kLdsBytes; }

struct Args {
    const uint32_t *cells;
    unsigned long long *D;        // [kmax + 1][n + 1]
    unsigned long long *counted;  // the global atomics issued (NULL: not counted)
    int64_t L, pitch, ntiles;
    int n, kmax;
    int logp;    // mode 1: P = 1 << logp
    int words;   // mode 1: hist_words(kmax)
};

// one update (k, v) += delta, delta = +1 or -1, of the lanes with `on`; every lane of the wave calls it
template <bool PRIVATE>
__device__ __forceinline__ void update(const Args &A, uint32_t *tab, bool on, int k, int v, int delta) {
    const uint32_t cell = (uint32_t)(k - 1) * (uint32_t)(A.n + 1) + (uint32_t)v;
    if (PRIVATE) {
        if (on) (void)__hip_atomic_fetch_add(tab + cell, (uint32_t)delta, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        return;
    }
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(on);
    while (todo) {
        const int first = __ffsll(todo) - 1;
        const uint32_t its = __shfl(cell, first);
        const bool mine = on && cell == its;
        const unsigned long long same = __ballot(mine);
        if (lane == first) {
            (void)__hip_atomic_fetch_add(A.D + its, (unsigned long long)((long long)delta * __popcll(same)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (A.counted) (void)__hip_atomic_fetch_add(A.counted, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        on = on && !mine;
        todo &= ~same;
    }
}

// mode 0, one tile of 256 positions: the running minimum down the planes
template <bool PRIVATE>
__device__ __forceinline__ void tile_conservation(const Args &A, uint32_t *tab, int64_t tile) {
    const int64_t p = tile * kThreads + threadIdx.x;
    const bool live = p < A.L;
    const uint32_t *mine = A.cells + p;
    const uint32_t kmax = (uint32_t)A.kmax;
    uint32_t m = kmax;  // sel_T so far; no plane yet: every k <= KMAX
    for (int g0 = 0; g0 < A.n; g0 += kLoads) {
        uint32_t c[kLoads];
#pragma unroll
        for (int u = 0; u < kLoads; ++u) c[u] = live && g0 + u < A.n ? mine[(int64_t)(g0 + u) * A.pitch] : kmax;
#pragma unroll
        for (int u = 0; u < kLoads; ++u) {
            if (g0 + u >= A.n) break;  // (uniform)
            const uint32_t lower = min(m, c[u]);
            const bool fell = live && lower < m;  // the run lower < k <= m has value g0 + u
            update<PRIVATE>(A, tab, fell, (int)lower + 1, g0 + u, +1);
            update<PRIVATE>(A, tab, fell, (int)m + 1, g0 + u, -1);
            m = lower;
        }
    }
    const bool left = live && m >= 1;  // 1 <= k <= m: held through every plane
    update<PRIVATE>(A, tab, left, 1, A.n, +1);
    update<PRIVATE>(A, tab, left, (int)m + 1, A.n, -1);
}

// mode 1, one tile of P positions: count, then walk.  hist: [P][words], part: [kThreads]
template <bool PRIVATE>
__device__ __forceinline__ void tile_membership(const Args &A, uint32_t *hist, uint32_t *part, uint32_t *tab, int64_t tile) {
    const int P = 1 << A.logp, S = kThreads >> A.logp;
    const int64_t p0 = tile << A.logp;
    const uint32_t kmax = (uint32_t)A.kmax;
    for (int i = threadIdx.x; i < P * A.words; i += kThreads) hist[i] = 0;
    __syncthreads();
    const int total = A.n << A.logp;
    if (p0 + P <= A.L) {
        // count, a whole tile: 16-byte loads (the planes and p0 are 16-byte aligned), lane i of a round takes four positions of plane
        // i / (P / 4).  A lane's four positions are taken in an order turned by lane / 8: rows are an odd number of words apart, so the
        // 32 lanes of a half wave then fall on 32 different banks when a stretch holds one value
        const int logq = A.logp - 2, nquads = A.n << logq, rot = (threadIdx.x >> 3) & 3;
        for (int i0 = threadIdx.x; i0 < nquads; i0 += kThreads * kLoads) {
            uint4 c[kLoads];
#pragma unroll
            for (int u = 0; u < kLoads; ++u) {
                const int i = i0 + u * kThreads;
                if (i < nquads) c[u] = *reinterpret_cast<const uint4 *>(A.cells + (int64_t)(i >> logq) * A.pitch + p0 + 4 * (i & ((1 << logq) - 1)));
            }
#pragma unroll
            for (int u = 0; u < kLoads; ++u) {
                const int i = i0 + u * kThreads;
                if (i < nquads) {
                    const int q = 4 * (i & ((1 << logq) - 1));
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int jj = (j + rot) & 3;
                        const uint32_t v = min(jj == 0 ? c[u].x : jj == 1 ? c[u].y : jj == 2 ? c[u].z : c[u].w, kmax);
                        (void)__hip_atomic_fetch_add(hist + (q + jj) * A.words + (v >> 1), 1u << ((v & 1) << 4), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                }
            }
        }
    } else
    // count, the window's last tile, cell by cell: lane i of a round takes position i % P of plane i / P
    for (int i0 = threadIdx.x; i0 < total; i0 += kThreads * kLoads) {
        uint32_t c[kLoads];
#pragma unroll
        for (int u = 0; u < kLoads; ++u) {
            const int i = i0 + u * kThreads, q = i & (P - 1);
            c[u] = i < total && p0 + q < A.L ? A.cells[(int64_t)(i >> A.logp) * A.pitch + p0 + q] : 0u;
        }
#pragma unroll
        for (int u = 0; u < kLoads; ++u) {
            const int i = i0 + u * kThreads, q = i & (P - 1);
            if (i < total && p0 + q < A.L) {
                const uint32_t v = min(c[u], kmax);
                (void)__hip_atomic_fetch_add(hist + q * A.words + (v >> 1), 1u << ((v & 1) << 4), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
    }
    __syncthreads();
    // walk: lane (q, s) takes the words [lo, hi) of position q, stretch 0 the highest values
    const int q = threadIdx.x & (P - 1), s = threadIdx.x >> A.logp;
    const bool live = p0 + q < A.L;
    const int W = (A.kmax >> 1) + 1;  // the words that hold a value
    const int each = (W + S - 1) / S;
    const int hi = W - s * each, lo = max(hi - each, 0);
    const uint32_t *row = hist + q * A.words;
    uint32_t sum = 0;
    for (int w = lo; w < hi; ++w) sum += (row[w] & 0xFFFFu) + (row[w] >> 16);
    part[threadIdx.x] = sum;
    __syncthreads();
    uint32_t above = 0;  // the values above this lane's stretch: cons(p, k) for the k just above it
    for (int t = 0; t < s; ++t) above += part[(t << A.logp) + q];
    for (int j = 0; j < each; ++j) {  // (the same count in every lane: update() is called by whole waves)
        const int w = hi - 1 - j;
        const bool has = live && w >= lo;
        const uint32_t x = has ? row[w] : 0u;
#pragma unroll
        for (int half = 1; half >= 0; --half) {
            const int k = 2 * w + half;
            const uint32_t h = half ? x >> 16 : x & 0xFFFFu;
            const bool ok = has && k >= 1 && k <= A.kmax;
            const bool top = ok && k == A.kmax;          // the run that ends at KMAX
            const bool step = ok && k < A.kmax && h > 0;  // cons changes between k + 1 and k
            update<PRIVATE>(A, tab, step, k + 1, (int)above, +1);
            update<PRIVATE>(A, tab, step || top, k + 1, (int)(above + h), -1);
            if (ok) above += h;
            update<PRIVATE>(A, tab, ok && k == 1, 1, (int)above, +1);
        }
    }
    __syncthreads();  // (the next tile clears hist)
}

template <int MODE, bool PRIVATE>
__global__ __launch_bounds__(kThreads) void spectrum_kernel(const Args A) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];  // mode 1: hist, part; PRIVATE: the table behind them
    uint32_t *hist = lds, *part = lds, *tab = lds;
    if (MODE == 1) {
        part = hist + ((size_t)A.words << A.logp);
        tab = part + kThreads;
    }
    const int cells = (A.n + 1) * (A.kmax + 1);
    if (PRIVATE) {
        for (int i = threadIdx.x; i < cells; i += kThreads) tab[i] = 0;
        __syncthreads();
    }
    for (int64_t tile = blockIdx.x; tile < A.ntiles; tile += gridDim.x) {
        if (MODE == 0) tile_conservation<PRIVATE>(A, tab, tile);
        else tile_membership<PRIVATE>(A, hist, part, tab, tile);
    }
    if (PRIVATE) {
        __syncthreads();
        for (int i = threadIdx.x; i < cells; i += kThreads) {
            const uint32_t x = tab[i];
            if (x) {
                (void)__hip_atomic_fetch_add(A.D + i, (unsigned long long)(long long)(int32_t)x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (A.counted) (void)__hip_atomic_fetch_add(A.counted, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

// grid (ceil((n + 1) / kFinishV)): exact[k - 1][v] = D[0][v] + ... + D[k - 1][v]
__global__ __launch_bounds__(kFinishV *kFinishParts) void spectrum_finish_kernel(const unsigned long long *D, unsigned long long *exact, int n, int kmax) {
    __shared__ unsigned long long sums[kFinishParts][kFinishV];
    const int vv = threadIdx.x % kFinishV, s = threadIdx.x / kFinishV;
    const int v = blockIdx.x * kFinishV + vv, stride = n + 1;
    const int each = (kmax + kFinishParts - 1) / kFinishParts;
    const int lo = min(s * each, kmax), hi = min(lo + each, kmax);
    unsigned long long sum = 0;
    if (v <= n)
        for (int j = lo; j < hi; ++j) sum += D[(size_t)j * stride + v];
    sums[s][vv] = sum;
    __syncthreads();
    if (v > n) return;
    unsigned long long run = 0;
    for (int t = 0; t < s; ++t) run += sums[t][vv];
    for (int j = lo; j < hi; ++j) {
        run += D[(size_t)j * stride + v];
        exact[(size_t)j * stride + v] = run;
    }
}

int check_shape(int32_t n, int32_t kmax) {
    if (n < 1 || n > kMaxDocs) return fail(MEMO_EINVAL, "num_docs must be in [1, %d] (got %d)", kMaxDocs, n);
    if (kmax < 1 || kmax > kMaxK) return fail(MEMO_EINVAL, "kmax must be in [1, %d] (got %d)", kMaxK, kmax);
    return MEMO_OK;
}

int check_scratch(const void *d_scratch) {
    if (!d_scratch || (reinterpret_cast<uintptr_t>(d_scratch) & 7)) return fail(MEMO_EINVAL, "d_scratch must be 8-byte aligned and not NULL");
    return MEMO_OK;
}

template <int MODE, bool PRIVATE>
int launch(const Args &A, size_t lds, unsigned grid, hipStream_t st) {
    if (lds > (64 << 10))  // above the default limit: opt in (per kernel and device)
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(spectrum_kernel<MODE, PRIVATE>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((spectrum_kernel<MODE, PRIVATE>), dim3(grid), dim3(kThreads), lds, st, A);
    return MEMO_OK;
}

}  // namespace

extern "C" {

size_t memo_spectrum_scratch_bytes(int32_t num_docs, int32_t kmax) {
    if (num_docs < 1 || num_docs > kMaxDocs || kmax < 1 || kmax > kMaxK) return 0;
    return table_cells(num_docs, kmax) * sizeof(uint64_t);
}

int32_t memo_spectrum_tile(int32_t num_docs, int32_t kmax, int32_t mode) {
    if (num_docs < 1 || num_docs > kMaxDocs || kmax < 1 || kmax > kMaxK || (mode != 0 && mode != 1)) return 0;
    return tile_of(kmax, mode);
}

int memo_spectrum_begin_dev(uint64_t *d_scratch, int32_t num_docs, int32_t kmax, int32_t device, void *stream) {
    if (int rc = check_shape(num_docs, kmax)) return rc;
    if (int rc = check_scratch(d_scratch)) return rc;
    OnDevice on(device);
    if (on.rc) return on.rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(d_scratch, 0, table_cells(num_docs, kmax) * sizeof(uint64_t), st));
    HIP_TRY(hipStreamSynchronize(st));
    return MEMO_OK;
}

int memo_spectrum_add_dev(const uint32_t *d_cells, int64_t L, int64_t pitch, int32_t num_docs, int32_t kmax, int32_t mode, uint64_t *d_scratch,
                          int32_t device, void *stream) {
    if (int rc = check_shape(num_docs, kmax)) return rc;
    if (mode != 0 && mode != 1) return fail(MEMO_EINVAL, "mode must be 0 (a conservation index) or 1 (a membership index) (got %d)", mode);
    if (L < 0 || L > kMaxL) return fail(MEMO_EINVAL, "a slice of %lld positions: L must be in [0, 2^31]", (long long)L);
    if (pitch < L || (pitch & 3)) return fail(MEMO_EINVAL, "pitch %lld: it must be a multiple of 4 and at least L = %lld", (long long)pitch, (long long)L);
    if ((int64_t)num_docs * pitch >= ((int64_t)1 << 32))
        return fail(MEMO_EINVAL, "%d planes of pitch %lld: 2^32 cells or more (take the window in slices)", num_docs, (long long)pitch);
    if (reinterpret_cast<uintptr_t>(d_cells) & 15) return fail(MEMO_EINVAL, "d_cells must be 16-byte aligned");
    if (L && !d_cells) return fail(MEMO_EINVAL, "d_cells is NULL");
    if (int rc = check_scratch(d_scratch)) return rc;
    if (!L) return MEMO_OK;
    OnDevice on(device);
    if (on.rc) return on.rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    Args A = {};
    A.cells = d_cells;
    A.D = reinterpret_cast<unsigned long long *>(d_scratch);
    A.L = L, A.pitch = pitch;
    A.n = num_docs, A.kmax = kmax;
    const int P = tile_of(kmax, mode);
    A.logp = 31 - __builtin_clz((unsigned)P);
    A.words = hist_words(kmax);
    A.ntiles = (L + P - 1) / P;
    const bool priv = table_fits(num_docs, kmax, mode);
    const size_t lds = (staging_words(kmax, mode) + (priv ? table_cells(num_docs, kmax) : 0)) * sizeof(uint32_t);
    const unsigned grid = (unsigned)std::min<int64_t>(A.ntiles, kMaxGrid);  // (2^31 positions over 2048 workgroups: 2^20 each)
    DevPtr<unsigned long long> counted;
    if (g_spectrum_timed & 2) {
        if (hipError_t err = counted.alloc(1); err != hipSuccess) return fail(MEMO_EHIP, "hipMalloc(8 bytes) for the atomics' count: %s", hipGetErrorString(err));
        HIP_TRY(hipMemsetAsync(counted.p, 0, sizeof(unsigned long long), st));
        A.counted = counted.p;
    }
    Laps laps(st, g_spectrum_timed, g_spectrum_ms);
    if (int rc = laps.start()) return rc;
    int rc;
    if (mode == 0) rc = priv ? launch<0, true>(A, lds, grid, st) : launch<0, false>(A, lds, grid, st);
    else rc = priv ? launch<1, true>(A, lds, grid, st) : launch<1, false>(A, lds, grid, st);
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    if (int rc2 = laps.lap(0)) return rc2;
    HIP_TRY(hipStreamSynchronize(st));
    g_spectrum_private = priv ? 1 : 0;
    if (A.counted) {
        unsigned long long got = 0;
        HIP_TRY(hipMemcpy(&got, counted.p, sizeof(got), hipMemcpyDeviceToHost));
        g_spectrum_atomics = got;
    }
    return MEMO_OK;
}

int memo_spectrum_finish_dev(const uint64_t *d_scratch, int32_t num_docs, int32_t kmax, uint64_t *d_exact, int32_t device, void *stream) {
    if (int rc = check_shape(num_docs, kmax)) return rc;
    if (int rc = check_scratch(d_scratch)) return rc;
    if (!d_exact || (reinterpret_cast<uintptr_t>(d_exact) & 7)) return fail(MEMO_EINVAL, "d_exact must be 8-byte aligned and not NULL");
    OnDevice on(device);
    if (on.rc) return on.rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    Laps laps(st, g_spectrum_timed, g_spectrum_ms);
    if (int rc = laps.start()) return rc;
    hipLaunchKernelGGL(spectrum_finish_kernel, dim3((unsigned)((num_docs + 1 + kFinishV - 1) / kFinishV)), dim3(kFinishV * kFinishParts), 0, st,
                       reinterpret_cast<const unsigned long long *>(d_scratch), reinterpret_cast<unsigned long long *>(d_exact), (int)num_docs, (int)kmax);
    HIP_TRY(hipGetLastError());
    if (int rc = laps.lap(1)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return MEMO_OK;
}

}  // extern "C"
