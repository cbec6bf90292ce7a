// memo_nearest.hip -- `memo nearest`: which genome of a membership index matches the pivot longest, position by position and bin by
// bin, from the finished lengths of `memo lengths` that are still in HBM: the argmax ACROSS the planes, where memo_breaks.hip and
// memo_pairs.hip reduce along them.  Haplotype painting: local ancestry, introgression, recombination breakpoints.  No counterpart
// in the reference.
//
// The cells are uint32 [planes][pitch], L of them per plane read (memo_lengths_finish_dev's layout, no halo: no cell has a neighbour
// relation here); v[g][p] = min(cell[g][p], cap).  C is the candidate set, a subset of 1 .. planes - 1 (bit g of 64 words; NULL:
// all of them): plane 0, the pivot's, is never a candidate and never read, and a plane outside C is not loaded.  Per position p
//     best[p]   = max{ v[g][p] : g in C }                 ok[p] = best[p] >= min_len
//     att[g][p] = g in C and ok[p] and v[g][p] == best[p]                       (every tied genome attains)
//     sole[g][p]= att[g][p] and no other genome attains at p
//     winner[p] = the smallest g with att[g][p], 0 where not ok[p]              uint16 [L], WRITTEN
// and per bin b, over the positions p of the slice in [edges[b], edges[b + 1])
//     wins[0][g][b] += #{ p : att[g][p] }     g >= 1;      wins[0][0][b] += #{ p : not ok[p] }       ("none")
//     wins[1][g][b] += #{ p : sole[g][p] }    g >= 1;      wins[1][0][b] += the same "none" count
//     sums[b]       += sum of best[p]                                            (min_len plays no part)
// uint64 [2][planes][bins] and uint64 [bins], ADDED to.  The launcher turns the edges into CELL coordinates as memo_breaks_dev does
// (edge - first clamped to [0, L], the first edge 0), so the bins cut [0, L) into consecutive runs and the kernel never sees `first`.
//
// A workgroup of 256 lanes takes a run of consecutive tiles of P positions (at most 1024 runs); P is the largest of 256, 128 ... 8
// whose LDS -- the staged tile, uint32 [planes][stride] with lengths_select_kernel's stride rule, the accumulators uint32
// [2][2][planes], three words per position and the 64 candidate words -- fits 72 KiB (nearest_tile): two workgroups share a CU's 160 KiB,
// which measured 1.7 times faster at 100 planes than one workgroup with a tile twice as long.  Per tile:
//   stage    the candidate rows with 16-byte loads, eight in flight per lane, clamped at the cap (a tile that crosses L: cell by cell)
//   phase A  S = 256 / P neighbouring lanes share a position, take the genomes part, part + S ... and fold (max, how many attain, the
//            lowest that attains) with wave shuffles; best, the flags sole / none and the winner per position go to LDS, the winner
//            to HBM where asked
//   phase B  the waves split the genomes; a wave reads row g along the tile (64 positions a read; at P < 64, 64 / P genomes a read),
//            compares with best, and the ballot of the comparison is counted by the lanes that begin a run of equal bin: population
//            counts under the run's mask.  A run in the bin the workgroup is in goes to acc[cur] in LDS, a run in the bin that goes
//            on into the next tile to acc[cur ^ 1], a run of a bin that begins and ends inside the tile to global memory directly.
//            "none" is row 0 of the same walk.  The sum of best stays in two registers a lane (this bin, the next) the same way.
//   flush    where the workgroup's bin ends: acc[cur] to global memory with 64-bit atomics (none for a zero), cleared; cur ^= 1
// The bin of a position is the workgroup's bin without a look at the edges while that bin goes on past the tile; a binary search
// between the workgroup's bin and the bin of the tile's end otherwise.
//
// Conditions the code holds:
//   - no workgroup waits for another: no look-back, no flag in memory, no cooperative launch
//   - nothing is read outside [0, L) of a plane or outside edges[0 .. bins]: a tile that crosses L is taken cell by cell, for the
//     cells before L.  The cells [L, pitch), plane 0 and the planes outside C are never read
//   - every cell of a candidate plane is loaded from global memory once per call
//   - the global atomics of a workgroup: at most 2 per genome and 1 for the sums for every bin it touches, and once more at its
//     end -- genomes x (bins it touches + 1), not genomes x tiles
//   - integer adds only, so the tables depend neither on the slicing nor on the launch shape.  The 32-bit counters in LDS cannot
//     wrap: the launcher refuses what would give a workgroup more than 2^31 cells
//   - vector loads and stores and plain C++ only; no inline assembly
//   - MEMO_EINVAL before any launch: d_cells not 16-byte aligned (or NULL where cells are read); pitch not a multiple of 4 or below
//     L; L < 0 or above 2^31; planes outside [2, 2048]; cap outside [1, 2^31 - 1]; min_len outside [1, cap]; a candidate set that is
//     empty, names bit 0 or names a bit at or past planes; all three outputs NULL; a table that is not 8-byte aligned, a winner that
//     is not 2-byte aligned; with a table: bins outside [1, 2^20 + 1], edges that are NULL or decrease, a slice that leaves the
//     edges (first < edges[0], or first + L > edges[bins]); without one: edges with bins != 0, or bins != 0 without edges
//   - L == 0 launches nothing and leaves everything as it was
//   - LDS above 64 KiB is opted into with hipFuncSetAttribute before the launch that needs it
//   - scratch: the uploaded edges ((bins + 1) x 8 bytes) and the 64 candidate words, owned by DevPtr; an allocation that fails is
//     MEMO_EHIP with the bytes asked for, and nothing stays allocated
#include <algorithm>
#include <vector>

#include "memo_common.h"

using namespace memo;

namespace memo {
thread_local int g_nearest_timed = 0;        // 1 = an event pair around the launch (memo_debug_nearest_times)
thread_local float g_nearest_ms = 0.f;       // ... of the last such call
thread_local int g_nearest_lds_kib = kNearestLdsKib;  // the LDS a workgroup may take (memo_debug_nearest_lds: the A/B of DESIGN.md 10.17)
}

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxBins = (1 << 20) + 1;      // memo_breaks_dev's
constexpr int kMaxPlanes = 2048;
constexpr int kCandWords = kMaxPlanes / 32;
constexpr int kMaxRuns = 1024;               // runs of tiles (workgroups) at most
constexpr int64_t kMaxCellsPerWg = (int64_t)1 << 31;
constexpr uint32_t kNever = 0xffffffffu;     // best where not ok: no clamped value is equal to it (cap < 2^31)

// (lengths_select_kernel's rule: the 64 addresses of a wave's read in phase A on 64 different banks)
constexpr int stride_of(int P) { return P == kThreads ? P : P + P / 4; }
// the LDS words of a workgroup: the tile, acc[2][2][n], best / flags / raw best per position, the candidate words
size_t lds_words(int n, int P) { return (size_t)n * stride_of(P) + 4 * (size_t)n + 3 * (size_t)P + kCandWords; }
int nearest_tile(int n) {
    for (int P = kThreads; P > 8; P >>= 1)
        if (lds_words(n, P) * sizeof(uint32_t) <= ((size_t)g_nearest_lds_kib << 10)) return P;
    return 8;  // (above 1310 planes more than the budget: 113 KiB at 2048, one workgroup a CU)
}

struct NearArgs {
    const uint32_t *cells;  // [planes][pitch]
    int64_t L, pitch, ntiles, tiles_per_wg;
    int planes, bins, all;  // all: every plane 1 .. planes - 1 is a candidate
    uint32_t cap, min_len;
    const uint32_t *cand;   // [64] words, bit g
    const int64_t *edges;   // [bins + 1], cell coordinates, non-decreasing, edges[0] == 0 and edges[bins] == L; NULL without a table
    uint64_t *wins;         // [2][planes][bins] or NULL
    uint64_t *sums;         // [bins] or NULL
    uint16_t *winner;       // [L] or NULL
};

// the first s in [lo, hi] with edges[s + 1] > p; the caller knows that edges[hi + 1] > p (memo_breaks.hip's)
__device__ inline int first_above(const int64_t *edges, int lo, int hi, int64_t p) {
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (edges[mid + 1] > p) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

__device__ inline uint64_t wave_sum(uint64_t x) {
#pragma unroll
    for (int o = 32; o; o >>= 1) x += __shfl_down(x, o);
    return x;  // (lane 0 holds the sum)
}

__device__ inline void add64(uint64_t *p, uint64_t x) { atomicAdd(reinterpret_cast<unsigned long long *>(p), (unsigned long long)x); }

template <int P>
__global__ __launch_bounds__(kThreads) void nearest_kernel(const NearArgs A) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    // S lanes a position in phase A; in phase B a wave's read is G rows of W positions, C of them along a row
    constexpr int S = kThreads / P, STRIDE = stride_of(P), W = P < 64 ? P : 64, C = P / W, G = 64 / W;
    const int n = A.planes, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t *vals = lds;                  // [n][STRIDE]: min(cell, cap) of the candidate rows; positions at or past L: 0
    uint32_t *acc = vals + n * STRIDE;     // [2][2][n]: [cur] the bin the workgroup is in, [cur ^ 1] the bin that goes on into the next tile
    uint32_t *bestk = acc + 4 * n;         // [P]: best where ok, kNever elsewhere
    uint32_t *flags = bestk + P;           // [P]: bit 0 sole, bit 1 none
    uint32_t *bestv = flags + P;           // [P]: best, 0 at or past L
    uint32_t *cw = bestv + P;              // [64]
    const bool tables = A.wins || A.sums;

    for (int i = tid; i < 4 * n; i += kThreads) acc[i] = 0;
    if (tid < kCandWords) cw[tid] = A.cand[tid];
    __syncthreads();
    auto is_cand = [&](int g) { return g >= 1 && g < n && (A.all || ((cw[g >> 5] >> (g & 31)) & 1u)); };

    const int64_t t0 = (int64_t)blockIdx.x * A.tiles_per_wg, t1 = min(t0 + A.tiles_per_wg, A.ntiles);
    int b = -2, cur = 0;                   // the workgroup's bin (there is one for its first cell: edges[bins] == L)
    int64_t bin_end = 0;
    if (tables) {
        b = first_above(A.edges, 0, A.bins - 1, t0 * P);
        bin_end = A.edges[b + 1];
    }
    uint64_t sum_cur = 0, sum_next = 0;    // the sum of best, a lane's share: this bin and the bin that goes on
    auto flush = [&]() {                   // every lane comes here, behind a barrier; b is a bin
        if (A.wins)
            for (int i = tid; i < 2 * n; i += kThreads) {  // i = which * n + g
                uint32_t *a = acc + cur * 2 * n + i;
                if (*a) add64(A.wins + (int64_t)i * A.bins + b, *a), *a = 0;
            }
        if (A.sums) {
            const uint64_t s = wave_sum(sum_cur);
            if (lane == 0 && s) add64(A.sums + b, s);
            sum_cur = sum_next, sum_next = 0;
        }
        cur ^= 1;
    };

    for (int64_t t = t0; t < t1; ++t) {
        const int64_t ts = t * P, te = min(ts + P, A.L);
        // ---- stage ----------------------------------------------------------------------------------------------------------
        if (ts + P <= A.L) {
            constexpr int Q = P / 4, kStage = 8;  // quads per row of the tile
            const int nquads = n * Q;
            for (int i0 = tid; i0 < nquads; i0 += kThreads * kStage) {
                uint4 v[kStage];
#pragma unroll
                for (int u = 0; u < kStage; ++u) {
                    const int i = i0 + u * kThreads;
                    if (i < nquads && is_cand(i / Q)) v[u] = *reinterpret_cast<const uint4 *>(A.cells + (int64_t)(i / Q) * A.pitch + ts + 4 * (i % Q));
                }
#pragma unroll
                for (int u = 0; u < kStage; ++u) {
                    const int i = i0 + u * kThreads;
                    if (i < nquads && is_cand(i / Q)) {
                        uint32_t *d = vals + (i / Q) * STRIDE + 4 * (i % Q);
                        d[0] = min(v[u].x, A.cap), d[1] = min(v[u].y, A.cap), d[2] = min(v[u].z, A.cap), d[3] = min(v[u].w, A.cap);
                    }
                }
            }
        } else {
            for (int i = tid; i < n * P; i += kThreads) {
                const int g = i / P, q = i % P;
                if (is_cand(g)) vals[g * STRIDE + q] = ts + q < A.L ? min(A.cells[(int64_t)g * A.pitch + ts + q], A.cap) : 0u;
            }
        }
        __syncthreads();
        // ---- phase A: best, how many attain, the lowest that attains ------------------------------------------------------------
        {
            const int pos = tid / S, part = tid % S;
            uint32_t best = 0;
            int cnt = 0, win = kMaxPlanes;
#pragma unroll 4
            for (int g = part; g < n; g += S) {
                if (!is_cand(g)) continue;
                const uint32_t v = vals[g * STRIDE + pos];
                if (v > best) best = v, cnt = 1, win = g;
                else if (v == best) ++cnt, win = min(win, g);
            }
#pragma unroll
            for (int d = 1; d < S; d <<= 1) {
                const uint32_t ob = (uint32_t)__shfl_xor((int)best, d);
                const int oc = __shfl_xor(cnt, d), ow = __shfl_xor(win, d);
                if (ob > best) best = ob, cnt = oc, win = ow;
                else if (ob == best) cnt += oc, win = min(win, ow);
            }
            if (part == 0) {
                const bool valid = ts + pos < A.L, ok = valid && best >= A.min_len;
                bestk[pos] = ok ? best : kNever;
                flags[pos] = (ok && cnt == 1 ? 1u : 0u) | (valid && !ok ? 2u : 0u);
                bestv[pos] = valid ? best : 0u;
                if (A.winner && valid) A.winner[ts + pos] = (uint16_t)(ok ? win : 0);
            }
        }
        __syncthreads();
        // ---- phase B: the ballots of v == best, counted run of equal bin by run ---------------------------------------------------
        const bool ends = tables && bin_end <= te;   // the workgroup's bin ends in this tile
        int tail = -2;                               // the bin that goes on into the next tile, where there is one
        if (tables) {
            if (ends && te < A.L) tail = first_above(A.edges, b + 1, A.bins - 1, te);
            const int qw = lane % W, sub = lane / W;
            uint64_t m[C], one[C];  // a run's mask in the lane that begins it (0 elsewhere); the positions with a sole winner
            int x[C];               // the lane's position's bin, -1 at or past L
            uint32_t bk[C];
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const int q = c * 64 + qw;
                const int64_t p = ts + q;
                int xx = -1;
                if (p < A.L) xx = !ends || p < bin_end ? b : first_above(A.edges, b + 1, tail >= 0 ? tail : A.bins - 1, p);
                const int before = __shfl_up(xx, 1, 64);
                const bool begins = qw == 0 || xx != before;
                const uint64_t rest = (__ballot(begins) >> lane) >> 1;
                const int len = rest ? __ffsll((unsigned long long)rest) : 64 - lane;
                m[c] = begins && xx >= 0 ? (len >= 64 ? ~0ull : ((1ull << len) - 1)) << lane : 0ull;
                x[c] = xx;
                const uint32_t fl = flags[q];
                one[c] = __ballot(fl & 1u);
                bk[c] = bestk[q];
                if (A.wins) {
                    const uint64_t none = __ballot((fl & 2u) && sub == 0);  // "none": row 0
                    if (wave == c % kWaves && m[c]) {
                        const uint32_t k = __popcll(none & m[c]);
                        if (k) {
                            if (xx == b || xx == tail) {
                                uint32_t *a = acc + (xx == b ? cur : cur ^ 1) * 2 * n;
                                atomicAdd(a, k), atomicAdd(a + n, k);
                            } else {
                                add64(A.wins + xx, k), add64(A.wins + (int64_t)n * A.bins + xx, k);
                            }
                        }
                    }
                }
                if (A.sums && wave == c % kWaves && sub == 0 && xx >= 0) {
                    const uint32_t v = bestv[q];
                    if (xx == b) sum_cur += v;
                    else if (xx == tail) sum_next += v;
                    else if (v) add64(A.sums + xx, v);
                }
            }
            if (A.wins)
                for (int gg = wave; gg * G < n; gg += kWaves) {
                    const int g = gg * G + sub;
                    const bool cand = is_cand(g);
                    if (G == 1 && !cand) continue;  // (the same in every lane)
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        const uint32_t v = cand ? vals[g * STRIDE + c * 64 + qw] : 0u;
                        const uint64_t att = __ballot(cand && v == bk[c]);
                        if (!m[c]) continue;
                        const uint32_t ka = __popcll(att & m[c]);
                        if (!ka) continue;
                        const uint32_t ks = __popcll(att & one[c] & m[c]);
                        if (x[c] == b || x[c] == tail) {
                            uint32_t *a = acc + (x[c] == b ? cur : cur ^ 1) * 2 * n + g;
                            atomicAdd(a, ka);
                            if (ks) atomicAdd(a + n, ks);
                        } else {
                            add64(A.wins + (int64_t)g * A.bins + x[c], ka);
                            if (ks) add64(A.wins + ((int64_t)n + g) * A.bins + x[c], ks);
                        }
                    }
                }
        }
        __syncthreads();
        if (ends) {
            flush();
            b = tail;
            if (b >= 0) bin_end = A.edges[b + 1];  // > te
        }
    }
    if (b >= 0) flush();
}

template <int P>
int launch_nearest(const NearArgs &A, int gx, hipStream_t st) {
    const size_t lds = lds_words(A.planes, P) * sizeof(uint32_t);
    if (lds > (64 << 10))  // above the default limit: opt in (per kernel and device)
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(nearest_kernel<P>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(nearest_kernel<P>, dim3((unsigned)gx), dim3(kThreads), lds, st, A);
    return MEMO_OK;
}

}  // namespace

extern "C" {

int32_t memo_nearest_tile(int32_t planes) { return planes < 2 || planes > kMaxPlanes ? 0 : nearest_tile(planes); }

int memo_nearest_dev(const uint32_t *d_cells, int64_t L, int64_t pitch, int32_t planes, uint32_t cap, uint32_t min_len, const uint32_t *cand_host,
                     int64_t first, const int64_t *edges_host, int32_t bins, uint64_t *d_wins, uint64_t *d_sums, uint16_t *d_winner, int32_t device,
                     void *stream) {
    if (planes < 2 || planes > kMaxPlanes) return fail(MEMO_EINVAL, "planes must be in [2, %d] (planes = %d)", kMaxPlanes, planes);
    if (L < 0 || L > ((int64_t)1 << 31)) return fail(MEMO_EINVAL, "L = %lld: a plane holds at most 2^31 cells", (long long)L);
    if (pitch < L || (pitch & 3)) return fail(MEMO_EINVAL, "pitch %lld must be a multiple of 4 and at least L = %lld", (long long)pitch, (long long)L);
    if (cap < 1 || cap > 0x7fffffffu) return fail(MEMO_EINVAL, "cap %u must be in [1, 2^31 - 1]", cap);
    if (min_len < 1 || min_len > cap) return fail(MEMO_EINVAL, "min_len %u must be in [1, cap = %u]", min_len, cap);
    if (reinterpret_cast<uintptr_t>(d_cells) & 15) return fail(MEMO_EINVAL, "d_cells must be 16-byte aligned");
    if (L && !d_cells) return fail(MEMO_EINVAL, "d_cells is NULL");
    uint32_t cand[kCandWords] = {};
    int all = 1;
    if (cand_host) {
        bool any = false;
        for (int w = 0; w < kCandWords; ++w) cand[w] = cand_host[w], any |= cand[w] != 0;
        if (!any) return fail(MEMO_EINVAL, "the candidate set is empty");
        if (cand[0] & 1u) return fail(MEMO_EINVAL, "the candidate set names genome 0: the pivot is never a candidate");
        for (int g = 0; g < kMaxPlanes; ++g) {
            const bool in = (cand[g >> 5] >> (g & 31)) & 1u;
            if (in && g >= planes) return fail(MEMO_EINVAL, "the candidate set names genome %d: there are %d planes", g, planes);
            if (!in && g >= 1 && g < planes) all = 0;
        }
    }
    if (!d_wins && !d_sums && !d_winner) return fail(MEMO_EINVAL, "d_wins, d_sums and d_winner are all NULL: nothing is asked for");
    if ((reinterpret_cast<uintptr_t>(d_wins) & 7) || (reinterpret_cast<uintptr_t>(d_sums) & 7))
        return fail(MEMO_EINVAL, "d_wins and d_sums must be 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_winner) & 1) return fail(MEMO_EINVAL, "d_winner must be 2-byte aligned");
    const bool tables = d_wins || d_sums;
    if (tables) {
        if (bins < 1 || bins > kMaxBins) return fail(MEMO_EINVAL, "bins must be in [1, %d] (bins = %d)", kMaxBins, bins);
        if (!edges_host) return fail(MEMO_EINVAL, "edges is NULL");
    } else if (edges_host ? bins < 1 || bins > kMaxBins : bins != 0) {
        return fail(MEMO_EINVAL, "bins = %d: without a table, 0 and no edges, or edges of [1, %d] bins", bins, kMaxBins);
    }
    if (edges_host) {
        for (int32_t s = 0; s < bins; ++s)
            if (edges_host[s + 1] < edges_host[s])
                return fail(MEMO_EINVAL, "the bin edges decrease: edge %d is %lld, edge %d is %lld", s, (long long)edges_host[s], s + 1,
                            (long long)edges_host[s + 1]);
        // (first + L cannot wrap where it matters: L <= edges[bins] - first is asked instead)
        if (first < edges_host[0] || first > edges_host[bins] || L > edges_host[bins] - first)
            return fail(MEMO_EINVAL, "the slice [%lld, %lld + %lld) leaves the bin edges [%lld, %lld)", (long long)first, (long long)first, (long long)L,
                        (long long)edges_host[0], (long long)edges_host[bins]);
    }
    if (!L) return MEMO_OK;

    NearArgs A = {};
    A.cells = d_cells;
    A.L = L;
    A.pitch = pitch;
    A.planes = planes;
    A.bins = tables ? bins : 0;
    A.all = all;
    A.cap = cap;
    A.min_len = min_len;
    A.wins = d_wins;
    A.sums = d_sums;
    A.winner = d_winner;
    const int P = nearest_tile(planes);
    A.ntiles = (L + P - 1) / P;
    const int64_t most = std::min<int64_t>(kMaxRuns, A.ntiles);
    A.tiles_per_wg = (A.ntiles + most - 1) / most;
    if (A.tiles_per_wg * P > kMaxCellsPerWg) return fail(MEMO_EINVAL, "a plane of %lld cells is too long", (long long)L);
    const int gx = (int)((A.ntiles + A.tiles_per_wg - 1) / A.tiles_per_wg);
    if (!cand_host)
        for (int g = 1; g < planes; ++g) cand[g >> 5] |= 1u << (g & 31);

    OnDevice on(device);
    if (on.rc) return on.rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    DevPtr<uint32_t> d_cand;
    if (hipError_t err = d_cand.alloc(kCandWords); err != hipSuccess)
        return fail(MEMO_EHIP, "hipMalloc(%zu bytes) for the candidate words: %s", sizeof cand, hipGetErrorString(err));
    HIP_TRY(hipMemcpyAsync(d_cand, cand, sizeof cand, hipMemcpyHostToDevice, st));
    A.cand = d_cand;
    // the edges in cell coordinates: [0, L) cut into consecutive bins, the first edge 0 and the last one L
    std::vector<int64_t> rel;
    DevPtr<int64_t> d_edges;
    if (tables) {
        rel.resize((size_t)bins + 1);
        for (int32_t s = 0; s <= bins; ++s) rel[s] = std::min<int64_t>(std::max<int64_t>(edges_host[s] - first, 0), L);
        rel[0] = 0;
        if (hipError_t err = d_edges.alloc(rel.size()); err != hipSuccess)
            return fail(MEMO_EHIP, "hipMalloc(%zu bytes) for the edges of %d bins: %s", rel.size() * sizeof(int64_t), bins, hipGetErrorString(err));
        HIP_TRY(hipMemcpyAsync(d_edges, rel.data(), rel.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
        A.edges = d_edges;
    }
    Laps laps(st, g_nearest_timed, &g_nearest_ms);
    if (int rc = laps.start()) return rc;
    int rc = MEMO_OK;
    switch (P) {
        case 256: rc = launch_nearest<256>(A, gx, st); break;
        case 128: rc = launch_nearest<128>(A, gx, st); break;
        case 64: rc = launch_nearest<64>(A, gx, st); break;
        case 32: rc = launch_nearest<32>(A, gx, st); break;
        case 16: rc = launch_nearest<16>(A, gx, st); break;
        default: rc = launch_nearest<8>(A, gx, st); break;
    }
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    if (int rc2 = laps.lap(0)) return rc2;
    HIP_TRY(hipStreamSynchronize(st));  // (cand, rel and the scratch go with this frame)
    return MEMO_OK;
}

}  // extern "C"
