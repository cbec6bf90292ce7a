// memo_mosaic.hip -- `memo mosaic`: the pivot as the fewest pieces, each copied whole from one genome of a membership index -- the greedy
// relative Lempel-Ziv parse by longest match -- from the finished lengths of `memo lengths` that are still in HBM.  Where `memo nearest`
// (memo_nearest.hip) paints every position with its own winner, this follows the winner's match to its end and asks again there.  No
// counterpart in the reference.
//
// FOLD (memo_mosaic_fold_dev): the cells are uint32 [planes][pitch], L of them per plane read (memo_lengths_finish_dev's layout, no
// halo); v[g][p] = min(cell[g][p], cap), C the candidate set exactly as memo_nearest_dev takes it.  Per position of the slice
//     best[p] = max{ v[g][p] : g in C }       ok[p] = best[p] >= min_len       winner[p] = the smallest g that attains best[p], 0 where not ok[p]
//     step[p] = ok[p] ? best[p] : 1           (a position no candidate reaches at min_len is a literal of one base)
// step uint32 [L] and winner uint16 [L], WRITTEN.  A plain streaming kernel, nothing staged: a lane owns four consecutive positions and
// reads 16 bytes a plane, walks the candidates in ascending order from a list in memory, eight loads in flight, clamps at the cap and
// replaces on strictly greater, so that the lowest annot keeps a tie.  The outputs are a slice's part of the whole window's vectors and
// sit at any element offset: a lane stores its four steps (winners) as one 16-byte (8-byte) store where the address allows it and
// one by one elsewhere; the quad that crosses L is read and written cell by cell.
//
// PARSE (memo_mosaic_parse_dev): step, winner, L -> the lines.  p_0 = 0, p_{i+1} = p_i + max(step[p_i], 1) while p_i < L are the REACHED
// positions; a reached p starts a line iff winner[p] != 0, or p == 0, or not (p - 1 is reached and winner[p - 1] == 0) -- consecutive
// phrases of no genome are one line, two phrases of one genome stay two.  With T positions a tile (memo_mosaic_tile), four steps,
// ordered by the stream:
//   exits  one workgroup per tile: nxt[i] = i + max(step, 1) as 32-bit tile-relative values in LDS (a step above 2^31 - 1 counts as
//          2^31 - 1: T - 1 + 2^31 - 1 fits 32 bits; in the last tile whatever lands at or past L has left the tile), then pointer
//          jumping nxt[i] = nxt[nxt[i]] while nxt[i] < T, a barrier a round, until a workgroup-wide vote says that every value has
//          left the tile and for log2 T + 1 rounds at most.  IN PLACE: a lane may read a value that another lane has already advanced
//          in the same round -- a 32-bit LDS word is read and written whole, and every value ever stored in nxt[j] lies further along
//          j's own chain, hence along i's; so a round never covers fewer hops than the synchronous one, r rounds cover at least 2^r,
//          and a chain has at most T hops inside its tile.  exit uint32 [L] goes to HBM; entry[tile] is set to the fill value.
//   walk   ONE lane: p = 0; while p < L: entry[p / T] = p % T; p = tile start + exit[p].  The only serial part: one dependent global
//          load per ENTERED tile.  Every hop lands in a strictly later tile; the loop also counts its hops and ends at the tile count.
//   mark   one workgroup per tile writes the tile's reached flags as a bitmap, T / 8 bytes, zeros included -- nothing is cleared
//          before.  An entered tile stages nxt again (16-bit: anything that leaves is T) and follows the chain from its entry, one of
//          two ways.  SERIAL: one lane walks the staged values, one dependent LDS read a hop.  DOUBLING: the mark rides the pointer
//          doubling -- after round r the first 2^r chain elements are marked, and the exact 2^r-jump applied to each marks the next
//          2^r; the jumps must be exact, so the rounds are synchronous and double-buffered (a mark set early in its round is still a
//          chain element and only marks chain elements).  Which one the product takes: kMosaicMark, from profiles/mosaic_timing.txt.
//   lines  memo_compact.h's compaction (count, scan, scatter; its own tile of 256 lanes x 4 loads x 8 positions): the key's flags()
//          applies the start rule to the bitmap and the winner, store() writes the winner as the payload; d_starts and d_genomes are
//          allocated for exactly the total and handed over.
//
// Conditions the code holds:
//   - no workgroup waits for another: no look-back, no flag in memory, no cooperative launch; the stream orders the launches
//   - fold: nothing is read outside [0, L) of a plane; the cells [L, pitch), plane 0 and the planes outside C are never read; every
//     cell of a candidate plane is loaded once; nothing is written outside [0, L) of the two outputs
//   - parse: nothing is read or written outside [0, L) of step, winner and exit; the bitmap holds whole tiles, and no bit at or past L
//     is ever set; a step of 0 counts as 1, so no input stalls a chain; every loop over a chain carries its own bound
//   - vector loads and stores and plain C++ only; no inline assembly
//   - MEMO_EINVAL before any launch, the outputs as they were: what memo_nearest_dev refuses of cells, pitch, L, planes, cap, min_len
//     and the candidate words; L above 2^31 - 1; d_step NULL or not 4-byte aligned, d_winner NULL or not 2-byte aligned (fold);
//     d_step or d_winner NULL or not 16-byte aligned (parse: they are whole vectors); NULL out-pointers
//   - L == 0 launches nothing; parse then returns zero lines and NULL arrays
//   - LDS above 64 KiB is opted into with hipFuncSetAttribute before the launch that needs it
//   - scratch: the candidate list (fold); exit (4 L bytes), the bitmap (T / 8 bytes a tile), entry (4 bytes a tile) and the compaction's
//     work area (parse), owned by DevPtr and freed before the call returns; an allocation that fails is MEMO_EHIP with the bytes asked
//     for, and nothing stays allocated
#include <algorithm>

#include "memo_compact.h"

using namespace memo;

namespace memo {
thread_local int g_mosaic_timed = 0;                               // 1 = event pairs around the launches (memo_debug_mosaic_times)
thread_local float g_mosaic_ms[5] = {0.f, 0.f, 0.f, 0.f, 0.f};     // ... of the last such calls: fold, exits, walk, mark, lines
thread_local int g_mosaic_tile = kMosaicTile;                      // positions a tile (memo_debug_mosaic_shape: the A/B of DESIGN.md 10.18)
thread_local int g_mosaic_mark = kMosaicMark;                      // 1 the serial lane, 2 the doubling mark
}

namespace {

constexpr int kFoldThreads = 256, kFoldFlight = 8;
constexpr int kMaxPlanes = 2048;
constexpr int kCandWords = kMaxPlanes / 32;
constexpr uint32_t kNotEntered = 0xffffffffu;  // entry[] of a tile the chain never enters
constexpr uint32_t kMaxStep = 0x7fffffffu;

// ---- fold ---------------------------------------------------------------------------------------------------------------------------
struct FoldArgs {
    const uint32_t *cells;  // [planes][pitch]
    int64_t L, pitch;
    int ncand;
    uint32_t cap, min_len;
    const int32_t *cand;    // [ncand], ascending
    uint32_t *step;         // [L]
    uint16_t *winner;       // [L]
};

__global__ __launch_bounds__(kFoldThreads) void mosaic_fold_kernel(const FoldArgs A) {
    const int64_t p = ((int64_t)blockIdx.x * kFoldThreads + threadIdx.x) * 4;
    if (p >= A.L) return;
    uint32_t best[4] = {0, 0, 0, 0}, win[4] = {0, 0, 0, 0};
    const bool full = p + 4 <= A.L;
    const int n = full ? 4 : (int)(A.L - p);
    if (full) {
        for (int c0 = 0; c0 < A.ncand; c0 += kFoldFlight) {
            uint4 v[kFoldFlight];
            int g[kFoldFlight];
#pragma unroll
            for (int u = 0; u < kFoldFlight; ++u)
                if (c0 + u < A.ncand) {
                    g[u] = A.cand[c0 + u];
                    v[u] = *reinterpret_cast<const uint4 *>(A.cells + (int64_t)g[u] * A.pitch + p);
                }
#pragma unroll
            for (int u = 0; u < kFoldFlight; ++u)
                if (c0 + u < A.ncand) {
                    const uint32_t x[4] = {min(v[u].x, A.cap), min(v[u].y, A.cap), min(v[u].z, A.cap), min(v[u].w, A.cap)};
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (x[j] > best[j]) best[j] = x[j], win[j] = (uint32_t)g[u];
                }
        }
    } else {
        for (int c = 0; c < A.ncand; ++c) {
            const int g = A.cand[c];
            for (int j = 0; j < n; ++j) {
                const uint32_t x = min(A.cells[(int64_t)g * A.pitch + p + j], A.cap);
                if (x > best[j]) best[j] = x, win[j] = (uint32_t)g;
            }
        }
    }
    uint32_t s[4];
    uint16_t w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool ok = best[j] >= A.min_len;
        s[j] = ok ? best[j] : 1u;
        w[j] = (uint16_t)(ok ? win[j] : 0u);
    }
    uint32_t *sp = A.step + p;
    if (full && !(reinterpret_cast<uintptr_t>(sp) & 15)) {
        *reinterpret_cast<uint4 *>(sp) = make_uint4(s[0], s[1], s[2], s[3]);
    } else {
        for (int j = 0; j < n; ++j) sp[j] = s[j];
    }
    uint16_t *wp = A.winner + p;
    if (full && !(reinterpret_cast<uintptr_t>(wp) & 7)) {
        *reinterpret_cast<uint2 *>(wp) = make_uint2((uint32_t)w[0] | ((uint32_t)w[1] << 16), (uint32_t)w[2] | ((uint32_t)w[3] << 16));
    } else {
        for (int j = 0; j < n; ++j) wp[j] = w[j];
    }
}

// ---- parse --------------------------------------------------------------------------------------------------------------------------
constexpr int log2_of(int t) { return t <= 1 ? 0 : 1 + log2_of(t >> 1); }
constexpr int tile_threads(int T) { return T / 16 > 1024 ? 1024 : T / 16; }  // 256 at 4096 ... 1024 from 16384 on

// the four steps of the quad at tile-relative position i (a multiple of 4): one 16-byte load where the quad lies before L
__device__ __forceinline__ void load_steps(const uint32_t *__restrict__ step, int64_t ts, int i, int64_t L, uint32_t (&s)[4]) {
    const int64_t p = ts + i;
    if (p + 4 <= L) {
        const uint4 q = *reinterpret_cast<const uint4 *>(step + p);
        s[0] = q.x, s[1] = q.y, s[2] = q.z, s[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] = p + j < L ? step[p + j] : 1u;
    }
}

// where position i of the tile at ts goes: tile-relative, T or more once it has left the tile; whatever lands at or past L has left it
template <int T>
__device__ __forceinline__ uint32_t next_of(int i, uint32_t s, int64_t ts, int64_t L) {
    uint32_t n = (uint32_t)i + min(max(s, 1u), kMaxStep);
    if (n < (uint32_t)T && ts + n >= L) n = T;
    return n;
}

template <int T>
__global__ __launch_bounds__(1024) void mosaic_exits_kernel(const uint32_t *__restrict__ step, int64_t L, uint32_t *__restrict__ exits,
                                                           uint32_t *__restrict__ entry) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    volatile uint32_t *nxt = lds;  // [T]
    const int tid = threadIdx.x, nt = blockDim.x;
    const int64_t ts = (int64_t)blockIdx.x * T;
    if (tid == 0) entry[blockIdx.x] = kNotEntered;
    for (int q = tid; q < T / 4; q += nt) {
        uint32_t s[4];
        load_steps(step, ts, 4 * q, L, s);
#pragma unroll
        for (int j = 0; j < 4; ++j) nxt[4 * q + j] = next_of<T>(4 * q + j, s[j], ts, L);
    }
    __syncthreads();
    // in place (see the head of the file): every value read lies further along i's own chain
    for (int r = 0; r <= log2_of(T); ++r) {
        int more = 0;
        for (int i = tid; i < T; i += nt) {
            const uint32_t v = nxt[i];
            if (v < (uint32_t)T) {
                const uint32_t v2 = nxt[v];
                nxt[i] = v2;
                more |= v2 < (uint32_t)T;
            }
        }
        if (!__syncthreads_or(more)) break;
    }
    for (int q = tid; q < T / 4; q += nt) {
        const int64_t p = ts + 4 * q;
        if (p + 4 <= L) {
            *reinterpret_cast<uint4 *>(exits + p) = make_uint4(nxt[4 * q], nxt[4 * q + 1], nxt[4 * q + 2], nxt[4 * q + 3]);
        } else {
            for (int j = 0; j < 4; ++j)
                if (p + j < L) exits[p + j] = nxt[4 * q + j];
        }
    }
}

template <int T>
__global__ void mosaic_walk_kernel(const uint32_t *__restrict__ exits, int64_t L, int64_t ntiles, uint32_t *__restrict__ entry) {
    if (threadIdx.x || blockIdx.x) return;
    int64_t p = 0;
    for (int64_t hops = 0; p < L && hops < ntiles; ++hops) {
        const int64_t t = p / T;
        entry[t] = (uint32_t)(p - t * T);
        p = t * T + exits[p];  // (at least T: a strictly later tile)
    }
}

template <int T, bool kDoubling>
__global__ __launch_bounds__(1024) void mosaic_mark_kernel(const uint32_t *__restrict__ step, int64_t L, const uint32_t *__restrict__ entry,
                                                          uint32_t *__restrict__ reached) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    uint32_t *bm = lds;                                            // [T / 32]: bit i = position i of the tile is reached
    uint16_t *a = reinterpret_cast<uint16_t *>(lds + T / 32);      // [T]: where i goes, T once it has left the tile
    uint16_t *b = a + T;                                           // [T]: the other buffer of the doubling rounds
    const int tid = threadIdx.x, nt = blockDim.x;
    const int64_t ts = (int64_t)blockIdx.x * T;
    uint32_t *out = reached + (int64_t)blockIdx.x * (T / 32);
    const uint32_t e = entry[blockIdx.x];  // (the same in every lane)
    if (e >= (uint32_t)T) {
        for (int k = tid; k < T / 32; k += nt) out[k] = 0u;
        return;
    }
    for (int k = tid; k < T / 32; k += nt) bm[k] = 0u;
    for (int q = tid; q < T / 4; q += nt) {
        uint32_t s[4];
        load_steps(step, ts, 4 * q, L, s);
#pragma unroll
        for (int j = 0; j < 4; ++j) a[4 * q + j] = (uint16_t)min(next_of<T>(4 * q + j, s[j], ts, L), (uint32_t)T);
    }
    __syncthreads();
    if (!kDoubling) {
        if (tid == 0) {
            uint32_t i = e;
            for (int hops = 0; i < (uint32_t)T && hops < T; ++hops) {
                bm[i >> 5] |= 1u << (i & 31);
                i = a[i];
            }
        }
    } else {
        if (tid == 0) bm[e >> 5] = 1u << (e & 31);
        __syncthreads();
        const volatile uint32_t *seen = bm;
        uint16_t *from = a, *to = b;
        for (int r = 0; r <= log2_of(T); ++r) {  // from[i]: exactly 2^r hops from i, or T
            int more = 0;
            for (int i = tid; i < T; i += nt) {
                const uint32_t j = from[i];
                uint32_t jj = j;
                if (j < (uint32_t)T) {
                    if ((seen[i >> 5] >> (i & 31)) & 1u) {
                        atomicOr(&bm[j >> 5], 1u << (j & 31));
                        more = 1;
                    }
                    jj = from[j];
                }
                to[i] = (uint16_t)jj;
            }
            if (!__syncthreads_or(more)) break;
            uint16_t *x = from;
            from = to, to = x;
        }
    }
    __syncthreads();
    for (int k = tid; k < T / 32; k += nt) out[k] = bm[k];
}

// the lines as a key of memo_compact.h's compaction: a lane owns the eight positions of one byte of the bitmap and of one 16-byte load
// of the winner
struct LinesKey {
    static constexpr int kPer = 8;
    using Start = int64_t;
    const uint8_t *reached;  // the bitmap: bit (p & 7) of byte p >> 3; no bit at or past L is set
    const uint16_t *winner;  // [L], 16-byte aligned
    uint16_t *payload;       // genomes[]
    int64_t L;

    __device__ __forceinline__ void tile_of(int64_t block, int64_t &plane, int64_t &p0) const { plane = 0, p0 = block * tile_positions<LinesKey>(); }

    // bit j: position p + j (p a multiple of 8) starts a line.  Called by whole waves (it shuffles).
    __device__ __forceinline__ uint32_t flags(int64_t, int64_t p) const {
        uint32_t r = 0, none = 0;
        if (p < L) {
            r = reached[p >> 3];
            uint16_t w[kPer];
            if (p + kPer <= L) {
                const uint4 q = *reinterpret_cast<const uint4 *>(winner + p);
                memcpy(w, &q, 16);
            } else {
#pragma unroll
                for (int j = 0; j < kPer; ++j) w[j] = p + j < L ? winner[p + j] : uint16_t(1);
            }
#pragma unroll
            for (int j = 0; j < kPer; ++j) none |= (uint32_t)(w[j] == 0) << j;
        }
        const uint32_t open = r & none;  // reached, and of no genome: the position behind it goes on with its line
        uint32_t prev = (uint32_t)__shfl_up((int)(open >> (kPer - 1)), 1, 64);
        if ((threadIdx.x & 63) == 0 && p > 0 && p < L) prev = ((reached[(p - 1) >> 3] >> ((p - 1) & 7)) & 1u) && winner[p - 1] == 0;
        if (p == 0) prev = 0;
        const uint32_t before = ((open << 1) | (prev & 1u)) & 0xffu;
        return r & (~none | ~before) & 0xffu;
    }

    __device__ __forceinline__ void store(int64_t, int64_t rank, int64_t i) const { payload[rank] = winner[i]; }
};

size_t exits_lds(int T) { return (size_t)T * sizeof(uint32_t); }
size_t mark_lds(int T, bool doubling) { return (size_t)T / 8 + (size_t)T * sizeof(uint16_t) * (doubling ? 2 : 1); }

template <typename K>
int opt_in(K kernel, size_t lds) {
    if (lds > (64 << 10))  // above the default limit: opt in (per kernel and device)
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return MEMO_OK;
}

// exits, walk, mark: the reached bitmap of a window of ntiles tiles of T positions
template <int T>
int reach(const uint32_t *d_step, int64_t L, int64_t ntiles, uint32_t *d_exit, uint32_t *d_entry, uint32_t *d_reached, int mark, Laps &laps,
          hipStream_t st) {
    const dim3 grid((unsigned)ntiles), block(tile_threads(T));
    // (the opt-ins before the first event: no lap holds a host call)
    if (int rc = opt_in(mosaic_exits_kernel<T>, exits_lds(T))) return rc;
    if (int rc = mark == 2 ? opt_in(mosaic_mark_kernel<T, true>, mark_lds(T, true)) : opt_in(mosaic_mark_kernel<T, false>, mark_lds(T, false))) return rc;
    if (int rc = laps.start()) return rc;
    hipLaunchKernelGGL(mosaic_exits_kernel<T>, grid, block, exits_lds(T), st, d_step, L, d_exit, d_entry);
    HIP_TRY(hipGetLastError());
    if (int rc = laps.lap(1)) return rc;
    hipLaunchKernelGGL(mosaic_walk_kernel<T>, dim3(1), dim3(64), 0, st, d_exit, L, ntiles, d_entry);
    HIP_TRY(hipGetLastError());
    if (int rc = laps.lap(2)) return rc;
    if (mark == 2) {
        hipLaunchKernelGGL((mosaic_mark_kernel<T, true>), grid, block, mark_lds(T, true), st, d_step, L, d_entry, d_reached);
    } else {
        hipLaunchKernelGGL((mosaic_mark_kernel<T, false>), grid, dim3(256), mark_lds(T, false), st, d_step, L, d_entry, d_reached);
    }
    HIP_TRY(hipGetLastError());
    return laps.lap(3);
}

}  // namespace

extern "C" {

int32_t memo_mosaic_tile(void) { return g_mosaic_tile; }

int memo_mosaic_fold_dev(const uint32_t *d_cells, int64_t L, int64_t pitch, int32_t planes, uint32_t cap, uint32_t min_len, const uint32_t *cand_host,
                         uint32_t *d_step, uint16_t *d_winner, int32_t device, void *stream) {
    if (planes < 2 || planes > kMaxPlanes) return fail(MEMO_EINVAL, "planes must be in [2, %d] (planes = %d)", kMaxPlanes, planes);
    if (L < 0 || L > 0x7fffffffLL) return fail(MEMO_EINVAL, "L = %lld: a window holds at most 2^31 - 1 positions", (long long)L);
    if (pitch < L || (pitch & 3)) return fail(MEMO_EINVAL, "pitch %lld must be a multiple of 4 and at least L = %lld", (long long)pitch, (long long)L);
    if (cap < 1 || cap > 0x7fffffffu) return fail(MEMO_EINVAL, "cap %u must be in [1, 2^31 - 1]", cap);
    if (min_len < 1 || min_len > cap) return fail(MEMO_EINVAL, "min_len %u must be in [1, cap = %u]", min_len, cap);
    if (reinterpret_cast<uintptr_t>(d_cells) & 15) return fail(MEMO_EINVAL, "d_cells must be 16-byte aligned");
    if (L && !d_cells) return fail(MEMO_EINVAL, "d_cells is NULL");
    std::vector<int32_t> cand;
    if (cand_host) {
        bool any = false;
        for (int w = 0; w < kCandWords; ++w) any |= cand_host[w] != 0;
        if (!any) return fail(MEMO_EINVAL, "the candidate set is empty");
        if (cand_host[0] & 1u) return fail(MEMO_EINVAL, "the candidate set names genome 0: the pivot is never a candidate");
        for (int g = 1; g < kMaxPlanes; ++g) {
            if (!((cand_host[g >> 5] >> (g & 31)) & 1u)) continue;
            if (g >= planes) return fail(MEMO_EINVAL, "the candidate set names genome %d: there are %d planes", g, planes);
            cand.push_back(g);
        }
    } else {
        for (int g = 1; g < planes; ++g) cand.push_back(g);
    }
    if (!d_step || !d_winner) return fail(MEMO_EINVAL, "d_step / d_winner is NULL");
    if (reinterpret_cast<uintptr_t>(d_step) & 3) return fail(MEMO_EINVAL, "d_step must be 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_winner) & 1) return fail(MEMO_EINVAL, "d_winner must be 2-byte aligned");
    if (!L) return MEMO_OK;

    OnDevice on(device);
    if (on.rc) return on.rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    DevPtr<int32_t> d_cand;
    if (hipError_t err = d_cand.alloc(cand.size()); err != hipSuccess)
        return fail(MEMO_EHIP, "hipMalloc(%zu bytes) for the candidate list: %s", cand.size() * sizeof(int32_t), hipGetErrorString(err));
    HIP_TRY(hipMemcpyAsync(d_cand, cand.data(), cand.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    const FoldArgs A = {d_cells, L, pitch, (int)cand.size(), cap, min_len, d_cand, d_step, d_winner};
    const int64_t quads = (L + 3) / 4, blocks = (quads + kFoldThreads - 1) / kFoldThreads;  // (at most 2^21 blocks)
    Laps laps(st, g_mosaic_timed, g_mosaic_ms);
    if (int rc = laps.start()) return rc;
    hipLaunchKernelGGL(mosaic_fold_kernel, dim3((unsigned)blocks), dim3(kFoldThreads), 0, st, A);
    HIP_TRY(hipGetLastError());
    if (int rc = laps.lap(0)) return rc;
    HIP_TRY(hipStreamSynchronize(st));  // (the candidate list goes with this frame)
    return MEMO_OK;
}

int memo_mosaic_parse_dev(const uint32_t *d_step, const uint16_t *d_winner, int64_t L, int64_t **d_starts, uint16_t **d_genomes, uint64_t *lines,
                          int32_t device, void *stream) {
    if (!d_starts || !d_genomes || !lines) return fail(MEMO_EINVAL, "d_starts / d_genomes / lines is NULL");
    if (L < 0 || L > 0x7fffffffLL) return fail(MEMO_EINVAL, "L = %lld: a window holds at most 2^31 - 1 positions", (long long)L);
    if ((reinterpret_cast<uintptr_t>(d_step) & 15) || (reinterpret_cast<uintptr_t>(d_winner) & 15))
        return fail(MEMO_EINVAL, "d_step and d_winner must be 16-byte aligned");
    if (L && (!d_step || !d_winner)) return fail(MEMO_EINVAL, "d_step / d_winner is NULL");
    *d_starts = nullptr;
    *d_genomes = nullptr;
    *lines = 0;
    if (!L) return MEMO_OK;

    const int T = g_mosaic_tile, mark = g_mosaic_mark;
    const int64_t ntiles = (L + T - 1) / T;
    OnDevice on(device);
    if (on.rc) return on.rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    DevPtr<uint32_t> d_exit, d_entry, d_reached;
    const size_t reached_words = (size_t)ntiles * (size_t)(T / 32);
    if (hipError_t err = d_exit.alloc((size_t)L); err != hipSuccess)
        return fail(MEMO_EHIP, "hipMalloc(%zu bytes) for the exits of %lld positions: %s", (size_t)L * 4, (long long)L, hipGetErrorString(err));
    if (hipError_t err = d_entry.alloc((size_t)ntiles); err != hipSuccess)
        return fail(MEMO_EHIP, "hipMalloc(%zu bytes) for the entries of %lld tiles: %s", (size_t)ntiles * 4, (long long)ntiles, hipGetErrorString(err));
    if (hipError_t err = d_reached.alloc(reached_words); err != hipSuccess)
        return fail(MEMO_EHIP, "hipMalloc(%zu bytes) for the reached flags of %lld tiles: %s", reached_words * 4, (long long)ntiles, hipGetErrorString(err));
    {
        Laps laps(st, g_mosaic_timed, g_mosaic_ms);
        int rc = MEMO_OK;
        switch (T) {
            case 4096: rc = reach<4096>(d_step, L, ntiles, d_exit, d_entry, d_reached, mark, laps, st); break;
            case 8192: rc = reach<8192>(d_step, L, ntiles, d_exit, d_entry, d_reached, mark, laps, st); break;
            case 16384: rc = reach<16384>(d_step, L, ntiles, d_exit, d_entry, d_reached, mark, laps, st); break;
            default: rc = reach<32768>(d_step, L, ntiles, d_exit, d_entry, d_reached, mark, laps, st); break;
        }
        if (rc) return rc;
    }
    d_exit.reset();  // (queued behind the walk: hipFree waits for the device)

    // ---- lines: count, scan, allocate exactly, scatter ----
    float ms3[3] = {0.f, 0.f, 0.f};
    LinesKey key = {reinterpret_cast<const uint8_t *>(d_reached.p), d_winner, nullptr, L};
    constexpr int64_t CT = tile_positions<LinesKey>();
    Compaction c(st, g_mosaic_timed, ms3);
    if (hipError_t err = c.lay_out((L + CT - 1) / CT, 0); err != hipSuccess)
        return fail(MEMO_EHIP, "hipMalloc(%zu bytes) for the counts of %lld tiles: %s", c.work_bytes, (long long)((L + CT - 1) / CT), hipGetErrorString(err));
    if (int rc = c.count(key)) return rc;
    const int64_t total = c.total();
    if (total <= 0) return fail(MEMO_EHIP, "a window of %lld positions parsed into no line", (long long)L);  // (position 0 starts one)
    DevPtr<int64_t> starts;
    DevPtr<uint16_t> genomes;
    if (hipError_t err = starts.alloc((size_t)total); err != hipSuccess)
        return fail(MEMO_EHIP, "hipMalloc(%zu bytes) for the starts of %lld lines: %s", (size_t)total * 8, (long long)total, hipGetErrorString(err));
    if (hipError_t err = genomes.alloc((size_t)total); err != hipSuccess)
        return fail(MEMO_EHIP, "hipMalloc(%zu bytes) for the genomes of %lld lines: %s", (size_t)total * 2, (long long)total, hipGetErrorString(err));
    key.payload = genomes;
    if (int rc = c.scatter(key, starts.p)) return rc;
    if (g_mosaic_timed) g_mosaic_ms[4] = ms3[0] + ms3[1] + ms3[2];
    *lines = (uint64_t)total;
    *d_starts = starts.release();
    *d_genomes = genomes.release();
    return MEMO_OK;
}

}  // extern "C"
