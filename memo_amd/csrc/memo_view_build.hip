// memo_view_build.hip -- HOW a k-class view of an index's rows is made: the kernels and the three passes that run them.
//
// A view holds the rows whose overlap is below its class's cap, with a bucket table of its own (memo_view.hip: which classes, and
// when one is worth its pass).  Dense rows: count -> scan -> one fused pass that compacts, places the rows inside their 16-byte
// groups against LDS bank conflicts and packs them (dense_view_build); the copy of a placed six-row view without its dead groups
// (live_view_copy); 4-byte words: keep / scan / scatter (packed_filter).  A pass takes a source and hands back a BuiltView
// (memo_view.h): nothing here knows of classes, ledgers or budgets.
#include "memo_view.h"

using namespace memo;

namespace {

// two-level exclusive scan of count[] (n entries): local[i] = prefix inside i's block of 1024, blocksum[b] = the block's total
__global__ __launch_bounds__(256) void scan_local_kernel(const uint32_t *count, uint64_t n, uint32_t *local, uint64_t *blocksum) {
    __shared__ uint32_t part[256];
    const uint64_t base = blockIdx.x * (uint64_t)1024 + 4 * threadIdx.x;
    uint32_t v[4], sum = 0;
    for (int i = 0; i < 4; ++i) {
        v[i] = base + i < n ? count[base + i] : 0;
        sum += v[i];
    }
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const uint32_t add = threadIdx.x >= (unsigned)d ? part[threadIdx.x - d] : 0;
        __syncthreads();
        part[threadIdx.x] += add;
        __syncthreads();
    }
    uint32_t run = part[threadIdx.x] - sum;
    for (int i = 0; i < 4; ++i) {
        if (base + i < n) local[base + i] = run;
        run += v[i];
    }
    if (threadIdx.x == 255) blocksum[blockIdx.x] = part[255];
}

// exclusive scan of blocksum[] in place (one workgroup; nb entries), total -> blocksum[nb]
__global__ __launch_bounds__(1024) void scan_blocks_kernel(uint64_t *blocksum, uint64_t nb) {
    __shared__ uint64_t part[1024];
    __shared__ uint64_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (uint64_t at = 0; at < nb; at += 1024) {
        const uint64_t i = at + threadIdx.x;
        const uint64_t v = i < nb ? blocksum[i] : 0;
        part[threadIdx.x] = v;
        __syncthreads();
        for (int d = 1; d < 1024; d <<= 1) {
            const uint64_t add = threadIdx.x >= (unsigned)d ? part[threadIdx.x - d] : 0;
            __syncthreads();
            part[threadIdx.x] += add;
            __syncthreads();
        }
        if (i < nb) blocksum[i] = carry + part[threadIdx.x] - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry += part[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0) blocksum[nb] = carry;
}

__device__ __forceinline__ uint64_t kept_before(uint64_t r, const uint32_t *keep, const uint32_t *local, const uint64_t *blockpre) {
    const uint64_t w = r >> 5;
    return blockpre[w >> 10] + local[w] + (uint32_t)__popc(keep[w] & ((1u << (r & 31)) - 1u));
}

// boff3[b] = rows that stay among the first boff[b] rows; the last entry is pinned to the total
__global__ void dense_table_kernel(const int64_t *boff, uint64_t nb, uint64_t rows, uint64_t total, const uint32_t *keep,
                                   const uint32_t *local, const uint64_t *blockpre, int64_t *boff3) {
    const uint64_t b = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (b >= nb) return;
    const uint64_t r = (uint64_t)boff[b];
    boff3[b] = (b == nb - 1 || r >= rows) ? (int64_t)total : (int64_t)kept_before(r, keep, local, blockpre);
}

// the same for the 4-byte words (formats 4 and 12): keep the rows whose overlap byte is below cap
__global__ __launch_bounds__(256) void packed_keep_kernel(const uint32_t *pk, uint64_t rows, int len_shift, uint32_t cap, uint32_t *keep,
                                                          uint32_t *count) {
    const uint64_t top = (rows + 255) & ~(uint64_t)255;
    for (uint64_t r = blockIdx.x * (uint64_t)256 + threadIdx.x; r < top; r += (uint64_t)gridDim.x * 256) {
        const uint32_t len = r < rows ? (pk[r] >> len_shift) & 0xFFu : 255u;
        const unsigned long long m = __ballot(r < rows && len < cap);
        const int lane = threadIdx.x & 63;
        if ((lane & 31) == 0 && (r >> 5) < ((rows + 31) >> 5)) {
            const uint32_t half = (uint32_t)(m >> (lane & 32));
            keep[r >> 5] = half;
            count[r >> 5] = (uint32_t)__popc(half);
        }
    }
}

__global__ __launch_bounds__(256) void packed_scatter_kernel(const uint32_t *pk, uint64_t rows, const uint32_t *keep, const uint32_t *local,
                                                             const uint64_t *blockpre, uint32_t *out) {
    for (uint64_t r = blockIdx.x * (uint64_t)256 + threadIdx.x; r < rows; r += (uint64_t)gridDim.x * 256)
        if ((keep[r >> 5] >> (r & 31)) & 1u) out[kept_before(r, keep, local, blockpre)] = pk[r];
}

// ======================================================================================================================
// Dense k-class views, round 5: count -> scan -> ONE fused pass.
//
// Round 4 built a dense view with five kernels -- keep bits (a lane per ROW: five lanes fetched the same 16 bytes), a scatter
// to 4-byte words, the places of the rows inside their groups chosen by one LANE per bucket straight from HBM with one wave per
// workgroup and 42 KiB of LDS (4.0 ms for config 3: three waves per CU, every lane on its own cache lines), the packing, a
// table -- 8.2 ms for BASELINE config 3 at k = 31, the price of 65 whole-chromosome sweeps.  Now:
//   1. view_count_kernel: a lane per 16-byte GROUP: the five keep bits of its rows as a byte, kept rows per 64 groups;
//   2. the two-level scan of those counts; view_table_kernel: the view's bucket table (kept rows before every bucket);
//   3. view_build_kernel<P>: one WAVE per run of up to 64 buckets: streams the run's source groups with coalesced 16-byte
//      loads (the source is read twice in all, nothing else), compacts the kept rows into LDS in source order (ballot +
//      mbcnt: deterministic), then lane j takes bucket j of the run: the
//      choice of one of P places per row (view_place_bucket: round 4's greedy rule, taken with colour MASKS per bank instead of
//      bank masks per colour and without its sort) -- when places were asked for -- and the wave packs the
//      groups and writes them with coalesced 16-byte stores.  P = 5: PackedRows3 groups, the view's rows back to back (a
//      group may straddle two buckets: the two edge groups of a run are written with atomicOr into zeroed groups); P = 6:
//      groups of six rows that carry their bucket and end at bucket boundaries (2.67 B per row; memo_sweep_dense.h:
//      group_rows6), places a bucket leaves empty hold a copy of its last row (min is idempotent).
// A bucket whose kept rows do not fit the LDS stage streams through it in pieces, in source order.
// ======================================================================================================================
// kept rows a piece stages (+ 8 carried): with places, the rows of 64 buckets of BASELINE's shape (a lane each: 39 KiB of LDS, four
// waves per CU -- the greedy loop is what the pass costs, and it wants every lane busy); without, a third of that (13 KiB, twelve
// waves per CU: the pass is a stream, and waves in flight are what hide HBM's latency)
constexpr int kViewCapPlaced = 5120, kViewCapPlain = 2048;
constexpr int kViewSlack = 6 * 64 + 16;     // slots beyond the rows: six-row views pad every bucket to whole groups
constexpr int kViewRun = 64;                // buckets per run: a lane each
constexpr int kColourMax5 = 128, kColourMax6 = 96;  // buckets of more rows keep the order they come in (as in round 4)
inline size_t view_lds_bytes(int cap, bool place) { return (size_t)(cap + 8) * 4 + (size_t)(cap + kViewSlack) * 2 + (place ? 4 * 32 * 64 : 0); }

// row i of group V as W = B | annot << 16   (B = (start mod 2^10) << 6 | min(overlap, 63): 16 bits; annot: 9 bits)
template <int I>
__device__ __forceinline__ uint32_t group_row(const uint4 &V) {
    const uint32_t hi = V.w >> 16;  // (bit i: the ninth annot bit of row i)
    if constexpr (I == 0) return (V.x & 0xFFFFu) | ((V.x >> 24) << 16) | ((hi & 1u) << 24);
    if constexpr (I == 1) return (V.y & 0xFFFFu) | ((V.y >> 24) << 16) | (((hi >> 1) & 1u) << 24);
    if constexpr (I == 2) return (V.z & 0xFFFFu) | ((V.z >> 24) << 16) | (((hi >> 2) & 1u) << 24);
    if constexpr (I == 3) return (V.w & 0xFFFFu) | ((V.w >> 24) << 16) | (((hi >> 3) & 1u) << 24);
    return ((V.x >> 16) & 0xFFu) | (((V.y >> 16) & 0xFFu) << 8) | (((V.z >> 16) & 0xFFu) << 16) | (((hi >> 4) & 1u) << 24);
}

// the keep bits of a group's five rows: overlap < cap, row number < rows
__device__ __forceinline__ uint32_t group_keep(const uint4 &V, uint64_t g, uint64_t rows, uint32_t cap) {
    uint32_t m = ((V.x & 63u) < cap ? 1u : 0u) | ((V.y & 63u) < cap ? 2u : 0u) | ((V.z & 63u) < cap ? 4u : 0u) |
                 ((V.w & 63u) < cap ? 8u : 0u) | (((V.x >> 16) & 63u) < cap ? 16u : 0u);
    const uint64_t r = 5 * g;
    if (r + 5 > rows) m &= r >= rows ? 0u : (1u << (uint32_t)(rows - r)) - 1u;
    return m;
}

__global__ __launch_bounds__(256) void view_count_kernel(const uint4 *__restrict__ p3, uint64_t rows, uint32_t cap,
                                                         uint8_t *__restrict__ keep8, uint32_t *__restrict__ count) {
    const uint64_t groups = (rows + 4) / 5, chunks = (groups + 63) >> 6;
    const int lane = threadIdx.x & 63;
    for (uint64_t chunk = blockIdx.x * 4ull + (threadIdx.x >> 6); chunk < chunks; chunk += gridDim.x * 4ull) {
        const uint64_t g = (chunk << 6) + (uint64_t)lane;
        uint32_t mask = 0;
        if (g < groups) mask = group_keep(p3[g], g, rows, cap);
        keep8[g] = (uint8_t)mask;  // (keep8 holds chunks * 64 bytes)
        uint32_t c = (uint32_t)__popc(mask);
        for (int off = 32; off; off >>= 1) c += (uint32_t)__shfl_xor((int)c, off, 64);
        if (lane == 0) count[chunk] = c;
    }
}

// kept rows among the first r source rows (keep8: a byte per group; local / blockpre: the scan of the kept rows per 64 groups)
__device__ __forceinline__ uint64_t view_kept_before(uint64_t r, uint64_t rows, uint64_t total, const uint8_t *keep8,
                                                     const uint32_t *local, const uint64_t *blockpre) {
    if (r >= rows) return total;
    const uint64_t g = r / 5, chunk = g >> 6;
    const uint32_t gl = (uint32_t)(g & 63), i = (uint32_t)(r - 5 * g);
    uint64_t n = blockpre[chunk >> 10] + local[chunk];
    const uint64_t *p = reinterpret_cast<const uint64_t *>(keep8 + (chunk << 6));
    for (uint32_t j = 0; j < (gl >> 3); ++j) n += (uint64_t)__popcll(p[j]);
    const uint32_t rem = gl & 7;
    const uint64_t last = p[gl >> 3];
    n += (uint64_t)__popcll(last & ((1ull << (8 * rem)) - 1ull));
    n += (uint64_t)__popc((uint32_t)(last >> (8 * rem)) & ((1u << i) - 1u));
    return n;
}

// boffv[b] = kept rows among the first boff[b] source rows; the last entry is pinned to the total
__global__ void view_table_kernel(const int64_t *__restrict__ boff, uint64_t nb, uint64_t rows, const uint8_t *__restrict__ keep8,
                                  const uint32_t *__restrict__ local, const uint64_t *__restrict__ blockpre, uint64_t nblk,
                                  int64_t *__restrict__ boffv) {
    const uint64_t b = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (b >= nb) return;
    const uint64_t total = blockpre[nblk];
    boffv[b] = b == nb - 1 ? (int64_t)total : (int64_t)view_kept_before((uint64_t)boff[b], rows, total, keep8, local, blockpre);
}

// groups of P rows every bucket of the view needs: count[b] = ceil(rows of bucket b / P)
__global__ void view_group_counts_kernel(const int64_t *__restrict__ boffv, int64_t nbuckets, uint32_t *__restrict__ count, int rpg) {
    const int64_t b = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (b < nbuckets) count[b] = (uint32_t)((boffv[b + 1] - boffv[b] + rpg - 1) / rpg);
}

// P = 5: the groups two runs share (a run's first kept row sits inside a group): zeroed before view_build_kernel or-s into them
__global__ void view_zero_edges_kernel(const int64_t *__restrict__ boffv, int64_t nbuckets, int run_buckets, uint4 *__restrict__ out) {
    const int64_t run = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const int64_t nruns = (nbuckets + run_buckets - 1) / run_buckets;
    if (run > nruns) return;
    const int64_t b = run * run_buckets < nbuckets ? run * run_buckets : nbuckets;
    const int64_t v = boffv[b];
    if (v % 5) out[v / 5] = make_uint4(0, 0, 0, 0);
}

struct ViewArgs {
    const uint4 *src;        // the dense rows the view is a view of
    const int64_t *boff;     // ... and their bucket table (nbuckets + 1 entries)
    const int64_t *boffv;    // kept rows before every bucket (nbuckets + 1 entries; the view's own table when P = 5)
    const uint32_t *glocal;  // P = 6: groups before every bucket = gblock[b >> 10] + glocal[b]
    const uint64_t *gblock;
    int64_t nbuckets;
    uint64_t rows;           // source rows
    uint4 *out;              // the view's groups
    int64_t *boff6;          // P = 6: the view's bucket table in row numbers: 6 x groups before the bucket (nbuckets + 1 entries)
    uint32_t cap;            // a row stays when its overlap is below cap
    int km1;                 // the k - 1 whose level arrays the places are chosen for (the class's cap); 0: rows keep their order
    int run_buckets;         // buckets per run (<= kViewRun)
    int stage_rows;          // kept rows the LDS stage holds (kViewCapPlaced / kViewCapPlain)
    const uint8_t *dead8;    // P = 6 with places: bit i of byte g: source row 5 g + i is contained (view_live_kernel); NULL: none is
    unsigned long long *dead_groups;  // ... groups flagged kDeadGroup (counted)
};

// A kept row b = (s, ov, order) covers [s + ov - (k - 1), s) at every k.  A kept row a of strictly LOWER order with s_a >= s_b and
// s_a + ov_a <= s_b + ov_b covers all of it at every k (k moves both left ends alike), so b never decides a minimum: b is DEAD.
// (Equal orders: both stay.)  a starts within ov_b < 32 positions of b: in b's bucket or the next (bshift 5: six-row views only).
// W (group_row) carries the verdict in bit 25 through the stage; a group of six slots that holds no live row has kDeadGroup set in
// its first dword (a bit group_rows6 does not decode): the sweep skips it (memo_sweep_cons3t.hip: LIVE).
constexpr uint32_t kDeadRow = 1u << 25;
constexpr uint32_t kDeadGroup = 1u << 20;

__device__ __forceinline__ uint32_t lanes_below(unsigned long long ballot) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
}

// one wave's LDS (dynamic): the kept rows of a piece in source order, slot -> row, colour masks per bank
struct ViewLds {
    uint32_t cap;     // rows the stage holds (ViewArgs::stage_rows)
    uint32_t *stage;  // [cap + 8]: W of the kept rows; the last 8: rows carried from the piece before (and the slot nobody reads)
    uint16_t *inv;    // [cap + kViewSlack]: which staged row a slot of the output holds
    uint8_t *am1;     // [32][64]: colours that hold a row whose FIRST block falls on bank a (a column per lane: its bucket's)
    uint8_t *am2;     // ... two rows or more
    uint8_t *bm1;     // the same for the second block
    uint8_t *bm2;
};

// source rows [r_lo, r_hi) -> their kept rows, in source order, at stage[at ...]; returns how many.
// U 16-byte loads per lane in flight, and the next U requested before these are used (the wave has the registers: its
// occupancy is set by its LDS, so nothing else hides HBM's latency).
__device__ __forceinline__ uint32_t view_load_compact(const ViewArgs &a, const ViewLds &L, uint64_t r_lo, uint64_t r_hi, uint32_t at,
                                                      int lane) {
    const uint64_t g_lo = r_lo / 5, g_hi = (r_hi + 4) / 5;
    constexpr int U = 8;
    uint32_t n = at;
    uint4 V[U], W[U];
    auto request = [&](uint4 (&R)[U], uint64_t g0) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t g = g0 + (uint64_t)(64 * u + lane);
            R[u] = g < g_hi ? a.src[g] : make_uint4(63u, 63u, 63u, 63u);
        }
    };
    auto compact = [&](const uint4 (&R)[U], uint64_t g0) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t g = g0 + (uint64_t)(64 * u + lane);
            if (g0 + (uint64_t)(64 * u) >= g_hi) break;  // (wave-uniform)
            uint32_t m = g < g_hi ? group_keep(R[u], g, a.rows, a.cap) : 0u;
            const uint32_t dm = (a.dead8 && g < g_hi) ? (uint32_t)a.dead8[g] << 25 : 0u;  // (bit 25 + i: row i is dead)
            const uint64_t r = 5 * g;  // rows of the group outside [r_lo, r_hi): the first and the last group of the range
            if (r < r_lo) m &= ~((1u << (uint32_t)(r_lo - r)) - 1u);
            if (r + 5 > r_hi) m &= r >= r_hi ? 0u : (1u << (uint32_t)(r_hi - r)) - 1u;
            const unsigned long long b0 = __ballot(m & 1u), b1 = __ballot(m & 2u), b2 = __ballot(m & 4u), b3 = __ballot(m & 8u),
                                     b4 = __ballot(m & 16u);
            uint32_t idx = n + lanes_below(b0) + lanes_below(b1) + lanes_below(b2) + lanes_below(b3) + lanes_below(b4);
            // (no branches: a row that goes is stored to a slot nobody reads -- plain stores of many lanes to one address cost one)
            const uint32_t kNowhere = L.cap + 7u;
            L.stage[(m & 1u) ? idx : kNowhere] = group_row<0>(R[u]) | ((dm >> 0) & kDeadRow);
            idx += m & 1u;
            L.stage[(m & 2u) ? idx : kNowhere] = group_row<1>(R[u]) | ((dm >> 1) & kDeadRow);
            idx += (m >> 1) & 1u;
            L.stage[(m & 4u) ? idx : kNowhere] = group_row<2>(R[u]) | ((dm >> 2) & kDeadRow);
            idx += (m >> 2) & 1u;
            L.stage[(m & 8u) ? idx : kNowhere] = group_row<3>(R[u]) | ((dm >> 3) & kDeadRow);
            idx += (m >> 3) & 1u;
            L.stage[(m & 16u) ? idx : kNowhere] = group_row<4>(R[u]) | ((dm >> 4) & kDeadRow);
            n += (uint32_t)(__popcll(b0) + __popcll(b1) + __popcll(b2) + __popcll(b3) + __popcll(b4));
        }
    };
    request(V, g_lo);
    for (uint64_t g0 = g_lo; g0 < g_hi; g0 += 2 * 64 * U) {
        if (g0 + 64 * U < g_hi) request(W, g0 + 64 * U);
        compact(V, g0);
        if (g0 + 64 * U >= g_hi) break;
        if (g0 + 2 * 64 * U < g_hi) request(V, g0 + 2 * 64 * U);
        compact(W, g0 + 64 * U);
    }
    return n - at;
}

// W (group_row) -> the fields of a five-row group / of a six-row group
__device__ __forceinline__ uint4 pack_five(const uint32_t (&w)[5]) {
    uint32_t hi = 0;
#pragma unroll
    for (int i = 0; i < 5; ++i) hi |= ((w[i] >> 24) & 1u) << i;
    const uint32_t b4 = w[4] & 0xFFFFu;
    return make_uint4((w[0] & 0xFFFFu) | ((b4 & 0xFFu) << 16) | (((w[0] >> 16) & 0xFFu) << 24),
                      (w[1] & 0xFFFFu) | ((b4 >> 8) << 16) | (((w[1] >> 16) & 0xFFu) << 24),
                      (w[2] & 0xFFFFu) | (((w[4] >> 16) & 0xFFu) << 16) | (((w[2] >> 16) & 0xFFu) << 24),
                      (w[3] & 0xFFFFu) | (hi << 16) | (((w[3] >> 16) & 0xFFu) << 24));
}

// (layout: memo_interleave.hip history / memo_sweep_dense.h: group_rows6)   lo = start mod 32 | overlap << 5
__device__ __forceinline__ uint4 pack_six(const uint32_t (&w)[6]) {
    uint32_t lo[6], an[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const uint32_t ov = w[i] & 63u;
        lo[i] = ((w[i] >> 6) & 31u) | ((ov > 31u ? 31u : ov) << 5);
        an[i] = (w[i] >> 16) & 0xFFu;
    }
    const uint32_t bucket5 = (w[0] >> 11) & 31u;  // (start mod 2^10) >> 5: every row of a group lies in the group's bucket
    return make_uint4(lo[0] | (lo[4] << 10) | (an[0] << 24), lo[1] | (an[4] << 10) | (an[1] << 24),
                      lo[2] | (an[5] << 10) | (bucket5 << 18) | (an[2] << 24), lo[3] | (lo[5] << 10) | (an[3] << 24));
}

// The slots inv[0 .. ns) as groups of P from group `gout` on: every whole group with one 16-byte store; P = 5 only: the rows
// before slot `from` of the first group belong to the run before this one, and with `tail` the last, partial group goes out
// too -- both with atomicOr into groups that were zeroed (view_zero_edges_kernel).  Returns the whole groups.
template <int P>
__device__ __forceinline__ uint32_t view_emit(const ViewArgs &a, const ViewLds &L, uint64_t gout, uint32_t ns, uint32_t from, bool tail,
                                              int lane) {
    const uint32_t whole = ns / P, all = whole + ((tail && ns % P) ? 1u : 0u);
    uint32_t flagged = 0;
    for (uint32_t t = (uint32_t)lane; t < all; t += 64) {
        const uint32_t lo = t == 0 ? from : 0u, hi = ns - P * t < (uint32_t)P ? ns - P * t : (uint32_t)P;
        if constexpr (P == 6) {
            uint32_t w[6];
#pragma unroll
            for (int i = 0; i < 6; ++i) w[i] = L.stage[L.inv[6 * t + i]];
            uint4 g = pack_six(w);
            if (a.dead8 && (w[0] & w[1] & w[2] & w[3] & w[4] & w[5] & kDeadRow)) {
                g.x |= kDeadGroup;
                ++flagged;
            }
            a.out[gout + t] = g;
        } else {
            uint32_t w[5];
#pragma unroll
            for (int i = 0; i < 5; ++i) w[i] = ((uint32_t)i >= lo && (uint32_t)i < hi) ? L.stage[L.inv[5 * t + i]] : 0u;
            const uint4 g = pack_five(w);
            if (lo == 0 && hi == 5) {
                a.out[gout + t] = g;
            } else {  // (fields of rows that are not this run's are zero: or-ing leaves the neighbour's alone)
                uint32_t *p = reinterpret_cast<uint32_t *>(a.out + gout + t);
                if (g.x) atomicOr(p + 0, g.x);
                if (g.y) atomicOr(p + 1, g.y);
                if (g.z) atomicOr(p + 2, g.z);
                if (g.w) atomicOr(p + 3, g.w);
            }
        }
    }
    if (P == 6 && a.dead8) {  // (every lane of the wave is here)
        for (int off = 32; off; off >>= 1) flagged += (uint32_t)__shfl_xor((int)flagged, off, 64);
        if (lane == 0 && flagged) atomicAdd(a.dead_groups, (unsigned long long)flagged);
    }
    return whole;
}

// lane's bucket: rows stage[off .. off + n) -> inv[bslot + place]: the place of every row among the bucket's slots.
// P = 5: slot q of the bucket is the view's row vb + q, its place in its group (vb + q) mod 5; P = 6: 6 * ng slots, place q mod 6.
// The lanes of a wave run this together, a bucket each.  nl: the bucket's first nl rows are its live ones (view_live_kernel; nl = n
// when there is no verdict) -- P = 6 places them inside the bucket's first ceil(nl / 6) groups, then the dead rows; lastp: the stage
// slot of the bucket's last row in source order (what the places no row took hold a copy of, as in the view without places).
//
// The places (round 4's one-lane-per-bucket kernel, NOTEBOOK.md; the cost model: profiles/r04_lds_atomics.txt, tools/view_order_model.py).  The sweep gives
// a lane one group, and a wave's i-th row instruction visits place i of 64 consecutive groups: a half-wave's 32 atomics of one
// instruction are place i of 32 groups.  A row's two ds_min go to cell A = start - (k - 1) + overlap (first block) and B = start -
// 2^level (second block); the 32 atomics cost max(2, lanes on the fullest bank) cycles.  So the rows of a bucket are split into P
// COLOURS (= places) with, as nearly as a greedy pass gets it, no three rows of one colour on one bank of A nor of B: each row, in
// the order the rows come, takes the colour of least penalty -- 4 for a second row on its A bank, 16 more for a third, 5 / 16 for B --
// then the emptier colour, then the lower one.  Round 4 kept a bank mask per colour and priced every colour for every row, and
// sorted the rows by their A bank first (175 instructions per row and three passes; one lane per bucket straight from HBM: 4 ms
// for config 3).  Here: colour MASKS per bank, in LDS bytes (a column per lane), from which the eight penalty classes are a few
// ANDs; no sort -- by the model the sort is worth 0.23 of 7.65 -> 5.5 cycles per row instruction and half-wave (5.76 without it),
// 0.5 % of a sweep, and it was a third of this pass's instructions and a quarter of its LDS.
template <int P>
__device__ __forceinline__ void view_place_bucket(const ViewArgs &a, const ViewLds &L, uint32_t off, uint32_t n, uint32_t bslot,
                                                  uint32_t vb_mod5, int lane, uint32_t nl, uint32_t lastp) {
    const uint32_t ng = (n + P - 1) / P;
    const bool colour = a.km1 > 0 && n >= 6 && n <= (uint32_t)(P == 6 ? kColourMax6 : kColourMax5);
    if (!colour) {  // as they come (P = 6: the places the bucket leaves empty hold a copy of its last row)
        if (n)
            for (uint32_t q = 0; q < (P == 6 ? 6 * ng : n); ++q) L.inv[bslot + q] = (uint16_t)(q < n ? off + q : lastp);
    }
    if (!__ballot(colour)) return;
    const uint32_t km1 = (uint32_t)a.km1;
    // rooms: how many slots of every place the bucket has (packed: 5 bits per place); skips: its first slot of every place
    uint32_t rooms = 0, skips = 0, notfull = 0;
#pragma unroll
    for (int c = 0; c < P; ++c) {
        uint32_t skip = (uint32_t)c, room = ng;
        if constexpr (P == 5) {
            skip = ((uint32_t)c + 5u - vb_mod5) % 5u;
            room = n > skip ? (n - skip + 4u) / 5u : 0u;
        }
        rooms |= room << (5 * c);
        skips |= skip << (3 * c);
        notfull |= room ? 1u << c : 0u;
    }
    const uint32_t nc = colour ? n : 0u;  // rows this lane places
    // P = 6: the live rows first, into the first gl groups (every colour's room gl), then the rest (room ng)
    const uint32_t gl = (nl + 5u) / 6u;
    uint32_t lim = ng;
    if (P == 6 && nl < n && nl) {
        lim = gl;
        notfull = 0x3Fu;
    }
    uint8_t *a1p = L.am1 + lane, *a2p = L.am2 + lane, *b1p = L.bm1 + lane, *b2p = L.bm2 + lane;
    uint32_t loads = 0;
    uint32_t w_next = nc ? L.stage[off] : 0u;
    for (uint32_t j = 0; __ballot(j < nc); ++j) {
        const uint32_t w = w_next;
        const bool on = j < nc;
        w_next = j + 1 < nc ? L.stage[off + j + 1] : 0u;  // (a row ahead: the read is in flight under this row's arithmetic)
        if (!on) continue;
        if (P == 6 && j == nl && lim != ng) {  // (the dead rows: every colour's room is ng again)
            lim = ng;
            notfull = 0;
#pragma unroll
            for (int c = 0; c < P; ++c) notfull |= ((loads >> (5 * c)) & 31u) < ng ? 1u << c : 0u;
        }
        const uint32_t ov = w & 63u, s = (w >> 6) & 1023u;
        const uint32_t nn = km1 - ov;  // (>= 1: the view holds the rows whose overlap is below the cap)
        const uint32_t ra = (s - nn) & 31u;                                           // first block: cell start - (k - 1) + overlap
        const uint32_t rb = (s - (1u << (31 - __clz((int)(nn ? nn : 1u))))) & 31u;  // second block: cell start - 2^level
        const uint32_t a1 = a1p[64u * ra], a2 = a2p[64u * ra], b1 = b1p[64u * rb], b2 = b2p[64u * rb];
        // the colours by rising penalty: 0 | 4 | 5 | 9 | 20 | 21 | 25 | 41
        const uint32_t x0 = notfull & ~a1, x1 = notfull & a1 & ~a2, x2 = notfull & a2;
        const uint32_t y0 = ~b1, y1 = b1 & ~b2, y2 = b2;
        uint32_t m = x0 & y0;
        if (!m) m = x1 & y0;
        if (!m) m = x0 & y1;
        if (!m) m = x1 & y1;
        if (!m) m = x2 & y0;
        if (!m) m = x0 & y2;
        if (!m) m = (x2 & y1) | (x1 & y2);
        if (!m) m = notfull;
        uint32_t best = 0xFFFFFFFFu;
#pragma unroll
        for (int c = 0; c < P; ++c) {
            const uint32_t key = (((loads >> (5 * c)) & 31u) << 3) | (uint32_t)c | (((m >> c) & 1u) ? 0u : 0x100u);
            best = key < best ? key : best;
        }
        const uint32_t c = best & 7u, ld = (best >> 3) & 31u;
        const uint32_t slot = P == 6 ? 6u * ld + c : ((skips >> (3 * c)) & 7u) + 5u * ld;
        L.inv[bslot + slot] = (uint16_t)(off + j);
        const uint32_t bit = 1u << c;
        a2p[64u * ra] = (uint8_t)(a2 | (a1 & bit));
        a1p[64u * ra] = (uint8_t)(a1 | bit);
        b2p[64u * rb] = (uint8_t)(b2 | (b1 & bit));
        b1p[64u * rb] = (uint8_t)(b1 | bit);
        loads += 1u << (5 * c);
        if (ld + 1u == (P == 6 ? lim : ((rooms >> (5 * c)) & 31u))) notfull &= ~bit;
    }
    if constexpr (P == 6) {  // the places no row took (6 ng - n of them, five at most): a copy of the bucket's last row
        if (nc)
            for (int c = 0; c < 6; ++c)
                for (uint32_t g = (loads >> (5 * c)) & 31u; g < ng; ++g) L.inv[bslot + 6u * g + (uint32_t)c] = (uint16_t)lastp;
    }
}

// source row r of the dense rows as W (group_row)
__device__ __forceinline__ uint32_t source_row(const uint4 *__restrict__ src, uint64_t r) {
    const uint4 V = src[r / 5];
    switch ((uint32_t)(r % 5)) {
        case 0: return group_row<0>(V);
        case 1: return group_row<1>(V);
        case 2: return group_row<2>(V);
        case 3: return group_row<3>(V);
    }
    return group_row<4>(V);
}

// The dead kept rows (ViewArgs::dead8; bshift 5) -- a wave per bucket b: M[t][j] = the least order of the kept rows of buckets b and
// b + 1 that start at position t of the two (0 .. 63) with overlap <= j, then a kept row (s, ov, order) of b is dead iff
// min over d = 0 .. ov of M[s + d][ov - d] < order.  dead: a byte per source group (zeroed), or-ed into as 32-bit words.
__global__ __launch_bounds__(64) void view_live_kernel(const uint4 *__restrict__ src, const int64_t *__restrict__ boff, int64_t nbuckets,
                                                       uint32_t cap, uint32_t *__restrict__ dead) {
    __shared__ uint32_t M[64 * 33];  // (33: a lane's row of the prefix pass on a bank of its own)
    const int lane = threadIdx.x;
    for (int64_t b = blockIdx.x; b < nbuckets; b += gridDim.x) {
        const uint64_t r0 = (uint64_t)boff[b], r1 = (uint64_t)boff[b + 1], r2 = b + 1 < nbuckets ? (uint64_t)boff[b + 2] : r1;
        for (int i = lane; i < 64 * 33; i += 64) M[i] = 0xFFFFFFFFu;
        __syncthreads();
        for (uint64_t r = r0 + (uint64_t)lane; r < r2; r += 64) {
            const uint32_t w = source_row(src, r), ov = w & 63u;
            if (ov < cap) atomicMin(&M[((r < r1 ? 0u : 32u) + ((w >> 6) & 31u)) * 33u + ov], (w >> 16) & 0x1FFu);
        }
        __syncthreads();
        uint32_t m = M[lane * 33];
        for (int j = 1; j < 32; ++j) {
            const uint32_t x = M[lane * 33 + j];
            m = x < m ? x : m;
            M[lane * 33 + j] = m;
        }
        __syncthreads();
        for (uint64_t r = r0 + (uint64_t)lane; r < r1; r += 64) {
            const uint32_t w = source_row(src, r), ov = w & 63u;
            if (ov >= cap) continue;
            const uint32_t s = (w >> 6) & 31u, order = (w >> 16) & 0x1FFu;
            uint32_t least = 0xFFFFFFFFu;
            for (uint32_t d = 0; d <= ov; ++d) {
                const uint32_t x = M[(s + d) * 33u + ov - d];
                least = x < least ? x : least;
            }
            if (least < order) {
                const uint64_t g = r / 5;
                atomicOr(dead + (g >> 2), 1u << (8u * (uint32_t)(g & 3) + (uint32_t)(r - 5 * g)));
            }
        }
        __syncthreads();
    }
}

// The copy of a placed six-row view without its dead groups (live_view_copy): every group whose kDeadGroup bit is clear, unchanged and
// in the order it comes (a group carries its bucket mod 32 and ends at a bucket boundary, so nothing is re-encoded), with a bucket table
// of its own.  count -> the scan of dense_view_build -> table + scatter.  mask: a bit per group, a word per 64 groups; count: live
// groups per 64.
__global__ __launch_bounds__(256) void live_count_kernel(const uint4 *__restrict__ groups, uint64_t ng, unsigned long long *__restrict__ mask,
                                                         uint32_t *__restrict__ count) {
    const uint64_t chunks = (ng + 63) >> 6;
    const int lane = threadIdx.x & 63;
    for (uint64_t chunk = blockIdx.x * 4ull + (threadIdx.x >> 6); chunk < chunks; chunk += gridDim.x * 4ull) {
        const uint64_t g = (chunk << 6) + (uint64_t)lane;
        const unsigned long long m = __ballot(g < ng && !(groups[g].x & kDeadGroup));
        if (lane == 0) {
            mask[chunk] = m;
            count[chunk] = (uint32_t)__popcll(m);
        }
    }
}

// live groups before group g (local / blockpre: the scan of count)
__device__ __forceinline__ uint64_t live_before(uint64_t g, const unsigned long long *mask, const uint32_t *local, const uint64_t *blockpre) {
    const uint64_t chunk = g >> 6;
    return blockpre[chunk >> 10] + local[chunk] + (uint64_t)__popcll(mask[chunk] & ((1ull << (g & 63)) - 1ull));
}

// the copy's bucket table in slots: 6 x the live groups before every bucket's first group (nb entries; the last is 6 x all of them)
__global__ void live_table_kernel(const int64_t *__restrict__ boff6, uint64_t nb, uint64_t ng, const unsigned long long *__restrict__ mask,
                                  const uint32_t *__restrict__ local, const uint64_t *__restrict__ blockpre, uint64_t nblk,
                                  int64_t *__restrict__ out) {
    const uint64_t b = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (b >= nb) return;
    const uint64_t g = (uint64_t)boff6[b] / 6;
    out[b] = (int64_t)(6 * (g >= ng ? blockpre[nblk] : live_before(g, mask, local, blockpre)));
}

// the live groups to their places in the copy (nout: groups the copy holds -- a place past it is never written)
__global__ __launch_bounds__(256) void live_scatter_kernel(const uint4 *__restrict__ groups, uint64_t ng, const unsigned long long *__restrict__ mask,
                                                           const uint32_t *__restrict__ local, const uint64_t *__restrict__ blockpre,
                                                           uint4 *__restrict__ out, uint64_t nout) {
    const uint64_t chunks = (ng + 63) >> 6;
    const int lane = threadIdx.x & 63;
    for (uint64_t chunk = blockIdx.x * 4ull + (threadIdx.x >> 6); chunk < chunks; chunk += gridDim.x * 4ull) {
        const unsigned long long m = mask[chunk];
        if (!((m >> lane) & 1ull)) continue;
        const uint64_t at = blockpre[chunk >> 10] + local[chunk] + (uint64_t)__popcll(m & ((1ull << lane) - 1ull));
        if (at < nout) out[at] = groups[(chunk << 6) + (uint64_t)lane];
    }
}

// ======================================================================================================================
// The DECIDING copy of a live copy (deciding_view_copy): the rows that win a position at ONE k - 1.
//
// A slot (start s, overlap ov, order) of a six-row view covers the n = k - 1 - ov cells [s - n, s) (n <= 0: none).  For every cell keep
// the slot of least (order, slot number) among those that cover it: the minimum over the kept slots is the minimum over all of
// them, for any window.  (Which slot a cell keeps does not change when every interval is moved alike, so the cells need not be the
// sweep's own.)  The places a bucket left empty hold a copy of its last row: slots like any other, and when such a copy wins, it is
// that row which is kept.
//   1. decide_mark_kernel: a workgroup per run of kDecideW cells [a, a + W), a = run x W.  Its slice, by tile_table_kernel's rule, is
//      the groups of the buckets a / 32 ... (a + W + k - 2) / 32: at most 32 of them, so a group's bucket -- carried mod 32 -- is known
//      from the run's first one.  W cells of LDS, all ones; every slot atomicMin-s order << 24 | slot (counted from the slice's first
//      group: it grows with the global slot number, so the winner is the same whatever the raster) into the cells it covers inside
//      the run; a cell that differs from its left neighbour's sets its winner's bit in a bitmap of one bit per slot.  A slice of
//      2^24 slots or more sets flags[0]: the pass gives up.
//   2. decide_count_kernel: winners per bucket -> groups of six; the scan of dense_view_build; decide_write_kernel: a lane per
//      bucket packs its winners, in slot order, into groups that carry the bucket and end at its boundary -- the encoding of
//      view_build_kernel<6>, the places left empty holding a copy of the bucket's last winner, no flag set -- and the copy's table.
// ======================================================================================================================
constexpr int kDecideW = 960;  // 30 buckets: with k - 1 <= 31 a run's slice spans at most 32

// slot i of a six-row group as lo | annot << 10  (lo = start mod 32 | overlap << 5; pack_six)
__device__ __forceinline__ uint32_t six_slot(const uint4 &V, uint32_t i) {
    switch (i) {
        case 0: return (V.x & 1023u) | ((V.x >> 24) << 10);
        case 1: return (V.y & 1023u) | ((V.y >> 24) << 10);
        case 2: return (V.z & 1023u) | ((V.z >> 24) << 10);
        case 3: return (V.w & 1023u) | ((V.w >> 24) << 10);
        case 4: return ((V.x >> 10) & 1023u) | (((V.y >> 10) & 255u) << 10);
    }
    return ((V.w >> 10) & 1023u) | (((V.z >> 10) & 255u) << 10);
}

__device__ __forceinline__ uint4 pack_six_slots(const uint32_t (&r)[6], uint32_t bucket5) {
    uint32_t lo[6], an[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        lo[i] = r[i] & 1023u;
        an[i] = (r[i] >> 10) & 255u;
    }
    return make_uint4(lo[0] | (lo[4] << 10) | (an[0] << 24), lo[1] | (an[4] << 10) | (an[1] << 24),
                      lo[2] | (an[5] << 10) | (bucket5 << 18) | (an[2] << 24), lo[3] | (lo[5] << 10) | (an[3] << 24));
}

// the slice of the run that begins at cell a: the groups [*g0, *g1) of the buckets that hold a start in [a, a + W + km1)
__device__ __forceinline__ void decide_slice(const int64_t *__restrict__ boff, int64_t nb, int64_t bbase, int64_t a, int km1, uint64_t *g0,
                                             uint64_t *g1) {
    const int64_t last = nb - 1;
    int64_t b0 = (a >> 5) - bbase, b1 = ((a + kDecideW + km1 + 31) >> 5) - bbase;
    b0 = b0 < 0 ? 0 : (b0 > last ? last : b0);
    b1 = b1 < 0 ? 0 : (b1 > last ? last : b1);
    *g0 = (uint64_t)boff[b0] / 6;
    *g1 = (uint64_t)boff[b1] / 6;
}

__global__ __launch_bounds__(256) void decide_mark_kernel(const uint4 *__restrict__ groups, const int64_t *__restrict__ boff, int64_t nb,
                                                          int64_t bbase, int64_t run_lo, int km1, uint32_t *__restrict__ bitmap,
                                                          uint32_t *__restrict__ flags) {
    __shared__ uint32_t cell[kDecideW];
    const int64_t a = (run_lo + (int64_t)blockIdx.x) * kDecideW;
    uint64_t g0, g1;
    decide_slice(boff, nb, bbase, a, km1, &g0, &g1);
    if (g1 <= g0) return;  // (the whole workgroup)
    if (6 * (g1 - g0) >= 0xFFFFFFull) {
        if (threadIdx.x == 0) atomicOr(flags, 1u);
        return;
    }
    for (int p = threadIdx.x; p < kDecideW; p += 256) cell[p] = 0xFFFFFFFFu;
    __syncthreads();
    const uint32_t fa = (uint32_t)(a >> 5) & 31u;  // the run's first bucket mod 32
    for (uint64_t g = g0 + threadIdx.x; g < g1; g += 256) {
        const uint4 V = groups[g];
        const int base = (int)(((((V.z >> 18) & 31u) - fa) & 31u) * 32u);  // the cell of the group's bucket, from a
        const uint32_t slot0 = (uint32_t)(6 * (g - g0));
#pragma unroll
        for (uint32_t i = 0; i < 6; ++i) {
            const uint32_t r = six_slot(V, i);
            const int n = km1 - (int)((r >> 5) & 31u), s = base + (int)(r & 31u);
            const uint32_t key = ((r >> 10) << 24) | (slot0 + i);
            const int hi = s < kDecideW ? s : kDecideW;
            for (int p = s - n < 0 ? 0 : s - n; p < hi; ++p) atomicMin(&cell[p], key);
        }
    }
    __syncthreads();
    for (int p = threadIdx.x; p < kDecideW; p += 256) {
        const uint32_t c = cell[p];
        if (c == 0xFFFFFFFFu || (p && cell[p - 1] == c)) continue;
        const uint64_t slot = 6 * g0 + (uint64_t)(c & 0xFFFFFFu);
        atomicOr(bitmap + (slot >> 5), 1u << (uint32_t)(slot & 31));
    }
}

// the winners among the slots [r0, r1): f(slot) for each, in slot order
template <typename F>
__device__ __forceinline__ void decide_each_winner(const uint32_t *__restrict__ bitmap, uint64_t r0, uint64_t r1, F f) {
    if (r1 <= r0) return;
    const uint64_t w0 = r0 >> 5, w1 = (r1 - 1) >> 5;
    for (uint64_t w = w0; w <= w1; ++w) {
        uint32_t m = bitmap[w];
        if (w == w0) m &= 0xFFFFFFFFu << (uint32_t)(r0 & 31);
        if (w == w1 && (r1 & 31)) m &= (1u << (uint32_t)(r1 & 31)) - 1u;
        while (m) {
            f((w << 5) + (uint64_t)(__ffs((int)m) - 1));
            m &= m - 1u;
        }
    }
}

__global__ void decide_count_kernel(const int64_t *__restrict__ boff, int64_t nbuckets, const uint32_t *__restrict__ bitmap,
                                    uint32_t *__restrict__ gcount, unsigned long long *__restrict__ winners) {
    const int64_t b = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (b >= nbuckets) return;
    uint32_t c = 0;
    decide_each_winner(bitmap, (uint64_t)boff[b], (uint64_t)boff[b + 1], [&](uint64_t) { ++c; });
    gcount[b] = (c + 5u) / 6u;
    if (c) atomicAdd(winners, (unsigned long long)c);
}

// glocal / gblock: the scan of gcount (groups of the copy before every bucket); total: all of them; out holds `total` groups
__global__ void decide_write_kernel(const uint4 *__restrict__ groups, const int64_t *__restrict__ boff, int64_t nbuckets,
                                    const uint32_t *__restrict__ bitmap, const uint32_t *__restrict__ glocal,
                                    const uint64_t *__restrict__ gblock, uint64_t total, uint4 *__restrict__ out, int64_t *__restrict__ boffd) {
    const int64_t b = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (b >= nbuckets) return;
    uint64_t gout = gblock[b >> 10] + glocal[b];
    boffd[b] = (int64_t)(6 * gout);
    if (b == nbuckets - 1) boffd[nbuckets] = (int64_t)(6 * total);
    uint32_t r[6] = {0, 0, 0, 0, 0, 0}, have = 0, bucket5 = 0;
    decide_each_winner(bitmap, (uint64_t)boff[b], (uint64_t)boff[b + 1], [&](uint64_t slot) {
        const uint4 V = groups[slot / 6];
        bucket5 = (V.z >> 18) & 31u;
        const uint32_t row = six_slot(V, (uint32_t)(slot % 6));
#pragma unroll
        for (uint32_t i = 0; i < 6; ++i)  // (the places behind it: a copy of the last winner so far)
            if (i >= have) r[i] = row;
        if (++have == 6) {
            if (gout < total) out[gout] = pack_six_slots(r, bucket5);
            ++gout;
            have = 0;
        }
    });
    if (have && gout < total) out[gout] = pack_six_slots(r, bucket5);
}

// ======================================================================================================================
// The RUN copy of a deciding copy (run_view_copy): the minimum of ONE k - 1 itself, resolved once and run-coded.
//
// The copy's buckets are the pivot buckets b0 ... b0 + buckets - 1 (b0: one below the index's first -- a row reaches back k - 1 <= 31
// positions; whole groups of kRunGroup).  Per bucket a start mask -- bit i: result[i] differs from result[i - 1]; bit 0 always -- and the
// byte offset of its first value; per run a byte, the least order that covers it, 255: none.  A group's values begin at a multiple of four.
//   1. runs_mark_kernel: decide_mark_kernel's sibling, on the same slices and runs of kDecideW cells: every slot atomicMin-s its order into
//      the cells it covers, and the cells go out as a byte each into `res` (ncells bytes from position p0 = 32 b0; all 255 before).
//   2. runs_count_kernel: a lane per bucket -> the values of its group in dwords, and all the runs; the scan of dense_view_build;
//      runs_write_kernel: a lane per bucket stores its table entry and its values.  (Counting inside the mark kernel instead -- a
//      wave's ballot over 64 cells, an atomic a bucket -- was measured: the marking went from 0.38 to 1.29 ms on 10^8 positions, more
//      than the 0.59 ms of the count kernel it replaced: profiles/run_copy.txt.)
// ======================================================================================================================
__global__ __launch_bounds__(256) void runs_mark_kernel(const uint4 *__restrict__ groups, const int64_t *__restrict__ boff, int64_t nb,
                                                        int64_t bbase, int64_t run_lo, int km1, int64_t p0, int64_t ncells,
                                                        uint32_t *__restrict__ res) {
    __shared__ uint32_t cell[kDecideW];
    const int64_t a = (run_lo + (int64_t)blockIdx.x) * kDecideW;
    uint64_t g0, g1;
    decide_slice(boff, nb, bbase, a, km1, &g0, &g1);
    if (g1 <= g0) return;  // (the whole workgroup: its cells stay 255)
    for (int p = threadIdx.x; p < kDecideW; p += 256) cell[p] = 255u;
    __syncthreads();
    const uint32_t fa = (uint32_t)(a >> 5) & 31u;  // the run's first bucket mod 32
    for (uint64_t g = g0 + threadIdx.x; g < g1; g += 256) {
        const uint4 V = groups[g];
        const int base = (int)(((((V.z >> 18) & 31u) - fa) & 31u) * 32u);  // the cell of the group's bucket, from a
#pragma unroll
        for (uint32_t i = 0; i < 6; ++i) {
            const uint32_t r = six_slot(V, i);
            const int n = km1 - (int)((r >> 5) & 31u), s = base + (int)(r & 31u);
            const int hi = s < kDecideW ? s : kDecideW;
            for (int p = s - n < 0 ? 0 : s - n; p < hi; ++p) atomicMin(&cell[p], r >> 10);
        }
    }
    __syncthreads();
    // four cells a lane, one dword: a and p0 are multiples of 32, ncells of 256
    for (int q = threadIdx.x; q < kDecideW / 4; q += 256) {
        const int64_t at = a - p0 + 4 * q;
        if (at < 0 || at + 4 > ncells) continue;
        res[at >> 2] = cell[4 * q] | (cell[4 * q + 1] << 8) | (cell[4 * q + 2] << 16) | (cell[4 * q + 3] << 24);
    }
}

// the start mask of the bucket whose 32 results are the bytes of A (positions 0 .. 15) and B (16 .. 31)
__device__ __forceinline__ uint32_t runs_mask(const uint4 &A, const uint4 &B) {
    const uint32_t w[8] = {A.x, A.y, A.z, A.w, B.x, B.y, B.z, B.w};
    uint32_t m = 1u;
#pragma unroll
    for (int i = 1; i < 32; ++i) {
        const uint32_t cur = (w[i >> 2] >> (8 * (i & 3))) & 255u, prev = (w[(i - 1) >> 2] >> (8 * ((i - 1) & 3))) & 255u;
        m |= (cur != prev ? 1u : 0u) << i;
    }
    return m;
}

// (whole waves: the grid covers `buckets`, a multiple of kRunGroup, rounded up to workgroups; a lane past the end counts nothing)
__global__ __launch_bounds__(256) void runs_count_kernel(const uint4 *__restrict__ res, int64_t buckets, uint32_t *__restrict__ gcount,
                                                         unsigned long long *__restrict__ runs) {
    const int64_t b = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    uint32_t c = 0;
    if (b < buckets) c = (uint32_t)__popc(runs_mask(res[2 * b], res[2 * b + 1]));
    c += __shfl_xor(c, 1);
    c += __shfl_xor(c, 2);
    c += __shfl_xor(c, 4);
    if (b < buckets && !(b & (kRunGroup - 1))) gcount[b / kRunGroup] = (c + 3u) >> 2;
    c += __shfl_xor(c, 8);
    c += __shfl_xor(c, 16);
    c += __shfl_xor(c, 32);
    if (!(threadIdx.x & 63) && c) atomicAdd(runs, (unsigned long long)c);
}

// glocal / gblock: the scan of gcount (dwords of values before every group); tab: an entry per bucket; vals: the values' bytes (zeroed)
__global__ __launch_bounds__(256) void runs_write_kernel(const uint4 *__restrict__ res, int64_t buckets, const uint32_t *__restrict__ glocal,
                                                         const uint64_t *__restrict__ gblock, uint64_t value_bytes, uint2 *__restrict__ tab,
                                                         uint8_t *__restrict__ vals) {
    const int64_t b = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const bool in = b < buckets;
    uint4 A = make_uint4(0, 0, 0, 0), B = A;
    if (in) A = res[2 * b], B = res[2 * b + 1];
    const uint32_t m = in ? runs_mask(A, B) : 0u, c = (uint32_t)__popc(m), sub = threadIdx.x & (kRunGroup - 1);
    uint32_t upto = c;  // inclusive, over the group's buckets so far
    for (uint32_t d = 1; d < (uint32_t)kRunGroup; d <<= 1) {
        const uint32_t t = __shfl_up(upto, d);
        if (sub >= d) upto += t;
    }
    if (!in) return;
    const int64_t g = b / kRunGroup;
    uint64_t at = 4 * (gblock[g >> 10] + glocal[g]) + (upto - c);
    tab[b] = make_uint2(m, (uint32_t)at);
    const uint32_t w[8] = {A.x, A.y, A.z, A.w, B.x, B.y, B.z, B.w};
#pragma unroll
    for (int i = 0; i < 32; ++i)
        if ((m >> i) & 1u) {
            if (at < value_bytes) vals[at] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
            ++at;
        }
}

template <int P>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 2))) void view_build_kernel(const ViewArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t view_lds[];
    ViewLds L;
    L.stage = view_lds;
    L.cap = (uint32_t)a.stage_rows;
    L.inv = reinterpret_cast<uint16_t *>(L.stage + L.cap + 8);
    L.am1 = reinterpret_cast<uint8_t *>(L.inv + L.cap + kViewSlack);  // (the four mask arrays exist only when places are chosen: a.km1 > 0)
    L.am2 = L.am1 + 32 * 64;
    L.bm1 = L.am2 + 32 * 64;
    L.bm2 = L.bm1 + 32 * 64;
    const int lane = threadIdx.x;
    const int RB = a.run_buckets;
    const int64_t nruns = (a.nbuckets + RB - 1) / RB;
    for (int64_t run = blockIdx.x; run < nruns; run += gridDim.x) {
        const int64_t b0 = run * RB;
        const int nbk = (int)(a.nbuckets - b0 < RB ? a.nbuckets - b0 : RB);
        const int64_t bj = b0 + (lane < nbk ? lane : nbk);  // (lanes past the run hold its end)
        const uint64_t sb = (uint64_t)a.boff[bj], vb = (uint64_t)a.boffv[bj];
        const int64_t bn = bj < a.nbuckets ? bj + 1 : a.nbuckets;
        const uint64_t se = (uint64_t)a.boff[bn], ve = (uint64_t)a.boffv[bn];
        uint64_t gq = 0;  // P = 6: groups of the view before this lane's bucket
        if constexpr (P == 6) {
            gq = bj < a.nbuckets ? a.gblock[bj >> 10] + a.glocal[bj] : 0;
            if (lane < nbk) a.boff6[bj] = (int64_t)(6 * gq);
            if (b0 + nbk == a.nbuckets && lane == nbk - 1) a.boff6[a.nbuckets] = (int64_t)(6 * (gq + (ve - vb + 5) / 6));
        }
        const uint64_t v_run0 = (uint64_t)__shfl((long long)vb, 0, 64);
        // P = 5: slot 0 of the output staging is the view's row pbase (a multiple of 5); rows before pfrom are not this run's
        uint64_t pbase = v_run0 / 5 * 5, pfrom = v_run0;
        // P = 5: slots of the last, partial group so far: rows carried from the piece before (staged at stage[cap ...]) -- and, at
        // the head of a run, the rows of that group that belong to the run before (never read: view_emit masks them by `from`)
        uint32_t carried = P == 5 ? (uint32_t)(pfrom - pbase) : 0u;
        if (lane < 8) L.inv[lane] = (uint16_t)(L.cap + lane);  // (slots of the first group that are not this run's: never used, but read)
        __syncthreads();
        int s = 0;
        while (s < nbk) {
            const uint64_t v0 = (uint64_t)__shfl((long long)vb, s, 64);
            const unsigned long long fits = __ballot(lane >= s && lane < nbk && ve - v0 <= (uint64_t)L.cap);
            const int e = s + (int)__popcll(fits);  // (ve rises with the lane: the buckets that fit are s .. e - 1)
            if (e > s) {
                // ---- buckets s .. e - 1 whole: load, place, emit ----
                const uint64_t r_lo = (uint64_t)__shfl((long long)sb, s, 64), r_hi = (uint64_t)__shfl((long long)se, e - 1, 64);
                const uint64_t v1 = (uint64_t)__shfl((long long)ve, e - 1, 64);
                const uint32_t got = view_load_compact(a, L, r_lo, r_hi, 0, lane);
                (void)got;
                __syncthreads();
                const bool mine = lane >= s && lane < e;
                const uint32_t n = mine ? (uint32_t)(ve - vb) : 0u, off = (uint32_t)(vb - v0);
                uint64_t gbase = 0;
                uint32_t bslot;
                if constexpr (P == 6) {
                    gbase = (uint64_t)__shfl((long long)gq, s, 64);
                    bslot = (uint32_t)(6 * (gq - gbase));
                } else {
                    bslot = (uint32_t)(vb - pbase);
                }
                if (a.km1 > 0)
                    for (int i = lane; i < 4 * 32 * 64 / 4; i += 64) reinterpret_cast<uint32_t *>(L.am1)[i] = 0;  // (no colour holds a row yet)
                // the live rows of the lane's bucket to its front (swaps: a row moves only when a live row comes after a dead one --
                // the last row in source order ends at nl - 1 when live, stays at n - 1 when dead)
                uint32_t nl = n, lastp = off + (n ? n - 1 : 0);
                if (P == 6 && a.dead8 && n) {
                    const bool last_live = !(L.stage[off + n - 1] & kDeadRow);
                    nl = 0;
                    for (uint32_t j = 0; j < n; ++j) {
                        const uint32_t w = L.stage[off + j];
                        if (w & kDeadRow) continue;
                        if (j != nl) {
                            L.stage[off + j] = L.stage[off + nl];
                            L.stage[off + nl] = w;
                        }
                        ++nl;
                    }
                    lastp = off + (last_live ? nl - 1 : n - 1);
                }
                __syncthreads();
                view_place_bucket<P>(a, L, off, n, bslot, (uint32_t)(vb % 5), lane, nl, lastp);
                __syncthreads();
                if constexpr (P == 6) {
                    const uint64_t gend = (uint64_t)__shfl((long long)(gq + (ve - vb + 5) / 6), e - 1, 64);
                    view_emit<6>(a, L, gbase, (uint32_t)(6 * (gend - gbase)), 0, false, lane);
                    __syncthreads();
                } else {
                    const uint32_t ns = (uint32_t)(v1 - pbase);
                    const bool last = e == nbk;
                    const uint32_t whole = view_emit<5>(a, L, pbase / 5, ns, (uint32_t)(pfrom - pbase), last, lane);
                    __syncthreads();
                    // the rows of the last, partial group stay for the next piece of this run
                    const uint32_t left = ns - 5 * whole;
                    uint32_t w = 0;
                    if (!last && (uint32_t)lane < left) w = L.stage[L.inv[5 * whole + lane]];
                    __syncthreads();
                    if (!last && (uint32_t)lane < left) {
                        L.stage[L.cap + lane] = w;
                        L.inv[lane] = (uint16_t)(L.cap + lane);
                    }
                    pbase += 5ull * whole;
                    if (pfrom < pbase) pfrom = pbase;
                    carried = left;
                    __syncthreads();
                }
                s = e;
                continue;
            }
            // ---- bucket s alone holds more kept rows than the stage: through it in pieces, in source order ----
            const uint64_t r_lo = (uint64_t)__shfl((long long)sb, s, 64), r_hi = (uint64_t)__shfl((long long)se, s, 64);
            const uint64_t v1 = (uint64_t)__shfl((long long)ve, s, 64);
            uint64_t gcur = 0;
            if constexpr (P == 6) {
                gcur = (uint64_t)__shfl((long long)gq, s, 64);
                carried = 0;
            }
            uint64_t done = v0;  // kept rows of the bucket emitted or carried so far
            const uint64_t piece = (uint64_t)L.cap / 5 * 5;  // source rows per piece
            for (uint64_t r = r_lo; r < r_hi; r += piece) {
                const uint64_t r_end = r + piece < r_hi ? r + piece : r_hi;
                const uint32_t got = view_load_compact(a, L, r, r_end, 0, lane);
                __syncthreads();
                for (uint32_t q = (uint32_t)lane; q < got; q += 64) L.inv[carried + q] = (uint16_t)q;
                __syncthreads();
                done += got;
                const bool last_piece = r_end >= r_hi;
                uint32_t ns = carried + got, whole;
                if constexpr (P == 6) {
                    if (last_piece && ns % 6) {  // (the places the bucket leaves empty: a copy of its last row)
                        const uint32_t pad = 6 - ns % 6;
                        const uint16_t lastrow = L.inv[ns - 1];
                        __syncthreads();
                        if ((uint32_t)lane < pad) L.inv[ns + lane] = lastrow;
                        ns += pad;
                        __syncthreads();
                    }
                    whole = view_emit<6>(a, L, gcur, ns, 0, false, lane);
                    gcur += whole;
                } else {
                    const bool last = last_piece && s + 1 == nbk;
                    whole = view_emit<5>(a, L, pbase / 5, ns, (uint32_t)(pfrom - pbase), last, lane);
                    pbase += 5ull * whole;
                    if (pfrom < pbase) pfrom = pbase;
                }
                __syncthreads();
                const uint32_t left = ns - P * whole;
                uint32_t w = 0;
                if ((uint32_t)lane < left) w = L.stage[L.inv[P * whole + lane]];
                __syncthreads();
                if ((uint32_t)lane < left) {
                    L.stage[L.cap + lane] = w;
                    L.inv[lane] = (uint16_t)(L.cap + lane);
                }
                carried = left;
                __syncthreads();
            }
            (void)done;
            (void)v1;
            if constexpr (P == 6) carried = 0;
            s += 1;
        }
    }
}


}  // namespace

namespace memo {
// Device memory for what a query builds on the side (views, tile tables).  These are optimisations: when the device has no
// room for them the query runs on the rows it has (callers see kNoRoom, not an error).  memo_debug_fail_side_allocations (AB
// library) makes every such allocation fail: the test of that path.
thread_local bool g_side_alloc_fails = false;
hipError_t side_alloc(void **p, size_t bytes) {
    if (g_side_alloc_fails) return hipErrorOutOfMemory;  // (memo_debug_fail_side_allocations of the AB library)
    const hipError_t err = hipMalloc(p, bytes);
    if (err == hipErrorOutOfMemory) (void)hipGetLastError();  // (not sticky: later calls are clean)
    return err;
}

namespace {
// The scratch and output buffers of one pass: freed when the pass returns, except what it hands to its caller (release).
struct SideBuffers {
    const char *what;  // (the pass, for its error messages)
    static constexpr int kMost = 5;
    void *owned[kMost] = {};
    int n = 0;
    hipError_t err = hipSuccess;
    explicit SideBuffers(const char *pass) : what(pass) {}
    SideBuffers(const SideBuffers &) = delete;
    SideBuffers &operator=(const SideBuffers &) = delete;
    ~SideBuffers() {
        for (int i = 0; i < n; ++i) (void)hipFree(owned[i]);
    }
    template <typename T>
    SideBuffers &alloc(T **p, size_t bytes) {  // (after a failed allocation the later ones of the group are not tried)
        *p = nullptr;
        if (err == hipSuccess) err = n < kMost ? side_alloc((void **)p, bytes) : hipErrorInvalidValue;
        if (err == hipSuccess) owned[n++] = *p;
        return *this;
    }
    int status() const {  // of the allocations so far: no room is not an error (the query runs on the rows it has)
        if (err == hipErrorOutOfMemory) return kNoRoom;
        return err == hipSuccess ? MEMO_OK : failed(err);
    }
    int failed(hipError_t e) const { return fail(MEMO_EHIP, "%s: %s", what, hipGetErrorString(e)); }
    template <typename T>
    T *release(T *p) {
        for (int i = 0; i < n; ++i)
            if (owned[i] == p) owned[i] = nullptr;
        return p;
    }
};

// the offsets of the arrays a pass carves out of ONE scratch allocation (each at a multiple of 256 bytes)
struct Carve {
    uint64_t bytes = 0;
    uint64_t take(uint64_t size) {
        const uint64_t at = bytes;
        bytes += (size + 255) & ~(uint64_t)255;
        return at;
    }
};

// workgroups of a kernel whose workgroups stride over their work: as many as there is work, `most` at most
unsigned grid_up_to(uint64_t want, uint64_t most = 256 * 32) { return (unsigned)(want < most ? want : most); }

// the two-level exclusive scan of count[] (n entries) in place, queued on st: count[i] + blockpre[i >> 10] = the sum before
// entry i; blockpre[(n + 1023) >> 10] = the total
void scan_counts(hipStream_t st, uint32_t *count, uint64_t n, uint64_t *blockpre) {
    const uint64_t nblk = (n + 1023) >> 10;
    hipLaunchKernelGGL(scan_local_kernel, dim3((unsigned)nblk), dim3(256), 0, st, count, n, count, blockpre);
    hipLaunchKernelGGL(scan_blocks_kernel, dim3(1), dim3(1024), 0, st, blockpre, nblk);
}

// One host wait of a pass: the launches queued so far checked, the totals the host needs next copied to it (dev == NULL: not
// this one), the stream waited for.
struct Total {
    const void *dev;
    uint64_t *host;
};
hipError_t wait_for(hipStream_t st, std::initializer_list<Total> totals) {
    hipError_t err = hipGetLastError();
    for (const Total &t : totals)
        if (err == hipSuccess && t.dev) err = hipMemcpyAsync(t.host, t.dev, 8, hipMemcpyDeviceToHost, st);
    if (err == hipSuccess) err = hipStreamSynchronize(st);
    return err;
}
}  // namespace

// The dense rows of `src` (groups, bucket table of nb entries, row count) whose overlap is below `cap`, as a view of their own
// -- groups of rpg = 5 rows back to back with the kept-rows table, or of rpg = 6 rows that carry their bucket, with a table in
// units of (padded) rows -- or nothing (out.p3 stays NULL) when fewer than min_tenths tenths of the rows would go.
// colour_km1 > 0: the place of a row inside its group is chosen for the level arrays of k - 1 = colour_km1.  Count, scan and
// the fused pass (view_build_kernel) are queued on `st`; the call waits for them twice (the kept rows decide the allocation).
int dense_view_build(int device, const uint32_t *src_p3, const int64_t *src_boff, uint64_t rows, uint64_t nb, int cap, int min_tenths,
                     hipStream_t st, int rpg, int colour_km1, BuiltView &out) {
    out = BuiltView();
    if (!rows || rows >= ((uint64_t)1 << 38) || nb < 2) return MEMO_OK;
    DeviceGuard guard(device);
    const uint64_t groups = (rows + 4) / 5, chunks = (groups + 63) >> 6, nblk = (chunks + 1023) >> 10;
    const uint64_t nbk = nb - 1, nblk6 = (nbk + 1023) >> 10;
    const bool live = rpg == 6 && colour_km1 > 0 && cap <= 32;  // (the dead rows: views of six rows with places)
    // one allocation for everything that goes again: keep bytes, the two scans' arrays
    Carve tmp_at;
    const uint64_t o_keep = tmp_at.take(chunks * 64), o_count = tmp_at.take(chunks * 4), o_bpre = tmp_at.take((nblk + 1) * 8),
                   o_gcount = tmp_at.take(rpg == 6 ? nbk * 4 + 4 : 0), o_gblock = tmp_at.take(rpg == 6 ? (nblk6 + 1) * 8 : 0),
                   o_dead = tmp_at.take(live ? chunks * 64 : 0), o_ndead = tmp_at.take(live ? 8 : 0);
    SideBuffers side("dense view");
    char *tmp = nullptr;
    uint4 *outg = nullptr;
    int64_t *boffv = nullptr, *boff6 = nullptr;
    if (int rc = side.alloc(&tmp, tmp_at.bytes).alloc(&boffv, nb * 8).status()) return rc;
    uint8_t *keep8 = reinterpret_cast<uint8_t *>(tmp + o_keep);
    uint32_t *count = reinterpret_cast<uint32_t *>(tmp + o_count);
    uint64_t *blockpre = reinterpret_cast<uint64_t *>(tmp + o_bpre);
    uint32_t *gcount = reinterpret_cast<uint32_t *>(tmp + o_gcount);
    uint64_t *gblock = reinterpret_cast<uint64_t *>(tmp + o_gblock);
    const uint4 *p3 = reinterpret_cast<const uint4 *>(src_p3);
    hipLaunchKernelGGL(view_count_kernel, dim3(grid_up_to((chunks + 3) / 4)), dim3(256), 0, st, p3, rows, (uint32_t)cap, keep8, count);
    scan_counts(st, count, chunks, blockpre);
    hipLaunchKernelGGL(view_table_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, st, src_boff, nb, rows, keep8, count, blockpre,
                       nblk, boffv);
    uint64_t total = 0, total6 = 0;
    hipError_t err = hipGetLastError();
    if (rpg == 6 && err == hipSuccess) {  // groups per bucket -> groups before every bucket
        hipLaunchKernelGGL(view_group_counts_kernel, dim3((unsigned)((nbk + 255) / 256)), dim3(256), 0, st, boffv, (int64_t)nbk, gcount, 6);
        scan_counts(st, gcount, nbk, gblock);
    }
    if (err == hipSuccess) err = wait_for(st, {{rpg == 6 ? gblock + nblk6 : nullptr, &total6}, {blockpre + nblk, &total}});
    if (err != hipSuccess) return side.failed(err);
    if (total + rows / 10 * (uint64_t)min_tenths > rows) return MEMO_OK;  // too few would go
    const uint64_t padded = rpg == 6 ? 6 * total6 : ((total + 15) & ~(uint64_t)15) + kPadRows;
    const uint64_t ngroups = rpg == 6 ? total6 + 64 : dense_groups_for(padded), used = rpg == 6 ? total6 : total / 5;
    side.alloc(&outg, ngroups * 16);
    if (rpg == 6) side.alloc(&boff6, nb * 8);
    if (int rc = side.status()) return rc;
    err = hipMemsetAsync(outg + used, 0, (ngroups - used) * 16, st);  // (behind the rows; P = 5: the last, partial group too)
    if (err != hipSuccess) return side.failed(err);
    ViewArgs a;
    a.src = p3;
    a.boff = src_boff;
    a.boffv = boffv;
    a.glocal = gcount;
    a.gblock = gblock;
    a.nbuckets = (int64_t)nbk;
    a.rows = rows;
    a.out = outg;
    a.boff6 = boff6;
    a.cap = (uint32_t)cap;
    a.km1 = colour_km1;
    a.dead8 = nullptr;
    a.dead_groups = reinterpret_cast<unsigned long long *>(tmp + o_ndead);
    uint64_t ndead = 0;
    if (live) {
        uint8_t *dead8 = reinterpret_cast<uint8_t *>(tmp + o_dead);
        err = hipMemsetAsync(dead8, 0, o_ndead + 8 - o_dead, st);  // (the dead bits and their group count)
        if (err != hipSuccess) return side.failed(err);
        hipLaunchKernelGGL(view_live_kernel, dim3(grid_up_to(nbk)), dim3(64), 0, st, p3, src_boff, (int64_t)nbk, (uint32_t)cap,
                           reinterpret_cast<uint32_t *>(dead8));
        a.dead8 = dead8;
    }
    // buckets per run: as many as (nearly always) fit the stage whole, so that a run is one piece and every lane has a bucket
    const double per_bucket = (double)total / (double)nbk;
    a.stage_rows = colour_km1 > 0 ? kViewCapPlaced : kViewCapPlain;
    int rb = per_bucket > 1.0 ? (int)(0.85 * a.stage_rows / per_bucket) : kViewRun;
    a.run_buckets = rb > kViewRun ? kViewRun : (rb < 4 ? 4 : rb);
    const size_t lds_bytes = view_lds_bytes(a.stage_rows, colour_km1 > 0);
    const int64_t nruns = ((int64_t)nbk + a.run_buckets - 1) / a.run_buckets;
    if (rpg == 5)
        hipLaunchKernelGGL(view_zero_edges_kernel, dim3((unsigned)((nruns + 1 + 255) / 256)), dim3(256), 0, st, boffv, (int64_t)nbk,
                           a.run_buckets, outg);
    const unsigned grid = grid_up_to((uint64_t)nruns, 256 * 16 * 4);
    if (rpg == 6)
        hipLaunchKernelGGL(view_build_kernel<6>, dim3(grid), dim3(64), lds_bytes, st, a);
    else
        hipLaunchKernelGGL(view_build_kernel<5>, dim3(grid), dim3(64), lds_bytes, st, a);
    err = wait_for(st, {{live ? a.dead_groups : nullptr, &ndead}});
    if (err != hipSuccess) return side.failed(err);
    out = {reinterpret_cast<uint32_t *>(side.release(outg)), side.release(rpg == 6 ? boff6 : boffv), total, padded, ndead};
    return MEMO_OK;
}

// A placed six-row view (`flagged`: groups of ng = padded / 6, bucket table of nb entries, dead_groups of them flagged kDeadGroup) without
// its flagged groups: a new allocation of ng - dead_groups groups (+ 64 zeroed, a wave-load of slack like every view) and a new
// bucket table.  Exact: a dead row's containers are in the view, a live one among them (containment is transitive and a row's
// containers start in its bucket or the next), and the dead slots left in live groups only repeat a minimum.  Queued on `st`,
// waited for once.
int live_view_copy(int device, const BuiltView &flagged, uint64_t nb, hipStream_t st, BuiltView &out) {
    out = BuiltView();
    const uint64_t ng = flagged.padded / 6, dead_groups = flagged.dead_groups;
    if (!ng || dead_groups == 0 || dead_groups > ng || nb < 2) return MEMO_OK;
    DeviceGuard guard(device);
    const uint64_t chunks = (ng + 63) >> 6, nblk = (chunks + 1023) >> 10, nlive = ng - dead_groups;
    Carve tmp_at;
    const uint64_t o_mask = tmp_at.take(chunks * 8), o_count = tmp_at.take(chunks * 4), o_bpre = tmp_at.take((nblk + 1) * 8);
    SideBuffers side("live view");
    char *tmp = nullptr;
    uint4 *outg = nullptr;
    int64_t *boff = nullptr;
    if (int rc = side.alloc(&tmp, tmp_at.bytes).alloc(&outg, (nlive + 64) * 16).alloc(&boff, nb * 8).status()) return rc;
    unsigned long long *mask = reinterpret_cast<unsigned long long *>(tmp + o_mask);
    uint32_t *count = reinterpret_cast<uint32_t *>(tmp + o_count);
    uint64_t *blockpre = reinterpret_cast<uint64_t *>(tmp + o_bpre);
    const uint4 *src = reinterpret_cast<const uint4 *>(flagged.p3);
    const unsigned grid = grid_up_to((chunks + 3) / 4);
    hipError_t err = hipMemsetAsync(outg + nlive, 0, 64 * 16, st);
    if (err != hipSuccess) return side.failed(err);
    hipLaunchKernelGGL(live_count_kernel, dim3(grid), dim3(256), 0, st, src, ng, mask, count);
    scan_counts(st, count, chunks, blockpre);
    hipLaunchKernelGGL(live_table_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, st, flagged.boff, nb, ng, mask, count, blockpre,
                       nblk, boff);
    hipLaunchKernelGGL(live_scatter_kernel, dim3(grid), dim3(256), 0, st, src, ng, mask, count, blockpre, outg, nlive);
    uint64_t total = 0;
    err = wait_for(st, {{blockpre + nblk, &total}});
    if (err != hipSuccess) return side.failed(err);
    if (total != nlive)
        return fail(MEMO_EHIP, "live view: %llu live groups, the placing pass counted %llu", (unsigned long long)total, (unsigned long long)nlive);
    // (rows: the flagged view's -- a dead row is answered by a live one that contains it; no group of the copy is flagged)
    out = {reinterpret_cast<uint32_t *>(side.release(outg)), side.release(boff), flagged.rows, 6 * nlive, 0};
    return MEMO_OK;
}

// A live copy (`live`: padded / 6 groups, bucket table of nb entries whose first belongs to bucket bbase) down to the slots that
// decide a minimum at k - 1 = km1 (the kernels above): a new allocation of groups (+ 64 zeroed) and a new bucket table; out.rows: the
// winners, out.padded: 6 x the groups.  first_start / last_start: the index's least and largest start (the runs that can hold a row).
// Nothing built (out.p3 stays NULL, MEMO_OK): a slice too long for the 24 slot bits, more runs than a grid holds, no winner at
// all.  Queued on `st`, waited for twice (the winners decide the allocation).
int deciding_view_copy(int device, const BuiltView &live, uint64_t nb, int64_t bbase, int64_t first_start, int64_t last_start, int km1,
                       hipStream_t st, BuiltView &out) {
    out = BuiltView();
    const uint64_t ng = live.padded / 6;
    if (!ng || nb < 2 || km1 < 1 || km1 > 31 || last_start < first_start) return MEMO_OK;
    auto run_of = [](int64_t x) { return x >= 0 ? x / kDecideW : -((-x + kDecideW - 1) / kDecideW); };
    const int64_t run_lo = run_of(first_start - 64), nruns = run_of(last_start + 1) - run_lo + 1;
    if (nruns < 1 || nruns >= ((int64_t)1 << 31) - 1) return MEMO_OK;
    DeviceGuard guard(device);
    const uint64_t nbk = nb - 1, nblk6 = (nbk + 1023) >> 10, words = (live.padded >> 5) + 1;
    Carve tmp_at;
    const uint64_t o_flags = tmp_at.take(16), o_bits = tmp_at.take(words * 4), o_gcount = tmp_at.take(nbk * 4 + 4),
                   o_gblock = tmp_at.take((nblk6 + 1) * 8);
    SideBuffers side("deciding view");
    char *tmp = nullptr;
    uint4 *outg = nullptr;
    int64_t *boffd = nullptr;
    if (int rc = side.alloc(&tmp, tmp_at.bytes).status()) return rc;
    uint32_t *flags = reinterpret_cast<uint32_t *>(tmp + o_flags), *bitmap = reinterpret_cast<uint32_t *>(tmp + o_bits);
    unsigned long long *winners = reinterpret_cast<unsigned long long *>(tmp + o_flags + 8);
    uint32_t *gcount = reinterpret_cast<uint32_t *>(tmp + o_gcount);
    uint64_t *gblock = reinterpret_cast<uint64_t *>(tmp + o_gblock);
    const uint4 *src = reinterpret_cast<const uint4 *>(live.p3);
    hipError_t err = hipMemsetAsync(tmp, 0, o_gcount, st);  // (the flag, the winners' count, the bitmap)
    if (err != hipSuccess) return side.failed(err);
    hipLaunchKernelGGL(decide_mark_kernel, dim3((unsigned)nruns), dim3(256), 0, st, src, live.boff, (int64_t)nb, bbase, run_lo, km1, bitmap, flags);
    hipLaunchKernelGGL(decide_count_kernel, dim3((unsigned)((nbk + 255) / 256)), dim3(256), 0, st, live.boff, (int64_t)nbk, bitmap, gcount, winners);
    scan_counts(st, gcount, nbk, gblock);
    uint64_t total6 = 0, nwin = 0, gave_up = 0;
    err = wait_for(st, {{gblock + nblk6, &total6}, {winners, &nwin}, {flags, &gave_up}});
    if (err != hipSuccess) return side.failed(err);
    if ((gave_up & 1) || !total6) return MEMO_OK;
    if (int rc = side.alloc(&outg, (total6 + 64) * 16).alloc(&boffd, nb * 8).status()) return rc;
    err = hipMemsetAsync(outg + total6, 0, 64 * 16, st);
    if (err != hipSuccess) return side.failed(err);
    hipLaunchKernelGGL(decide_write_kernel, dim3((unsigned)((nbk + 255) / 256)), dim3(256), 0, st, src, live.boff, (int64_t)nbk, bitmap, gcount,
                       gblock, total6, outg, boffd);
    err = wait_for(st, {});
    if (err != hipSuccess) return side.failed(err);
    out = {reinterpret_cast<uint32_t *>(side.release(outg)), side.release(boffd), nwin, 6 * total6, 0};
    return MEMO_OK;
}

// A deciding copy (`dec`: padded / 6 groups, bucket table of nb entries whose first belongs to bucket bbase; exact for k - 1 = km1, orders
// <= 254) resolved into the run copy of that k - 1 (the kernels above): a new allocation of values and a table entry per bucket;
// out.rows: the runs, out.padded: the buckets, *first_bucket: the pivot bucket of the first.
// The values are followed by 512 zeroed bytes.  What needs them: a lane of the decode (memo_runs_decode.h) reads whole dwords from the
// one that holds its first byte A on, bytes [A & ~3, (A & ~3) + P + 4) for P positions a lane, A < value_bytes -- at most P bytes past
// value_bytes, 8 as memo_sweep_runs.hip is built.
// The minima are staged as a byte per position in a buffer that is freed before the call returns: the write kernel that reads them
// takes 0.04 ms on 10^8 positions, a second run of runs_mark_kernel in their place would take its 0.38 ms.  Nothing built (out.p3
// stays NULL, MEMO_OK): more runs than a grid holds, values past 2^32 bytes.  Queued on `st`, waited for twice (the runs decide the
// allocation).
int run_view_copy(int device, const BuiltView &dec, uint64_t nb, int64_t bbase, int64_t first_start, int64_t last_start, int km1,
                  hipStream_t st, BuiltView &out, int64_t *first_bucket, uint64_t *value_bytes_out) {
    out = BuiltView();
    const uint64_t ng = dec.padded / 6;
    if (!ng || nb < 2 || km1 < 1 || km1 > 31 || last_start < first_start) return MEMO_OK;
    auto run_of = [](int64_t x) { return x >= 0 ? x / kDecideW : -((-x + kDecideW - 1) / kDecideW); };
    const int64_t run_lo = run_of(first_start - 64), nruns = run_of(last_start + 1) - run_lo + 1;
    if (nruns < 1 || nruns >= ((int64_t)1 << 31) - 1) return MEMO_OK;
    const int64_t b0 = (first_start >> 5) - 1;
    const uint64_t buckets = ((uint64_t)((last_start >> 5) - b0 + 1) + kRunGroup - 1) / kRunGroup * kRunGroup, ngroups = buckets / kRunGroup;
    const uint64_t ncells = buckets * 32, nblk = (ngroups + 1023) >> 10;
    if ((buckets + 255) / 256 >= ((uint64_t)1 << 31)) return MEMO_OK;
    DeviceGuard guard(device);
    Carve tmp_at;
    const uint64_t o_runs = tmp_at.take(16), o_gcount = tmp_at.take(ngroups * 4 + 4), o_gblock = tmp_at.take((nblk + 1) * 8), o_res = tmp_at.take(ncells);
    SideBuffers side("run copy");
    char *tmp = nullptr, *vals = nullptr;
    int64_t *tab = nullptr;
    if (int rc = side.alloc(&tmp, tmp_at.bytes).status()) return rc;
    unsigned long long *runs = reinterpret_cast<unsigned long long *>(tmp + o_runs);
    uint32_t *gcount = reinterpret_cast<uint32_t *>(tmp + o_gcount);
    uint64_t *gblock = reinterpret_cast<uint64_t *>(tmp + o_gblock);
    hipError_t err = hipMemsetAsync(tmp, 0, o_res, st);
    if (err == hipSuccess) err = hipMemsetAsync(tmp + o_res, 0xFF, ncells, st);
    if (err != hipSuccess) return side.failed(err);
    const unsigned grid = (unsigned)((buckets + 255) / 256);
    hipLaunchKernelGGL(runs_mark_kernel, dim3((unsigned)nruns), dim3(256), 0, st, reinterpret_cast<const uint4 *>(dec.p3), dec.boff, (int64_t)nb,
                       bbase, run_lo, km1, b0 * 32, (int64_t)ncells, reinterpret_cast<uint32_t *>(tmp + o_res));
    hipLaunchKernelGGL(runs_count_kernel, dim3(grid), dim3(256), 0, st, reinterpret_cast<const uint4 *>(tmp + o_res), (int64_t)buckets, gcount, runs);
    scan_counts(st, gcount, ngroups, gblock);
    uint64_t dwords = 0, nrun = 0;
    err = wait_for(st, {{gblock + nblk, &dwords}, {runs, &nrun}});
    if (err != hipSuccess) return side.failed(err);
    if (!nrun || dwords >= ((uint64_t)1 << 30)) return MEMO_OK;
    const uint64_t value_bytes = dwords * 4;
    if (int rc = side.alloc(&vals, value_bytes + 512).alloc(&tab, buckets * 8).status()) return rc;
    err = hipMemsetAsync(vals, 0, value_bytes + 512, st);
    if (err != hipSuccess) return side.failed(err);
    hipLaunchKernelGGL(runs_write_kernel, dim3(grid), dim3(256), 0, st, reinterpret_cast<const uint4 *>(tmp + o_res), (int64_t)buckets, gcount, gblock,
                       value_bytes, reinterpret_cast<uint2 *>(tab), reinterpret_cast<uint8_t *>(vals));
    err = wait_for(st, {});
    if (err != hipSuccess) return side.failed(err);
    out = {reinterpret_cast<uint32_t *>(side.release(vals)), side.release(tab), nrun, buckets, 0};
    *first_bucket = b0;
    *value_bytes_out = value_bytes;
    return MEMO_OK;
}

// The same for the 4-byte WORDS (formats 4 / 12: the overlap byte sits at bit len_shift): the words whose overlap is below cap, in
// the order they come, with the kept-rows table -- keep bits, scan, scatter (the order inside the view's buckets is the caller's).
int packed_filter(int device, const uint32_t *src, const int64_t *src_boff, uint64_t rows, uint64_t nb, int cap, int min_tenths,
                  hipStream_t st, int len_shift, BuiltView &out) {
    out = BuiltView();
    if (!rows || rows >= ((uint64_t)1 << 38)) return MEMO_OK;
    DeviceGuard guard(device);
    const uint64_t n32 = (rows + 31) >> 5, nblk = (n32 + 1023) >> 10;
    const unsigned row_grid = grid_up_to((rows + 255) / 256, (uint64_t)1 << 20);
    SideBuffers side("packed view");
    uint32_t *keep = nullptr, *local = nullptr, *words = nullptr;
    uint64_t *blockpre = nullptr;
    int64_t *boffv = nullptr;
    if (int rc = side.alloc(&keep, n32 * 4 + 4).alloc(&local, n32 * 4).alloc(&blockpre, (nblk + 1) * 8).status()) return rc;
    hipLaunchKernelGGL(packed_keep_kernel, dim3(row_grid), dim3(256), 0, st, src, rows, len_shift, (uint32_t)cap, keep, local);
    scan_counts(st, local, n32, blockpre);
    uint64_t total = 0;
    hipError_t err = wait_for(st, {{blockpre + nblk, &total}});
    if (err != hipSuccess) return side.failed(err);
    if (total + rows / 10 * (uint64_t)min_tenths > rows) return MEMO_OK;  // too few would go
    const uint64_t padded = ((total + 15) & ~(uint64_t)15) + kPadRows;
    if (int rc = side.alloc(&words, padded * 4).alloc(&boffv, nb * 8).status()) return rc;
    err = hipMemsetAsync(words + total, 0, (padded - total) * 4, st);
    if (err != hipSuccess) return side.failed(err);
    hipLaunchKernelGGL(packed_scatter_kernel, dim3(row_grid), dim3(256), 0, st, src, rows, keep, local, blockpre, words);
    hipLaunchKernelGGL(dense_table_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, st, src_boff, nb, rows, total, keep, local,
                       blockpre, boffv);
    err = wait_for(st, {});
    if (err != hipSuccess) return side.failed(err);
    out = {side.release(words), side.release(boffv), total, padded, 0};
    return MEMO_OK;
}
}  // namespace memo

