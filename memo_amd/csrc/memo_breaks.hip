// memo_breaks.hip -- `memo breaks`: per genome and bin, how many maximal matches start in the bin and what the match lengths of the
// bin's positions sum to, from the finished lengths of `memo lengths` / `memo maxk` that are still in HBM.  Where a genome's match
// ends and the next begins it differs from the pivot, so the starts per bin are a variant-density track and sum / width is the mean
// match length: both k-free.  No counterpart in the reference.
//
// The cells are uint32 [planes][pitch], L of them per plane read (memo_lengths_*_dev's layout; memo_maxk_*_dev's cells are one
// plane of it).  With halo = 1 cell 0 of every plane is only the left neighbour of cell 1 and is not counted; with halo = 0 it is
// position 0 of its record.  Over the counted cells p of bin b of plane g
//     table[0][g][b] += #{ p : v[p] >= min_len and p starts a match }      memo_mems.hip's rule, literally: v[p - 1] < v[p], or
//                                                                          v[p - 1] == v[p] < cap, or cell 0 with halo = 0
//     table[1][g][b] += sum of v[p]                                        (min_len plays no part)
// uint64 [2][planes][bins], ADDED to.  The launcher turns the edges into CELL coordinates -- (edge - first, clamped to [0, L - halo])
// + halo, the first edge 0 -- so that the bins cut [0, L) into consecutive runs; with halo = 1 cell 0 lies in the first bin and adds
// nothing to it (it starts no match, and its value is taken as 0).  The kernel never sees `first`.
//
// One tile = 256 lanes x 4 cells, the four cells of one 16-byte load a lane; grid.y is the plane, grid.x runs of consecutive tiles
// (at most 1024 runs), so a tile never crosses a plane.  The cell before a lane's first comes from the lane below through a wave
// shuffle, a wave's first lane makes one extra load of v[i - 1] that is not made at i == 0 (memo_mems.hip's CellsKey::flags).  The
// next tile's load is issued before the current tile is counted.  The bins are walked as memo_features.hip's segment_kernel walks its
// segments: once per workgroup a binary search for the bin of its first cell; a 64-bit sum and a 32-bit count a lane in registers
// for the bin the workgroup is in (the head of a tile); where the bin ends a shuffle reduction in every wave and at most two 64-bit
// atomics a wave (none for a zero); the bins that begin and end inside a tile (the middle) by every lane over its own four cells,
// with its own atomics wherever the lane's bin changes; the tail into the cleared registers, which go on into the next tile.  The
// head and tail tests are the same in every lane, so the shuffles run with all lanes on, and there is no barrier at all.
//
// Conditions the code holds:
//   - no workgroup waits for another: no look-back, no flag in memory, no cooperative launch
//   - nothing is read outside [0, L) of a plane or outside edges[0 .. bins]: a load that would cross L is made cell by cell for the
//     cells before L.  The cells [L, pitch) are never read
//   - vector loads and stores and plain C++ only; no inline assembly
//   - MEMO_EINVAL before any launch: d_cells not 16-byte aligned (or NULL where cells are read); pitch not a multiple of 4 or below
//     L; L < 0 or above 2^31; planes outside [0, 2048]; bins outside [1, 2^20 + 1]; cap outside [1, 2^31 - 1]; min_len outside
//     [1, cap]; halo not 0 or 1; edges that are NULL or decrease; a slice that leaves the edges (first < edges[0], or
//     first + (L - halo) > edges[bins]); a table that is NULL or not 8-byte aligned
//   - L - halo <= 0 or planes == 0 launches nothing and leaves the table as it was
//   - integer adds only, so the table depends neither on the slicing nor on the launch shape.  The 32-bit count cannot wrap: the
//     launcher refuses what would give a workgroup more than 2^31 cells
//   - scratch: the uploaded edges ((bins + 1) x 8 bytes), owned by DevPtr; an allocation that fails is MEMO_EHIP with the bytes asked
//     for, and nothing stays allocated
#include <algorithm>
#include <vector>

#include "memo_common.h"

using namespace memo;

namespace memo {
thread_local int g_breaks_timed = 0;    // 1 = an event pair around the launch (memo_debug_breaks_times)
thread_local float g_breaks_ms = 0.f;   // ... of the last such call
}

namespace {

constexpr int kThreads = 256;
constexpr int kPer = 4;                        // uint32 cells in a 16-byte load
constexpr int kTile = kThreads * kPer;
constexpr int kMaxBins = (1 << 20) + 1;        // memo_segment_conservation_dev's: the segments of 2^19 features
constexpr int kMaxPlanes = 2048;
constexpr int kMaxGridX = 1024;                // runs of tiles a plane at most
constexpr int64_t kMaxCellsPerWg = (int64_t)1 << 31;

struct BreakArgs {
    const uint32_t *cells;  // [planes][pitch]
    int64_t L, pitch, ntiles, tiles_per_wg;
    int bins, planes, halo;
    uint32_t cap, min_len;
    const int64_t *edges;   // [bins + 1], cell coordinates, non-decreasing, edges[0] == 0 and edges[bins] == L
    uint64_t *table;        // [2][planes][bins]
};

// (memo_features.hip's three helpers, duplicated: that file's kernels stay as they are)
// the first s in [lo, hi] with edges[s + 1] > p; the caller knows that edges[hi + 1] > p
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

// the four cells at q of a plane; a cell at or past L is 0 and is not read
__device__ inline uint4 load_cells(const uint32_t *__restrict__ v, int64_t q, int64_t L) {
    if (q + kPer <= L) return *reinterpret_cast<const uint4 *>(v + q);
    uint4 w;
    w.x = q < L ? v[q] : 0u;
    w.y = q + 1 < L ? v[q + 1] : 0u;
    w.z = q + 2 < L ? v[q + 2] : 0u;
    w.w = q + 3 < L ? v[q + 3] : 0u;
    return w;
}

__global__ __launch_bounds__(kThreads) void breaks_kernel(const BreakArgs A) {
    const uint32_t *__restrict__ v = A.cells + (int64_t)blockIdx.y * A.pitch;
    uint64_t *starts = A.table + (int64_t)blockIdx.y * A.bins, *sums = starts + (int64_t)A.planes * A.bins;
    const int64_t t0 = (int64_t)blockIdx.x * A.tiles_per_wg, t1 = min(t0 + A.tiles_per_wg, A.ntiles);
    // the bin of the workgroup's first cell (there is one: edges[bins] == L)
    int b = first_above(A.edges, 0, A.bins - 1, t0 * kTile);
    int64_t bin_end = A.edges[b + 1];
    uint64_t acc_s = 0;
    uint32_t acc_c = 0;
    auto flush = [&](int bin) {  // every lane comes here
        const uint64_t s = wave_sum(acc_s), c = wave_sum((uint64_t)acc_c);
        if ((threadIdx.x & 63) == 0 && bin < A.bins) {
            if (c) add64(starts + bin, c);
            if (s) add64(sums + bin, s);
        }
        acc_s = 0, acc_c = 0;
    };
    uint4 next = load_cells(v, t0 * kTile + kPer * (int64_t)threadIdx.x, A.L);
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t ts = t * kTile, te = min(ts + kTile, A.L), q = ts + kPer * (int64_t)threadIdx.x;
        const uint4 w = next;
        if (t + 1 < t1) next = load_cells(v, q + kTile, A.L);
        // val: what a cell adds to the sum; st: 1 where it starts a match that is counted
        uint32_t val[kPer] = {w.x, w.y, w.z, w.w}, st[kPer];
        uint32_t prev = (uint32_t)__shfl_up((int)w.w, 1, 64);
        if ((threadIdx.x & 63) == 0 && q > 0 && q < A.L) prev = v[q - 1];
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            const uint32_t cur = val[j];
            const bool first = j == 0 && q == 0;  // (prev is not a cell's value at the first cell of a plane)
            const bool f = cur >= A.min_len && (first ? !A.halo : prev < cur || (prev == cur && cur < A.cap));
            st[j] = f && q + j < A.L;
            if (first && A.halo) val[j] = 0;      // the neighbour cell is not counted
            prev = cur;
        }
        auto take = [&](int64_t from, int64_t to) {  // the lane's cells at [from, to) into the registers
#pragma unroll
            for (int j = 0; j < kPer; ++j)
                if (q + j >= from && q + j < to) acc_s += val[j], acc_c += st[j];
        };
        take(ts, min(bin_end, te));                                  // the head
        if (bin_end > te || (bin_end == te && te == A.L)) continue;  // the bin goes on, or everything ends with it
        flush(b);
        // the tail's bin holds the next tile's first cell; behind the last tile there is none, and all the rest is middle
        const int bl = te < A.L ? first_above(A.edges, b + 1, A.bins - 1, te) : A.bins;
        const int64_t m = te < A.L ? A.edges[bl] : A.L;  // bin_end <= m <= te
        {   // the middle [bin_end, m): the bins b + 1 .. bl - 1, each of them inside the tile
            const int64_t from = max(q, bin_end), to = min(q + kPer, m);
            if (from < to) {
                int s = first_above(A.edges, b + 1, bl - 1, from);  // (edges[bl] == m > from)
                int64_t s_end = A.edges[s + 1];
                uint64_t own_s = 0, own_c = 0;
                auto leave = [&]() {
                    if (own_c) add64(starts + s, own_c);
                    if (own_s) add64(sums + s, own_s);
                    own_s = 0, own_c = 0;
                };
#pragma unroll
                for (int j = 0; j < kPer; ++j) {
                    const int64_t p = q + j;
                    if (p < from || p >= to) continue;
                    while (p >= s_end) {  // (p < m == edges[bl]: s stays below bl)
                        leave();
                        s_end = A.edges[++s + 1];
                    }
                    own_s += val[j], own_c += st[j];
                }
                leave();
            }
        }
        b = bl;
        if (te < A.L) {
            bin_end = A.edges[bl + 1];  // > te
            take(m, te);                // the tail
        }
    }
    flush(b);
}

}  // namespace

extern "C" {

int32_t memo_breaks_tile(void) { return kTile; }

int memo_breaks_dev(const uint32_t *d_cells, int64_t L, int64_t pitch, int32_t planes, uint32_t cap, uint32_t min_len, int32_t halo,
                    int64_t first, const int64_t *edges_host, int32_t bins, uint64_t *d_table, int32_t device, void *stream) {
    if (planes < 0 || planes > kMaxPlanes) return fail(MEMO_EINVAL, "planes must be in [0, %d] (planes = %d)", kMaxPlanes, planes);
    if (bins < 1 || bins > kMaxBins) return fail(MEMO_EINVAL, "bins must be in [1, %d] (bins = %d)", kMaxBins, bins);
    if (L < 0 || L > ((int64_t)1 << 31)) return fail(MEMO_EINVAL, "L = %lld: a plane holds at most 2^31 cells", (long long)L);
    if (pitch < L || (pitch & 3)) return fail(MEMO_EINVAL, "pitch %lld must be a multiple of 4 and at least L = %lld", (long long)pitch, (long long)L);
    if (cap < 1 || cap > 0x7fffffffu) return fail(MEMO_EINVAL, "cap %u must be in [1, 2^31 - 1]", cap);
    if (min_len < 1 || min_len > cap) return fail(MEMO_EINVAL, "min_len %u must be in [1, cap = %u]", min_len, cap);
    if (halo != 0 && halo != 1) return fail(MEMO_EINVAL, "halo %d: 0 (cell 0 is a record's first position) or 1 (cell 0 is only a neighbour)", halo);
    if (reinterpret_cast<uintptr_t>(d_cells) & 15) return fail(MEMO_EINVAL, "d_cells must be 16-byte aligned");
    if (L && planes && !d_cells) return fail(MEMO_EINVAL, "d_cells is NULL");
    if (!edges_host) return fail(MEMO_EINVAL, "edges is NULL");
    if (!d_table || (reinterpret_cast<uintptr_t>(d_table) & 7)) return fail(MEMO_EINVAL, "d_table is NULL or not 8-byte aligned");
    for (int32_t s = 0; s < bins; ++s)
        if (edges_host[s + 1] < edges_host[s])
            return fail(MEMO_EINVAL, "the bin edges decrease: edge %d is %lld, edge %d is %lld", s, (long long)edges_host[s], s + 1,
                        (long long)edges_host[s + 1]);
    const int64_t counted = std::max<int64_t>(L - halo, 0);
    // (first + counted cannot wrap where it matters: counted <= edges[bins] - first is asked instead)
    if (first < edges_host[0] || first > edges_host[bins] || counted > edges_host[bins] - first)
        return fail(MEMO_EINVAL, "the slice [%lld, %lld + %lld) leaves the bin edges [%lld, %lld)", (long long)first, (long long)first,
                    (long long)counted, (long long)edges_host[0], (long long)edges_host[bins]);
    if (!counted || !planes) return MEMO_OK;

    BreakArgs A = {};
    A.cells = d_cells;
    A.L = L;
    A.pitch = pitch;
    A.bins = bins;
    A.planes = planes;
    A.halo = halo;
    A.cap = cap;
    A.min_len = min_len;
    A.table = d_table;
    A.ntiles = (L + kTile - 1) / kTile;
    const int64_t most = std::min<int64_t>(kMaxGridX, A.ntiles);
    A.tiles_per_wg = (A.ntiles + most - 1) / most;
    if (A.tiles_per_wg * kTile > kMaxCellsPerWg) return fail(MEMO_EINVAL, "a plane of %lld cells is too long", (long long)L);
    const int gx = (int)((A.ntiles + A.tiles_per_wg - 1) / A.tiles_per_wg);
    // the edges in cell coordinates: [0, L) cut into consecutive bins, the first edge 0 (a neighbour cell adds nothing) and the last one L
    std::vector<int64_t> rel((size_t)bins + 1);
    for (int32_t s = 0; s <= bins; ++s) rel[s] = std::min<int64_t>(std::max<int64_t>(edges_host[s] - first, 0), counted) + halo;
    rel[0] = 0;

    OnDevice on(device);
    if (on.rc) return on.rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    DevPtr<int64_t> d_edges;
    if (hipError_t err = d_edges.alloc(rel.size()); err != hipSuccess)
        return fail(MEMO_EHIP, "hipMalloc(%zu bytes) for the edges of %d bins: %s", rel.size() * sizeof(int64_t), bins, hipGetErrorString(err));
    HIP_TRY(hipMemcpyAsync(d_edges, rel.data(), rel.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
    A.edges = d_edges;
    Laps laps(st, g_breaks_timed, &g_breaks_ms);
    if (int rc = laps.start()) return rc;
    hipLaunchKernelGGL(breaks_kernel, dim3((unsigned)gx, (unsigned)planes), dim3(kThreads), 0, st, A);
    HIP_TRY(hipGetLastError());
    if (int rc = laps.lap(0)) return rc;
    HIP_TRY(hipStreamSynchronize(st));  // (rel and d_edges go with this frame)
    return MEMO_OK;
}

}  // extern "C"
