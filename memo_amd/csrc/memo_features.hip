// memo_features.hip -- `memo features`: what lies between a table counted per elementary segment and a table per feature of a BED
// file.  Features overlap, nest and repeat; cut at every feature endpoint, a record falls into consecutive segments, each feature
// is a run lo .. hi of them, and with prefix sums P along the segments a feature is P[hi] - P[lo], however the features lie.  No
// counterpart in the reference.  Two entry points:
//
// memo_segment_conservation_dev: the segment table of a conservation result that is still in HBM (with -m the table is memo_tracks_dev's),
//     sums[0][s] += sum of v,  sums[1][s] += #{v >= threshold}     over the positions p of the slice with edges[s] <= p < edges[s + 1]
//   The launcher turns the edges into slice coordinates as memo_tracks_dev does (edge - first, clamped to [0, L]).  One tile = 256
//   lanes x 8 values = 2048 positions, one 16-byte load a lane; a workgroup takes a run of consecutive tiles and keeps the sum and
//   the count of the segment it is in in registers (a 64-bit sum and a 32-bit count a lane).  Once per workgroup: a binary search
//   for the segment of its first position.  A tile has three parts:
//     - the head, up to the end of the segment the workgroup is in: into the registers.  A tile inside one segment is all head.
//       Where the segment ends, the registers leave: a shuffle reduction in every wave, then two 64-bit atomics a wave (none for
//       a zero).  So a segment wider than the run costs the workgroup at most eight atomics, and a tile inside it none.
//     - the tail, from the start of the segment that holds the next tile's first position (a binary search, the same in every
//       lane): into the cleared registers, which go on into the next tile.
//     - the middle, the segments that begin and end inside the tile: the shape for NARROW segments.  Every lane walks its own eight
//       positions: a binary search for the segment of its first one, then a sum and a count in registers that leave with two
//       atomics wherever the lane's segment changes (none for a zero).  A segment of one position costs one atomic pair of its
//       own, one of 32 positions four lanes' pairs on one address; no reduction across lanes is tried (DESIGN.md 10.14 has the times).
//   The head and tail tests are the same in every lane, so the shuffles run with all lanes on, and there is no barrier at all.
//
// memo_feature_sums_dev: out[f][r] = sum over lo[f] <= s < hi[f] of sums[r][s], feature-major.  An inclusive prefix scan along every
//   row, in place, in three launches ordered by the stream -- the sums of tiles of 2048 segments, the exclusive scan of a row's tile
//   sums (one workgroup a row, 256 at a time with a carry), the scan of every tile from its base -- and a gather launch in which
//   neighbouring lanes write the rows of one feature: out[f][r] = P[r][hi - 1] - P[r][lo - 1], P[r][-1] = 0.  All modulo 2^64: a
//   prefix that wraps still gives exact differences.
//
// Conditions the code holds:
//   - no workgroup waits for another: no look-back, no flag in memory, no cooperative launch
//   - nothing is read outside d_vec[0 .. L) and edges[0 .. segs]: a lane whose eight values do not all lie below L loads them one by one
//   - a d_vec that is not 16-byte aligned is MEMO_EINVAL before any launch; so are decreasing edges, a slice that leaves them,
//     lo / hi outside 0 <= lo <= hi <= segs
//   - L == 0 launches nothing and leaves d_sums as it was; features == 0 launches nothing at all
//   - L and positions are int64; the tables are 64-bit; integer adds are exact in any order, so a table depends neither on the
//     slices nor on the launch shape.  The 32-bit counts cannot wrap: the launcher refuses what would give a workgroup more than
//     2^31 positions
//   - scratch: the uploaded edges ((segs + 1) x 8 bytes); lo and hi (features x 8 bytes) and the tile sums (rows x tiles x 8 bytes);
//     DevPtr owns them; an allocation that fails is MEMO_EHIP with the bytes asked for, and nothing stays allocated
//   - vector stores and plain C++ only
#include <algorithm>
#include <vector>

#include "memo_common.h"

using namespace memo;

namespace memo {
thread_local int g_features_timed = 0;      // 1 = event pairs around the launches (memo_debug_features_times)
thread_local float g_features_ms[3] = {};   // ... of the last such calls: the segment kernel; the three scan launches; the gather
}

namespace {

constexpr int kThreads = 256;
constexpr int kPerLane = 8;                    // uint16 values in a 16-byte load
constexpr int kTile = kThreads * kPerLane;     // positions a tile of the segment kernel; segments a tile of the scan
constexpr int kMaxSegs = (1 << 20) + 1;        // the segments of 2^19 features, and memo_tracks_dev's 2^20 bins
constexpr int kMaxRows = 2048;
constexpr int kMaxGridX = 1024;                // workgroups of the segment kernel at most
constexpr int kMaxGatherGrid = 1 << 16;
constexpr int64_t kMaxPositionsPerWg = (int64_t)1 << 31;

// ---- the segment table of a conservation result ---------------------------------------------------------------------------------
struct SegArgs {
    const uint16_t *vec;
    int64_t L, ntiles, tiles_per_wg;
    int segs;
    uint32_t threshold;
    const int64_t *edges;  // [segs + 1], slice coordinates, non-decreasing, edges[0] == 0 and edges[segs] == L
    uint64_t *sums;        // [2][segs]
};

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

__global__ __launch_bounds__(kThreads) void segment_kernel(const SegArgs A) {
    const int64_t t0 = (int64_t)blockIdx.x * A.tiles_per_wg, t1 = min(t0 + A.tiles_per_wg, A.ntiles);
    // the segment of the workgroup's first position (there is one: edges[segs] == L)
    int b = first_above(A.edges, 0, A.segs - 1, t0 * kTile);
    int64_t seg_end = A.edges[b + 1];
    uint64_t acc_s = 0;
    uint32_t acc_c = 0;
    auto flush = [&](int seg) {  // every lane comes here
        const uint64_t s = wave_sum(acc_s), c = wave_sum((uint64_t)acc_c);
        if ((threadIdx.x & 63) == 0 && seg < A.segs) {
            if (s) add64(A.sums + seg, s);
            if (c) add64(A.sums + A.segs + seg, c);
        }
        acc_s = 0, acc_c = 0;
    };
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t ts = t * kTile, te = min(ts + kTile, A.L), q = ts + kPerLane * (int64_t)threadIdx.x;
        uint32_t v[kPerLane];
        if (q + kPerLane <= A.L) {
            const uint4 w = *reinterpret_cast<const uint4 *>(A.vec + q);
            const uint32_t words[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int j = 0; j < kPerLane; ++j) v[j] = (words[j >> 1] >> (16 * (j & 1))) & 0xFFFFu;
        } else {
#pragma unroll
            for (int j = 0; j < kPerLane; ++j) v[j] = q + j < A.L ? A.vec[q + j] : 0u;
        }
        auto take = [&](int64_t from, int64_t to) {  // the lane's values at [from, to) into the registers
#pragma unroll
            for (int j = 0; j < kPerLane; ++j)
                if (q + j >= from && q + j < to) acc_s += v[j], acc_c += v[j] >= A.threshold;
        };
        take(ts, min(seg_end, te));                                  // the head
        if (seg_end > te || (seg_end == te && te == A.L)) continue;  // the segment goes on, or everything ends with it
        flush(b);
        // the tail's segment holds the next tile's first position; behind the last tile there is none, and all the rest is middle
        const int bl = te < A.L ? first_above(A.edges, b + 1, A.segs - 1, te) : A.segs;
        const int64_t m = te < A.L ? A.edges[bl] : A.L;  // seg_end <= m <= te
        {   // the middle [seg_end, m): the segments b + 1 .. bl - 1, each of them inside the tile
            const int64_t from = max(q, seg_end), to = min(q + kPerLane, m);
            if (from < to) {
                int s = first_above(A.edges, b + 1, bl - 1, from);  // (edges[bl] == m > from)
                int64_t s_end = A.edges[s + 1];
                uint64_t own_s = 0, own_c = 0;
                auto leave = [&]() {
                    if (own_s) add64(A.sums + s, own_s);
                    if (own_c) add64(A.sums + A.segs + s, own_c);
                    own_s = 0, own_c = 0;
                };
#pragma unroll
                for (int j = 0; j < kPerLane; ++j) {
                    const int64_t p = q + j;
                    if (p < from || p >= to) continue;
                    while (p >= s_end) {  // (p < m == edges[bl]: s stays below bl)
                        leave();
                        s_end = A.edges[++s + 1];
                    }
                    own_s += v[j], own_c += v[j] >= A.threshold;
                }
                leave();
            }
        }
        b = bl;
        if (te < A.L) {
            seg_end = A.edges[bl + 1];  // > te
            take(m, te);                // the tail
        }
    }
    flush(b);
}

// ---- from segments to features ------------------------------------------------------------------------------------------------
// the inclusive scan of one value a lane over the workgroup; total: the sum of all 256.  wtot: 4 words of LDS
__device__ inline uint64_t block_scan(uint64_t x, uint64_t *wtot, uint64_t &total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    if (lane == 63) wtot[w] = x;
    __syncthreads();
    uint64_t base = 0, all = 0;
#pragma unroll
    for (int i = 0; i < kThreads / 64; ++i) {
        const uint64_t y = wtot[i];
        if (i < w) base += y;
        all += y;
    }
    __syncthreads();  // (wtot is written again by the caller's next round)
    total = all;
    return x + base;
}

// tsum[r][t] = the sum of tile t of row r
__global__ __launch_bounds__(kThreads) void tile_sums_kernel(const uint64_t *sums, int segs, int ntiles, uint64_t *tsum) {
    __shared__ uint64_t wtot[kThreads / 64];
    const int r = blockIdx.y, t = blockIdx.x;
    const uint64_t *row = sums + (int64_t)r * segs;
    uint64_t x = 0;
    for (int i = t * kTile + (int)threadIdx.x; i < min((t + 1) * kTile, segs); i += kThreads) x += row[i];
    x = wave_sum(x);
    if ((threadIdx.x & 63) == 0) wtot[threadIdx.x >> 6] = x;
    __syncthreads();
    if (threadIdx.x == 0) tsum[(int64_t)r * ntiles + t] = wtot[0] + wtot[1] + wtot[2] + wtot[3];
}

// tsum[r][t] = the sum of the tiles before t of row r: one workgroup a row, 256 tiles at a time with a carry
__global__ __launch_bounds__(kThreads) void scan_tile_sums_kernel(uint64_t *tsum, int ntiles) {
    __shared__ uint64_t wtot[kThreads / 64];
    uint64_t *row = tsum + (int64_t)blockIdx.x * ntiles;
    uint64_t carry = 0;
    for (int base = 0; base < ntiles; base += kThreads) {
        const int i = base + (int)threadIdx.x;
        const uint64_t x = i < ntiles ? row[i] : 0;
        uint64_t total;
        const uint64_t incl = block_scan(x, wtot, total);
        if (i < ntiles) row[i] = carry + incl - x;
        carry += total;
    }
}

// sums[r][i] = the sum of sums[r][0 .. i], in place: tile t from its base tsum[r][t], 256 segments at a time with a carry
__global__ __launch_bounds__(kThreads) void scan_tiles_kernel(uint64_t *sums, int segs, int ntiles, const uint64_t *tsum) {
    __shared__ uint64_t wtot[kThreads / 64];
    const int r = blockIdx.y, t = blockIdx.x;
    uint64_t *row = sums + (int64_t)r * segs;
    uint64_t carry = tsum[(int64_t)r * ntiles + t];
    const int end = min((t + 1) * kTile, segs);
    for (int base = t * kTile; base < end; base += kThreads) {
        const int i = base + (int)threadIdx.x;
        const uint64_t x = i < end ? row[i] : 0;
        uint64_t total;
        const uint64_t incl = block_scan(x, wtot, total);
        if (i < end) row[i] = carry + incl;
        carry += total;
    }
}

// out[f][r] = P[r][hi[f] - 1] - P[r][lo[f] - 1]: the lanes of a wave write neighbouring rows of one feature
__global__ __launch_bounds__(kThreads) void gather_kernel(const uint64_t *prefix, int rows, int segs, const int32_t *lo, const int32_t *hi,
                                                          int64_t cells, uint64_t *out) {
    for (int64_t id = (int64_t)blockIdx.x * kThreads + threadIdx.x; id < cells; id += (int64_t)gridDim.x * kThreads) {
        const int64_t f = id / rows;
        const int r = (int)(id - f * rows);
        const uint64_t *row = prefix + (int64_t)r * segs;
        const int a = lo[f], b = hi[f];
        out[id] = (b ? row[b - 1] : 0) - (a ? row[a - 1] : 0);
    }
}

}  // namespace

extern "C" {

int32_t memo_segment_conservation_tile(void) { return kTile; }
int32_t memo_feature_sums_tile(void) { return kTile; }

int memo_segment_conservation_dev(const uint16_t *d_vec, int64_t L, int64_t first, const int64_t *edges_host, int32_t segs,
                                  int32_t threshold, uint64_t *d_sums, int32_t device, void *stream) {
    if (segs < 1 || segs > kMaxSegs) return fail(MEMO_EINVAL, "segs must be in [1, %d] (segs = %d)", kMaxSegs, segs);
    if (threshold < 0 || threshold > 65536) return fail(MEMO_EINVAL, "threshold must be in [0, 65536] (threshold = %d)", threshold);
    if (L < 0 || (L && !d_vec)) return fail(MEMO_EINVAL, "bad conservation result (L = %lld)", (long long)L);
    if (!edges_host) return fail(MEMO_EINVAL, "edges is NULL");
    if (!d_sums || (reinterpret_cast<uintptr_t>(d_sums) & 7)) return fail(MEMO_EINVAL, "d_sums is NULL or not 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_vec) & 15) return fail(MEMO_EINVAL, "d_vec must be 16-byte aligned");
    for (int32_t s = 0; s < segs; ++s)
        if (edges_host[s + 1] < edges_host[s])
            return fail(MEMO_EINVAL, "the segment edges decrease: edge %d is %lld, edge %d is %lld", s, (long long)edges_host[s], s + 1,
                        (long long)edges_host[s + 1]);
    // (first + L cannot wrap where it matters: L <= edges[segs] - first is asked instead)
    if (first < edges_host[0] || first > edges_host[segs] || L > edges_host[segs] - first)
        return fail(MEMO_EINVAL, "the slice [%lld, %lld + %lld) leaves the segment edges [%lld, %lld)", (long long)first, (long long)first,
                    (long long)L, (long long)edges_host[0], (long long)edges_host[segs]);
    if (!L) return MEMO_OK;

    SegArgs A = {};
    A.vec = d_vec;
    A.L = L;
    A.segs = segs;
    A.threshold = (uint32_t)threshold;
    A.sums = d_sums;
    A.ntiles = (L + kTile - 1) / kTile;
    const int64_t cap = std::min<int64_t>(kMaxGridX, A.ntiles);
    A.tiles_per_wg = (A.ntiles + cap - 1) / cap;
    if (A.tiles_per_wg * kTile > kMaxPositionsPerWg) return fail(MEMO_EINVAL, "a result of %lld positions is too long", (long long)L);
    const int gx = (int)((A.ntiles + A.tiles_per_wg - 1) / A.tiles_per_wg);
    // the edges in slice coordinates: [0, L] cut into consecutive segments, the first edge 0 and the last one L
    std::vector<int64_t> rel((size_t)segs + 1);
    for (int32_t s = 0; s <= segs; ++s) rel[s] = std::min<int64_t>(std::max<int64_t>(edges_host[s] - first, 0), L);

    OnDevice on(device);
    if (on.rc) return on.rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    DevPtr<int64_t> d_edges;
    if (hipError_t err = d_edges.alloc(rel.size()); err != hipSuccess)
        return fail(MEMO_EHIP, "hipMalloc(%zu bytes) for the edges of %d segments: %s", rel.size() * sizeof(int64_t), segs, hipGetErrorString(err));
    HIP_TRY(hipMemcpyAsync(d_edges, rel.data(), rel.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
    A.edges = d_edges;
    Laps laps(st, g_features_timed, g_features_ms);
    if (int rc = laps.start()) return rc;
    hipLaunchKernelGGL(segment_kernel, dim3((unsigned)gx), dim3(kThreads), 0, st, A);
    HIP_TRY(hipGetLastError());
    if (int rc = laps.lap(0)) return rc;
    HIP_TRY(hipStreamSynchronize(st));  // (rel and d_edges go with this frame)
    return MEMO_OK;
}

int memo_feature_sums_dev(uint64_t *d_sums, int32_t rows, int32_t segs, const int32_t *lo_host, const int32_t *hi_host, int32_t features,
                          uint64_t *d_out, int32_t device, void *stream) {
    if (rows < 1 || rows > kMaxRows) return fail(MEMO_EINVAL, "rows must be in [1, %d] (rows = %d)", kMaxRows, rows);
    if (segs < 1 || segs > kMaxSegs) return fail(MEMO_EINVAL, "segs must be in [1, %d] (segs = %d)", kMaxSegs, segs);
    if (features < 0) return fail(MEMO_EINVAL, "features must not be negative (features = %d)", features);
    if (!d_sums || (reinterpret_cast<uintptr_t>(d_sums) & 7)) return fail(MEMO_EINVAL, "d_sums is NULL or not 8-byte aligned");
    if (features && (!lo_host || !hi_host)) return fail(MEMO_EINVAL, "lo or hi is NULL");
    if (features && (!d_out || (reinterpret_cast<uintptr_t>(d_out) & 7))) return fail(MEMO_EINVAL, "d_out is NULL or not 8-byte aligned");
    for (int32_t f = 0; f < features; ++f)
        if (lo_host[f] < 0 || lo_host[f] > hi_host[f] || hi_host[f] > segs)
            return fail(MEMO_EINVAL, "feature %d: the segments [%d, %d) are not inside [0, %d]", f, lo_host[f], hi_host[f], segs);
    if (!features) return MEMO_OK;

    const int ntiles = (segs + kTile - 1) / kTile;
    OnDevice on(device);
    if (on.rc) return on.rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    DevPtr<int32_t> d_lohi;
    DevPtr<uint64_t> d_tsum;
    if (hipError_t err = d_lohi.alloc(2 * (size_t)features); err != hipSuccess)
        return fail(MEMO_EHIP, "hipMalloc(%zu bytes) for the segments of %d features: %s", 2 * (size_t)features * sizeof(int32_t), features,
                    hipGetErrorString(err));
    if (hipError_t err = d_tsum.alloc((size_t)rows * ntiles); err != hipSuccess)
        return fail(MEMO_EHIP, "hipMalloc(%zu bytes) for the tile sums of %d rows: %s", (size_t)rows * ntiles * sizeof(uint64_t), rows,
                    hipGetErrorString(err));
    HIP_TRY(hipMemcpyAsync(d_lohi, lo_host, (size_t)features * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_lohi + features, hi_host, (size_t)features * sizeof(int32_t), hipMemcpyHostToDevice, st));
    Laps laps(st, g_features_timed, g_features_ms);
    if (int rc = laps.start()) return rc;
    hipLaunchKernelGGL(tile_sums_kernel, dim3((unsigned)ntiles, (unsigned)rows), dim3(kThreads), 0, st, d_sums, segs, ntiles, d_tsum.p);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(scan_tile_sums_kernel, dim3((unsigned)rows), dim3(kThreads), 0, st, d_tsum.p, ntiles);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(scan_tiles_kernel, dim3((unsigned)ntiles, (unsigned)rows), dim3(kThreads), 0, st, d_sums, segs, ntiles, d_tsum.p);
    HIP_TRY(hipGetLastError());
    if (int rc = laps.lap(1)) return rc;
    const int64_t cells = (int64_t)features * rows;
    const int gx = (int)std::min<int64_t>((cells + kThreads - 1) / kThreads, kMaxGatherGrid);
    hipLaunchKernelGGL(gather_kernel, dim3((unsigned)gx), dim3(kThreads), 0, st, d_sums, rows, segs, d_lohi.p, d_lohi.p + features, cells, d_out);
    HIP_TRY(hipGetLastError());
    if (int rc = laps.lap(2)) return rc;
    HIP_TRY(hipStreamSynchronize(st));  // (the scratch goes with this frame)
    return MEMO_OK;
}

}  // extern "C"
