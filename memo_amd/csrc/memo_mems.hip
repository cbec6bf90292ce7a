// memo_mems.hip -- `memo mems`: the maximal shared matches of a window from the finished lengths of `memo maxk` / `memo lengths` that
// are still in HBM, compacted there, so that a list of matches and not one line per position leaves the device.  No counterpart in
// the reference.
//
// The cells are uint32 [planes][pitch], L of them per plane (memo_lengths_*_dev's layout; memo_maxk_*_dev's cells and
// memo_lengths_select_dev's output are one plane of it).  Two keys over every plane by itself:
//   starts  cell i is REPORTED when v[i] >= min_len and it starts a match: v[i - 1] < v[i], or v[i - 1] == v[i] < cap (a run at the
//           cap is one match, reported at its first cell).  Cell 0 has no left neighbour: with halo = 0 it is position 0 of its record
//           and is reported where v[0] >= min_len; with halo = 1 it is only the neighbour of cell 1 and is never reported.
//           starts[r] = i and lengths[r] = v[i] per reported cell
//   band    the boundaries of v[i] >= min_len, the cell before cell 0 counting as false (memo_runs.hip's band key): only boundaries
//           are stored, 2j opens an interval, 2j + 1 closes it, an odd count leaves a plane's last interval to end at L
// One code path, a template on the key.  A lane owns the four cells of one 16-byte load.
//
// Four launches, ordered by the stream (memo_runs.hip's structure):
//   mems_count_kernel    per tile of 256 lanes x 4 loads x 4 cells: its flags counted, one uint32 per tile, no atomics.  The tiles run
//                        over planes x ceil(L / tile): a tile never crosses a plane, and the tile order is plane-major
//   the scan             memo::scan_tile_counts: int64 bases and the total
//   mems_plane_bases     the bases at the plane boundaries and the total, gathered into planes + 1 entries: the host reads them in one
//                        copy, takes the per-plane counts as their differences and allocates exactly the total
//   mems_scatter_kernel  the flags recomputed; rank = tile base + the flags of the waves before + of the loads before + of the lanes
//                        below (ballot / mbcnt); starts[rank] = i, lengths[rank] = v[i]: plane-major, ascending within a plane
//
// Conditions the code holds:
//   - no workgroup waits for another: no look-back, no flag in memory, no cooperative launch
//   - nothing is read outside [0, L) of a plane: a lane's first cell is compared with the lane below through a wave shuffle, a wave's
//     first with one extra load of v[i - 1] that is not made at i == 0; a load that would cross L is made cell by cell for the cells
//     before L.  The cells [L, pitch) are never read
//   - d_cells is 16-byte aligned and pitch a multiple of 4, so every four-cell load is aligned (anything else is MEMO_EINVAL before
//     any launch)
//   - L == 0 or planes == 0 launches nothing; tile counts are uint32, bases and totals 64-bit
//   - a cell at or past L never sets a flag, and the scatter writes no rank at or past the total
//   - vector loads and stores only; no inline assembly
#include <vector>

#include "memo_common.h"

using namespace memo;

namespace memo {
thread_local int g_mems_timed = 0;                   // 1 = event pairs around the launches (memo_debug_mems_times)
thread_local float g_mems_ms[3] = {0.f, 0.f, 0.f};  // ... of the last such call: count, scan + plane bases, scatter
}

namespace {

constexpr int kThreads = 256, kIters = 4, kPer = 4;  // a wave owns kIters x 64 x kPer cells in a row
constexpr int kTile = kThreads * kIters * kPer;

struct Planes {
    const uint32_t *cells;
    int64_t L, pitch, tiles_per_plane;
    uint32_t cap, min_len;
    int halo;
};

struct Tile {
    const uint32_t *v;  // the plane
    int64_t tile0;      // the tile's first cell
};

__device__ __forceinline__ Tile tile_of(const Planes &P) {
    const int64_t plane = (int64_t)blockIdx.x / P.tiles_per_plane, tile = (int64_t)blockIdx.x - plane * P.tiles_per_plane;
    return {P.cells + plane * P.pitch, tile * kTile};
}

__device__ __forceinline__ int64_t chunk_pos(int64_t tile0, int it) {
    return tile0 + (int64_t)(((threadIdx.x >> 6) * kIters + it) * 64 + (threadIdx.x & 63)) * kPer;
}

// bit j: cell p + j (p a multiple of kPer) is flagged.  Called by whole waves (it shuffles).
template <bool kBand>
__device__ __forceinline__ uint32_t flags(const Planes &P, const uint32_t *__restrict__ v, int64_t p) {
    const int64_t L = P.L;
    uint32_t e[kPer];
    if (p + kPer <= L) {
        const uint4 q = *reinterpret_cast<const uint4 *>(v + p);
        e[0] = q.x, e[1] = q.y, e[2] = q.z, e[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < kPer; ++j) e[j] = p + j < L ? v[p + j] : 0u;
    }
    uint32_t prev = (uint32_t)__shfl_up((int)e[kPer - 1], 1, 64);
    if ((threadIdx.x & 63) == 0 && p > 0 && p < L) prev = v[p - 1];
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        const uint32_t cur = e[j];
        const bool first = j == 0 && p == 0, in = cur >= P.min_len;  // (prev is not a cell's value at the first cell of a plane)
        bool f;
        if (kBand) f = in != (first ? false : prev >= P.min_len);
        else f = in && (first ? !P.halo : prev < cur || (prev == cur && cur < P.cap));
        m |= (uint32_t)(f && p + j < L) << j;
        prev = cur;
    }
    return m;
}

template <bool kBand>
__global__ __launch_bounds__(kThreads) void mems_count_kernel(Planes P, uint32_t *__restrict__ counts) {
    __shared__ uint32_t wsum[kThreads / 64];
    const Tile t = tile_of(P);
    uint32_t n = 0;
#pragma unroll
    for (int it = 0; it < kIters; ++it) n += (uint32_t)__popc(flags<kBand>(P, t.v, chunk_pos(t.tile0, it)));
    for (int off = 32; off; off >>= 1) n += __shfl_xor(n, off, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// out[pl] = the base of plane pl's first tile, out[planes] = the total
__global__ __launch_bounds__(kThreads) void mems_plane_bases(const int64_t *__restrict__ bases, const int64_t *__restrict__ total,
                                                             int64_t tiles_per_plane, int64_t planes, int64_t *__restrict__ out) {
    const int64_t pl = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (pl < planes) out[pl] = bases[pl * tiles_per_plane];
    else if (pl == planes) out[pl] = *total;
}

template <bool kBand>
__global__ __launch_bounds__(kThreads) void mems_scatter_kernel(Planes P, const int64_t *__restrict__ bases, int64_t total,
                                                                uint32_t *__restrict__ starts, uint32_t *__restrict__ lengths) {
    __shared__ uint32_t wtot[kThreads / 64];
    const Tile t = tile_of(P);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // rank of a lane's first flag among its wave's: the lanes below by ballot + mbcnt, the loads before by a running sum
    uint32_t mask[kIters], rank[kIters], running = 0;
#pragma unroll
    for (int it = 0; it < kIters; ++it) {
        const uint32_t m = flags<kBand>(P, t.v, chunk_pos(t.tile0, it));
        uint32_t below = 0, count = 0;
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            const unsigned long long bal = __ballot((m >> j) & 1u);
            below += __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
            count += (uint32_t)__popcll(bal);
        }
        mask[it] = m;
        rank[it] = running + below;
        running += count;
    }
    if (lane == 0) wtot[wave] = running;
    __syncthreads();
    int64_t base = bases[blockIdx.x];
    for (int w = 0; w < wave; ++w) base += wtot[w];
#pragma unroll
    for (int it = 0; it < kIters; ++it) {
        int64_t idx = base + rank[it];
        const int64_t p = chunk_pos(t.tile0, it);
        for (uint32_t m = mask[it]; m; m &= m - 1, ++idx) {
            if (idx >= total) break;  // (cannot happen while both passes see the same cells: a caller that writes them meanwhile)
            const int64_t i = p + __builtin_ctz(m);  // flagged: i < L
            starts[idx] = (uint32_t)i;
            if (!kBand) lengths[idx] = t.v[i];
        }
    }
}

// event pairs around the launches of a timed call (memo_debug_mems_times), as memo_maxk.hip's
struct Laps {
    hipEvent_t e[2] = {};
    hipStream_t st;
    explicit Laps(hipStream_t s) : st(s) {}
    ~Laps() {
        for (hipEvent_t x : e)
            if (x) (void)hipEventDestroy(x);
    }
    int start() {
        if (!g_mems_timed) return MEMO_OK;
        for (hipEvent_t &x : e)
            if (!x) HIP_TRY(hipEventCreate(&x));
        HIP_TRY(hipEventRecord(e[0], st));
        return MEMO_OK;
    }
    int lap(int i) {
        if (!g_mems_timed) return MEMO_OK;
        float ms = 0.f;
        HIP_TRY(hipEventRecord(e[1], st));
        HIP_TRY(hipEventSynchronize(e[1]));
        HIP_TRY(hipEventElapsedTime(&ms, e[0], e[1]));
        g_mems_ms[i] = ms;
        HIP_TRY(hipEventRecord(e[0], st));
        return MEMO_OK;
    }
};

// count, scan, the plane bases to the host, allocate exactly, scatter.  Blocking.
template <bool kBand>
int compact(Planes P, int64_t planes, uint32_t **d_starts, uint32_t **d_lengths, uint64_t *counts, hipStream_t st) {
    const int64_t ntiles = planes * P.tiles_per_plane;
    // one allocation: the total, the tiles' bases, the planes' bases and the total again, the tiles' counts
    DevPtr<int64_t> work;
    const size_t words = (size_t)(1 + ntiles + planes + 1 + (ntiles + 1) / 2);
    if (hipError_t err = work.alloc(words); err != hipSuccess)
        return fail(MEMO_EHIP, "hipMalloc(%zu bytes) for the counts of %lld tiles: %s", words * sizeof(int64_t), (long long)ntiles,
                    hipGetErrorString(err));
    int64_t *d_total = work, *d_bases = d_total + 1, *d_plane = d_bases + ntiles;
    uint32_t *d_counts = reinterpret_cast<uint32_t *>(d_plane + planes + 1);
    Laps laps(st);
    if (int rc = laps.start()) return rc;
    hipLaunchKernelGGL(mems_count_kernel<kBand>, dim3((unsigned)ntiles), dim3(kThreads), 0, st, P, d_counts);
    HIP_TRY(hipGetLastError());
    if (int rc = laps.lap(0)) return rc;
    HIP_TRY(scan_tile_counts(d_counts, ntiles, d_bases, d_total, st));
    hipLaunchKernelGGL(mems_plane_bases, dim3((unsigned)(planes / kThreads + 1)), dim3(kThreads), 0, st, d_bases, d_total,
                       P.tiles_per_plane, planes, d_plane);
    HIP_TRY(hipGetLastError());
    if (int rc = laps.lap(1)) return rc;
    std::vector<int64_t> plane_base((size_t)planes + 1);
    HIP_TRY(hipMemcpyAsync(plane_base.data(), d_plane, plane_base.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int64_t total = plane_base[(size_t)planes];
    if (total <= 0) return MEMO_OK;
    DevPtr<uint32_t> starts, lengths;
    const size_t bytes = (size_t)total * sizeof(uint32_t);
    if (hipError_t err = starts.alloc((size_t)total); err != hipSuccess)
        return fail(MEMO_EHIP, "hipMalloc(%zu bytes) for the starts of %lld matches: %s", bytes, (long long)total, hipGetErrorString(err));
    if (!kBand)
        if (hipError_t err = lengths.alloc((size_t)total); err != hipSuccess)
            return fail(MEMO_EHIP, "hipMalloc(%zu bytes) for the lengths of %lld matches: %s", bytes, (long long)total, hipGetErrorString(err));
    if (int rc = laps.start()) return rc;
    hipLaunchKernelGGL(mems_scatter_kernel<kBand>, dim3((unsigned)ntiles), dim3(kThreads), 0, st, P, d_bases, total, starts.p, lengths.p);
    HIP_TRY(hipGetLastError());
    if (int rc = laps.lap(2)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    for (int64_t pl = 0; pl < planes; ++pl) counts[pl] = (uint64_t)(plane_base[(size_t)pl + 1] - plane_base[(size_t)pl]);
    *d_starts = starts.release();
    if (!kBand) *d_lengths = lengths.release();
    return MEMO_OK;
}

}  // namespace

extern "C" {

int32_t memo_mems_tile(void) { return kTile; }

int memo_mems_dev(const uint32_t *d_cells, int64_t L, int64_t pitch, int32_t planes, uint32_t cap, uint32_t min_len, int32_t key,
                  int32_t halo, uint32_t **d_starts, uint32_t **d_lengths, uint64_t *counts, int32_t device, void *stream) {
    if (key != 1 && key != 2) return fail(MEMO_EINVAL, "key %d: 1 (the starts of the matches) or 2 (the boundaries of the band)", key);
    if (!d_starts || (key == 1 && !d_lengths)) return fail(MEMO_EINVAL, "d_starts / d_lengths is NULL");
    *d_starts = nullptr;
    if (d_lengths) *d_lengths = nullptr;
    if (planes < 0) return fail(MEMO_EINVAL, "planes must not be negative (got %d)", planes);
    if (planes && !counts) return fail(MEMO_EINVAL, "counts is NULL");
    for (int32_t pl = 0; pl < planes; ++pl) counts[pl] = 0;
    if (L < 0 || L > ((int64_t)1 << 31)) return fail(MEMO_EINVAL, "L = %lld: a plane holds at most 2^31 cells", (long long)L);
    if (pitch < L || (pitch & 3)) return fail(MEMO_EINVAL, "pitch %lld must be a multiple of 4 and at least L = %lld", (long long)pitch, (long long)L);
    if (cap < 1 || cap > 0x7fffffffu) return fail(MEMO_EINVAL, "cap %u must be in [1, 2^31 - 1]", cap);
    if (min_len < 1 || min_len > cap) return fail(MEMO_EINVAL, "min_len %u must be in [1, cap = %u]", min_len, cap);
    if (halo != 0 && halo != 1) return fail(MEMO_EINVAL, "halo %d: 0 (cell 0 is a record's first position) or 1 (cell 0 is only a neighbour)", halo);
    if (key == 2 && halo) return fail(MEMO_EINVAL, "the band key takes no halo: the cell before cell 0 counts as outside the band");
    if (reinterpret_cast<uintptr_t>(d_cells) & 15) return fail(MEMO_EINVAL, "d_cells must be 16-byte aligned");
    if (L && planes && !d_cells) return fail(MEMO_EINVAL, "d_cells is NULL");
    if (!L || !planes) return MEMO_OK;
    Planes P = {d_cells, L, pitch, (L + kTile - 1) / kTile, cap, min_len, halo};
    if ((int64_t)planes * P.tiles_per_plane > INT32_MAX)
        return fail(MEMO_EINVAL, "%d planes of %lld cells are too many tiles for one launch", planes, (long long)L);
    if (int rc = device_ok(device)) return rc;
    DeviceGuard guard(device);
    if (!guard.ok) return fail(MEMO_EHIP, "cannot select HIP device %d", device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    return key == 2 ? compact<true>(P, planes, d_starts, d_lengths, counts, st) : compact<false>(P, planes, d_starts, d_lengths, counts, st);
}

}  // extern "C"
