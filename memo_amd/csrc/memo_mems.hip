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
// Both are keys of memo_compact.h's compaction (CellsKey<kBand>): a lane owns the four cells of one 16-byte load, a tile is 256 lanes x
// 4 loads x 4 cells, and the tiles run over planes x ceil(L / tile) -- a tile never crosses a plane, and the tile order is plane-major.
// Four launches, ordered by the stream: the count, the scan of the tile counts, the gather of the bases at the plane boundaries and
// the total into planes + 1 entries (the host reads them in one copy, takes the per-plane counts as their differences and allocates
// exactly the total), and the scatter: starts[rank] = i, lengths[rank] = v[i], plane-major, ascending within a plane.
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
#include "memo_compact.h"

using namespace memo;

namespace memo {
thread_local int g_mems_timed = 0;                   // 1 = event pairs around the launches (memo_debug_mems_times)
thread_local float g_mems_ms[3] = {0.f, 0.f, 0.f};  // ... of the last such call: count, scan + plane bases, scatter
}

namespace {

template <bool kBand>
struct CellsKey {
    static constexpr int kPer = 4;  // a lane owns the four cells of one 16-byte load
    using Start = uint32_t;
    const uint32_t *cells;
    uint32_t *lengths;  // nullptr for the band
    int64_t L, pitch, tiles_per_plane;
    uint32_t cap, min_len;
    int halo;

    __device__ __forceinline__ void tile_of(int64_t block, int64_t &plane, int64_t &p0) const {
        plane = block / tiles_per_plane;
        p0 = (block - plane * tiles_per_plane) * tile_positions<CellsKey>();
    }

    __device__ __forceinline__ uint32_t flags(int64_t plane, int64_t p) const {
        const uint32_t *__restrict__ v = cells + plane * pitch;
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
            const bool first = j == 0 && p == 0, in = cur >= min_len;  // (prev is not a cell's value at the first cell of a plane)
            bool f;
            if (kBand) f = in != (first ? false : prev >= min_len);
            else f = in && (first ? !halo : prev < cur || (prev == cur && cur < cap));
            m |= (uint32_t)(f && p + j < L) << j;
            prev = cur;
        }
        return m;
    }

    __device__ __forceinline__ void store(int64_t plane, int64_t rank, int64_t i) const {
        if (!kBand) lengths[rank] = cells[plane * pitch + i];  // flagged: i < L
    }
};

constexpr int kTile = tile_positions<CellsKey<false>>();

// count, scan, the plane bases to the host, allocate exactly, scatter.  Blocking.
template <bool kBand>
int compact(CellsKey<kBand> key, int64_t planes, uint32_t **d_starts, uint32_t **d_lengths, uint64_t *counts, hipStream_t st) {
    Compaction c(st, g_mems_timed, g_mems_ms);
    const int64_t ntiles = planes * key.tiles_per_plane;
    if (hipError_t err = c.lay_out(ntiles, planes); err != hipSuccess)
        return fail(MEMO_EHIP, "hipMalloc(%zu bytes) for the counts of %lld tiles: %s", c.work_bytes, (long long)ntiles, hipGetErrorString(err));
    if (int rc = c.count(key)) return rc;
    const int64_t total = c.total();
    if (total <= 0) return MEMO_OK;
    DevPtr<uint32_t> starts, lengths;
    const size_t bytes = (size_t)total * sizeof(uint32_t);
    if (hipError_t err = starts.alloc((size_t)total); err != hipSuccess)
        return fail(MEMO_EHIP, "hipMalloc(%zu bytes) for the starts of %lld matches: %s", bytes, (long long)total, hipGetErrorString(err));
    if (!kBand)
        if (hipError_t err = lengths.alloc((size_t)total); err != hipSuccess)
            return fail(MEMO_EHIP, "hipMalloc(%zu bytes) for the lengths of %lld matches: %s", bytes, (long long)total, hipGetErrorString(err));
    key.lengths = lengths;
    if (int rc = c.scatter(key, starts.p)) return rc;
    for (int64_t pl = 0; pl < planes; ++pl) counts[pl] = (uint64_t)(c.plane_base[(size_t)pl + 1] - c.plane_base[(size_t)pl]);
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
    const int64_t tiles_per_plane = (L + kTile - 1) / kTile;
    if ((int64_t)planes * tiles_per_plane > INT32_MAX)
        return fail(MEMO_EINVAL, "%d planes of %lld cells are too many tiles for one launch", planes, (long long)L);
    OnDevice on(device);
    if (on.rc) return on.rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (key == 2) return compact(CellsKey<true>{d_cells, nullptr, L, pitch, tiles_per_plane, cap, min_len, halo}, planes, d_starts, d_lengths, counts, st);
    return compact(CellsKey<false>{d_cells, nullptr, L, pitch, tiles_per_plane, cap, min_len, halo}, planes, d_starts, d_lengths, counts, st);
}

}  // extern "C"
