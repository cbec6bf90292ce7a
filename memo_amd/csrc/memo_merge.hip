// memo_merge.hip -- `memo merge`: the row builder's matrix of chosen genomes, in a chosen order, from the planes of one or more membership
// indexes on one pivot.  The planes of all inputs lie stacked in one buffer with one pitch, genome-major uint32 as memo_lengths.hip leaves
// them (cell[plane][p]: how far that genome matches the pivot from position p); a column map names the plane of every column of the
// position-major int32 matrix (memo_dap.hip reads it), clipped at the end of the record:
//     dap[i][c] = min( cell[plane_of[c]][first + i], remaining - i )            0 <= i < positions, 0 <= c < cols
// A plane may be named by no column, by one or by several; an entry outside [0, planes) names none and its column is 0.  No counterpart in
// the reference.
//
// merge_dap_kernel is the transposition of memo_planes_dap.h (the lane layout, the bank argument, the conditions the code holds) with
// the mapped source: the 64 plane bases of a tile are taken from the map; how the map is read, and what else was built for it and
// dropped, stands there.  Nothing outside plane_of[0 .. cols) is read.  Besides the refusals listed there, MEMO_EINVAL for planes outside
// [1, 65 536] and cols outside [1, 2047].
#include "memo_planes_dap.h"

using namespace memo;
using namespace memo::planes_dap;

namespace {

constexpr int kMaxPlanes = 65536;
constexpr int kMaxCols = 2047;

struct MergeArgs {
    Frame f;
    const uint32_t *cells;    // plane 0 of the stack
    const int32_t *plane_of;  // cols entries
    int planes;
};

__global__ __launch_bounds__(kThreads) void merge_dap_kernel(const MergeArgs A) {
    __shared__ uint32_t tile[kTG * kStride];
    const Tile T = tile_of(A.f);
    load_planes(tile, A.f, T, T.ng, Mapped{A.cells, A.plane_of + T.c0, A.planes});
    __syncthreads();
    store_rows(tile, A.f, T);
}

}  // namespace

extern "C" {

int32_t memo_merge_tile(void) { return kTP; }

int memo_merge_dap_dev(const uint32_t *d_cells, int64_t pitch, int32_t planes, const int32_t *d_plane_of, int32_t cols, int64_t first,
                       int64_t positions, int64_t remaining, int32_t *d_dap, int32_t device, void *stream) {
    if (planes < 1 || planes > kMaxPlanes) return fail(MEMO_EINVAL, "planes must be in [1, %d] (got %d)", kMaxPlanes, planes);
    if (cols < 1 || cols > kMaxCols) return fail(MEMO_EINVAL, "cols must be in [1, %d] (got %d)", kMaxCols, cols);
    if (int rc = refuse(d_cells, pitch, first, positions, remaining, d_dap, d_plane_of, "d_plane_of")) return rc;
    if (!positions) return MEMO_OK;
    if (!d_cells || !d_plane_of || !d_dap) return fail(MEMO_EINVAL, "d_cells, d_plane_of or d_dap is NULL");
    return launch(merge_dap_kernel, MergeArgs{frame(pitch, first, positions, remaining, cols, d_dap), d_cells, d_plane_of, planes}, device, stream);
}

}  // extern "C"
