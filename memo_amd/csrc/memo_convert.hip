// memo_convert.hip -- `memo convert`: the step between the planes of `memo lengths` and the row builder of `memo index`.  A finished slice
// of genome-major uint32 planes (memo_lengths.hip: cell[g][p], how far genome g matches the pivot from position p) becomes the
// position-major int32 matrix the row builder reads (memo_dap.hip: one row per position, one column per non-pivot genome), clipped at
// the end of the record:
//     dap[i][g - 1] = min( cell[g][first + i], remaining - i )        0 <= i < positions, 1 <= g < N
// Plane 0, the pivot, is not read: a DAP has no column for it.  No counterpart in the reference.
//
// convert_dap_kernel is the transposition of memo_planes_dap.h (the lane layout, the bank argument, the conditions the code holds) with
// the straight source: column c is plane 1 + c.  Besides the refusals listed there, MEMO_EINVAL for N outside [2, 2048].
#include "memo_planes_dap.h"

using namespace memo;
using namespace memo::planes_dap;

namespace {

constexpr int kMaxDocs = 2048;

struct ConvertArgs {
    Frame f;
    const uint32_t *cells;  // plane 0
};

__global__ __launch_bounds__(kThreads) void convert_dap_kernel(const ConvertArgs A) {
    __shared__ uint32_t tile[kTG * kStride];
    const Tile T = tile_of(A.f);
    load_planes(tile, A.f, T, T.ng, Straight{A.cells + (int64_t)(1 + T.c0) * A.f.pitch});
    __syncthreads();
    store_rows(tile, A.f, T);
}

}  // namespace

extern "C" {

int32_t memo_convert_tile(void) { return kTP; }

int memo_convert_dap_dev(const uint32_t *d_cells, int64_t pitch, int32_t num_docs, int64_t first, int64_t positions, int64_t remaining,
                         int32_t *d_dap, int32_t device, void *stream) {
    if (num_docs < 2 || num_docs > kMaxDocs) return fail(MEMO_EINVAL, "num_docs must be in [2, %d] (got %d)", kMaxDocs, num_docs);
    if (int rc = refuse(d_cells, pitch, first, positions, remaining, d_dap)) return rc;
    if (!positions) return MEMO_OK;
    if (!d_cells || !d_dap) return fail(MEMO_EINVAL, "d_cells or d_dap is NULL");
    return launch(convert_dap_kernel, ConvertArgs{frame(pitch, first, positions, remaining, num_docs - 1, d_dap), d_cells}, device, stream);
}

}  // extern "C"
