// memo_add.hip -- `memo add`: the row builder's matrix of N + m genomes from two sources.  The old genomes' columns are read back from the
// membership index as genome-major uint32 planes (memo_lengths.hip: cell[g][p]), as `memo convert` reads them; the new genomes' columns
// are matching statistics computed now, position-major int32 rows [positions][new_cols] (memo_ms.hip: memo_ms_rows_dev).  Both become
// ONE position-major int32 matrix of W = N - 1 + new_cols columns (memo_dap.hip reads it), clipped at the end of the record:
//     dap[i][c] = min( cell[c + 1][first + i], remaining - i )                  0 <= c < N - 1         0 <= i < positions
//     dap[i][c] = min( (uint32) new[i][c - (N - 1)], remaining - i )            N - 1 <= c < W
// Plane 0, the pivot, is not read: a DAP has no column for it.  No counterpart in the reference.
//
// add_dap_kernel is the transposition of memo_planes_dap.h (the lane layout, the bank argument, the conditions the code holds) over the
// COMBINED column space [0, W): a tile holds old columns, new columns or both, staged through one LDS tile, so that an output row
// segment is written in one contiguous run whatever (N - 1) mod 64 is.  The old columns come by the straight source, column c is
// plane 1 + c.  What is its own:
//   load   new columns (either kind of tile): the column index fastest across lanes, element e = q * nn + j (nn new columns in this tile):
//          lane t takes e = t, t + 256 ...; a row's nn values are one contiguous run of d_new, and with nn = new_cols (the whole of the
//          new columns in one tile) so is the tile's whole piece of d_new.  Rows outside [0, positions) are not read.  (q, j) advance by
//          (256 / nn, 256 % nn) with one carry: one division per lane and tile.
//   LDS    the new columns' store of element (q, j) goes to word (no + j) * 129 + q: 32 neighbouring j per group are 32 banks
//          (129 mod 32 = 1); where a group runs over the end of one row's columns into the next row's it is 2-way at most.
// Nothing is read outside d_new[0 .. positions * new_cols); offsets into it are 64-bit.  Besides the refusals listed there, MEMO_EINVAL
// for N outside [2, 2047], new_cols outside [1, 2047] and W > 2047.
#include "memo_planes_dap.h"

using namespace memo;
using namespace memo::planes_dap;

namespace {

constexpr int kMaxWidth = 2047;           // columns of the matrix, and each of its two parts

struct AddArgs {
    Frame f;                // cols: W
    const uint32_t *cells;  // plane 0
    const int32_t *fresh;   // the new columns' rows
    int old_cols;           // N - 1
    int new_cols;
};

__global__ __launch_bounds__(kThreads) void add_dap_kernel(const AddArgs A) {
    __shared__ uint32_t tile[kTG * kStride];
    const Tile T = tile_of(A.f);
    const int no = max(0, min(T.ng, A.old_cols - T.c0));  // the first `no` of the tile's columns are old, the other nn new
    const int nn = T.ng - no;
    if (no > 0) load_planes(tile, A.f, T, no, Straight{A.cells + (int64_t)(1 + T.c0) * A.f.pitch});
    if (nn > 0) {
        const int j0 = T.c0 + no - A.old_cols;  // the tile's first new column
        const int dq = kThreads / nn, dj = kThreads % nn;
        int q = threadIdx.x / nn, j = threadIdx.x % nn;
        while (q < kTP) {
            const int64_t at = T.t0 + q - A.f.first;  // the row of both matrices
            if (at >= 0 && at < A.f.positions) tile[(no + j) * kStride + q] = (uint32_t)A.fresh[at * A.new_cols + j0 + j];
            q += dq, j += dj;
            if (j >= nn) j -= nn, ++q;
        }
    }
    __syncthreads();
    store_rows(tile, A.f, T);
}

}  // namespace

extern "C" {

int32_t memo_add_tile(void) { return kTP; }

int memo_add_dap_dev(const uint32_t *d_cells, int64_t pitch, int32_t num_docs, int64_t first, int64_t positions, int64_t remaining,
                     const int32_t *d_new, int32_t new_cols, int32_t *d_dap, int32_t device, void *stream) {
    if (num_docs < 2 || num_docs > kMaxWidth) return fail(MEMO_EINVAL, "num_docs must be in [2, %d] (got %d)", kMaxWidth, num_docs);
    if (new_cols < 1 || new_cols > kMaxWidth) return fail(MEMO_EINVAL, "new_cols must be in [1, %d] (got %d)", kMaxWidth, new_cols);
    if (num_docs - 1 + new_cols > kMaxWidth)
        return fail(MEMO_EINVAL, "num_docs - 1 + new_cols = %d columns: the limit is %d", num_docs - 1 + new_cols, kMaxWidth);
    if (int rc = refuse(d_cells, pitch, first, positions, remaining, d_dap, d_new, "d_new")) return rc;
    if (!positions) return MEMO_OK;
    if (!d_cells || !d_new || !d_dap) return fail(MEMO_EINVAL, "d_cells, d_new or d_dap is NULL");
    const AddArgs A = {frame(pitch, first, positions, remaining, num_docs - 1 + new_cols, d_dap), d_cells, d_new, num_docs - 1, new_cols};
    return launch(add_dap_kernel, A, device, stream);
}

}  // extern "C"
