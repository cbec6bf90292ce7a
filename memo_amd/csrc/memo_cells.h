// memo_cells.h -- the row pass over planes of cells that memo_maxk.hip and memo_lengths.hip share: the three int64 columns streamed 16
// bytes a lane and load, and the cell and value a row bounds.  The passes over the planes themselves -- fill, carry-in, tile minima,
// their scan, apply -- are memo_cells.hip's, behind the launchers that memo_common.h declares.  Not part of the public ABI.
//
// Cells.  uint32 cell[planes][pitch], relative to the window's start qs, L <= pitch of them per plane.  The identity is ident = L - 1 +
// CAP (L <= 2^31 and CAP < 2^31: below 2^32); every value is saturated to [0, ident], which is exact: a bound at or above ident yields
// CAP at every position.
#ifndef MEMO_CELLS_H
#define MEMO_CELLS_H

#include <algorithm>

#include "memo_common.h"

namespace memo {

constexpr int kRowThreads = 256;
constexpr int kLoads = 4;                                       // 16-byte loads of each column a lane has in flight
constexpr int64_t kPairsPerWg = (int64_t)kRowThreads * kLoads;  // row pairs a workgroup takes at a time
constexpr uint32_t kNone = 0xFFFFFFFFu;                         // above every cell value; as a cell index: no cell

struct Columns {
    const int64_t *s, *e, *a;
    uint64_t rows;
    int64_t head;    // rows before the first 16-byte pair (0 or 1)
    int64_t npairs;  // 16-byte pairs behind them
};

struct RowWindow {
    int64_t qs, s_end, e_hi;  // s_end = qs + L + CAP (a start at or past it is ignored), e_hi = qs + ident (an end at or past it is ident)
    uint32_t last, ident;     // last = L - 1
    void set(int64_t q, int64_t L, uint32_t cap) {
        ident = (uint32_t)(L - 1 + cap), last = (uint32_t)(L - 1);
        qs = q, s_end = q + L + (int64_t)cap, e_hi = q + (int64_t)ident;
    }
};

inline int check_columns(const int64_t *d_start, const int64_t *d_end, const int64_t *d_annot, uint64_t rows) {
    if ((reinterpret_cast<uintptr_t>(d_start) | reinterpret_cast<uintptr_t>(d_end) | reinterpret_cast<uintptr_t>(d_annot)) & 7)
        return fail(MEMO_EINVAL, "the row columns must be 8-byte aligned");
    if (rows && (!d_start || !d_end || !d_annot)) return fail(MEMO_EINVAL, "a row column is NULL");
    return MEMO_OK;
}

// the columns of a row pass: 16-byte loads when all three have the same alignment mod 16, else 8-byte loads.  Returns the grid.
inline unsigned set_columns(Columns &C, const int64_t *d_start, const int64_t *d_end, const int64_t *d_annot, uint64_t rows, bool &vec, int64_t most) {
    C.s = d_start, C.e = d_end, C.a = d_annot;
    C.rows = rows;
    const uintptr_t off = reinterpret_cast<uintptr_t>(d_start) & 15;
    vec = (reinterpret_cast<uintptr_t>(d_end) & 15) == off && (reinterpret_cast<uintptr_t>(d_annot) & 15) == off;
    C.head = vec && off ? 1 : 0;
    C.npairs = (int64_t)((rows - (uint64_t)C.head) / 2);
    const int64_t nchunks = (C.npairs + kPairsPerWg - 1) / kPairsPerWg;
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(nchunks, most));
}

// the cell (inside its plane) and value of a row that passes its caller's predicate; cell kNone: the row is ignored
__device__ __forceinline__ void row_bound(const RowWindow &W, bool pred, int64_t s, int64_t e, uint32_t &j, uint32_t &v) {
    j = kNone, v = kNone;
    if (!pred || s <= W.qs || s >= W.s_end) return;
    v = e <= W.qs ? 0u : e >= W.e_hi ? W.ident : (uint32_t)(e - W.qs);
    if (v >= W.ident) return;  // the identity
    const uint64_t d = (uint64_t)(s - W.qs - 1);
    j = d < W.last ? (uint32_t)d : W.last;
}

// every row of the columns to f, once: the pairs grid-strided in chunks of kPairsPerWg, a lane's two rows together (f.pair: whole
// waves call it, lanes without a pair with starts that no window takes), the rows outside the pairs (the first row of columns that
// start 8 bytes off a 16-byte line, the last odd row) by two lanes of workgroup 0, singly (f.one)
template <bool VEC, typename F>
__device__ __forceinline__ void stream_rows(const Columns &C, const F &f) {
    const int64_t nchunks = (C.npairs + kPairsPerWg - 1) / kPairsPerWg;
    for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const int64_t p0 = c * kPairsPerWg + threadIdx.x;
        longlong2 s[kLoads], e[kLoads], a[kLoads];
#pragma unroll
        for (int u = 0; u < kLoads; ++u) {
            const int64_t p = p0 + (int64_t)u * kRowThreads, r = C.head + 2 * p;
            // (a pair past the end: a start that no window takes)
            s[u] = e[u] = a[u] = make_longlong2(INT64_MIN, INT64_MIN);
            if (p < C.npairs) {
                if (VEC) {
                    s[u] = *reinterpret_cast<const longlong2 *>(C.s + r);
                    e[u] = *reinterpret_cast<const longlong2 *>(C.e + r);
                    a[u] = *reinterpret_cast<const longlong2 *>(C.a + r);
                } else {
                    s[u] = make_longlong2(C.s[r], C.s[r + 1]);
                    e[u] = make_longlong2(C.e[r], C.e[r + 1]);
                    a[u] = make_longlong2(C.a[r], C.a[r + 1]);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kLoads; ++u) f.pair(s[u], e[u], a[u]);
    }
    if (blockIdx.x == 0 && threadIdx.x < 2) {
        const uint64_t behind = (uint64_t)(C.head + 2 * C.npairs);
        const bool first = threadIdx.x == 0;
        if (first ? C.head == 1 : behind < C.rows) {
            const uint64_t r = first ? 0 : behind;
            f.one(C.s[r], C.e[r], C.a[r]);
        }
    }
}

}  // namespace memo

#endif  // MEMO_CELLS_H
