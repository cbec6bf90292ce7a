// memo_view.h -- the k-class views of an index's rows (internal): what memo_view_build.hip (HOW a view is made: kernels and the
// three passes) and memo_view.hip (WHEN one is made, and which rows a sweep reads) share with each other and with their callers.
#ifndef MEMO_VIEW_H
#define MEMO_VIEW_H

#include "memo_common.h"

namespace memo {

// ---- memo_view_build.hip -------------------------------------------------------------------------------------------------------
constexpr int kNoRoom = 1;  // (internal) the device has no memory for a view / tile table: run without it
// Device memory for what a query builds on the side (views, tile tables).  These are optimisations: when the device has no
// room for them the query runs on the rows it has (callers see kNoRoom, not an error).
hipError_t side_alloc(void **p, size_t bytes);
extern thread_local bool g_side_alloc_fails;  // (AB library, memo_debug_fail_side_allocations: every side_alloc fails -- the test of kNoRoom)

inline uint64_t dense_view_bytes(uint64_t padded, int rows_per_group) {  // what dense_view_build allocates for a view's rows
    return (rows_per_group == 6 ? padded / 6 + 64 : (padded + 4) / 5 + 64) * 16;
}
constexpr int kRunGroup = 8;  // buckets per group of a run copy: 256 positions, whose values begin at a multiple of four bytes
inline uint64_t run_view_bytes(uint64_t buckets, uint64_t value_bytes) {  // what run_view_copy allocates for a copy's table and values
    return buckets * 8 + value_bytes + 512;
}
// The passes: a source in, a BuiltView (memo_common.h) out.  Each allocates, queues its kernels on `st` and waits for them; kNoRoom when an allocation found no room.
// (hidden: they were file-local before the file was split, and the library exports what it exported)
#pragma GCC visibility push(hidden)
int dense_view_build(int device, const uint32_t *src_p3, const int64_t *src_boff, uint64_t rows, uint64_t nb, int cap, int min_tenths,
                     hipStream_t st, int rpg, int colour_km1, BuiltView &out);
int live_view_copy(int device, const BuiltView &flagged, uint64_t nb, hipStream_t st, BuiltView &out);
int deciding_view_copy(int device, const BuiltView &live, uint64_t nb, int64_t bbase, int64_t first_start, int64_t last_start, int km1,
                       hipStream_t st, BuiltView &out);
// (dec: a deciding copy of k - 1 = km1; out.p3: the run values, out.boff: mask | offset << 32 per bucket, out.rows: the runs, out.padded:
// the buckets; *first_bucket: the pivot bucket of the first, *value_bytes: of the values, every group's padded to dwords)
int run_view_copy(int device, const BuiltView &dec, uint64_t nb, int64_t bbase, int64_t first_start, int64_t last_start, int km1,
                  hipStream_t st, BuiltView &out, int64_t *first_bucket, uint64_t *value_bytes);
int packed_filter(int device, const uint32_t *src, const int64_t *src_boff, uint64_t rows, uint64_t nb, int cap, int min_tenths,
                  hipStream_t st, int len_shift, BuiltView &out);
#pragma GCC visibility pop

// ---- memo_view.hip -------------------------------------------------------------------------------------------------------------
// The rows a sweep reads: the index's own, or the k-class view of them that exists or was due -- and what the sweep's launcher has
// to know of it.  memo_index_info_t's last_rows_read / last_view_* are this value, written by the sweep that read it
// (note_dense_rows_read; the 4-byte words: use_words, memo_sweep.h).
struct RowSource {
    uint32_t *p3 = nullptr;  // dense groups (dense_rows_for) or 4-byte words (packed_rows_for)
    int64_t *boff = nullptr;
    uint64_t rows = 0;       // rows to read (six rows per group: slots -- the places a bucket leaves empty are read and swept like rows)
    int cap = 0;             // of the dense view handed out: its rows are exactly those with overlap < cap (0: no view, or words)
    int rpg = 5;             // rows per 16-byte group: 5, or 6 (a view whose groups carry their bucket)
    int placed = 0;          // the view's rows have their places chosen
    double dead_share = 0;   // ... the share of its groups flagged dead (the sweep skips them where it pays)
    float build_ms = 0.f;    // device time of the view's pass, when this call ran it (else 0)
    // the run copy of this k - 1, where one answers in the rows' place (run_tab != nullptr; memo_sweep_runs.hip decodes it):
    const uint32_t *run_vals = nullptr;  // a byte per run, 255: no row covers it
    const int64_t *run_tab = nullptr;    // per bucket: start mask | offset of its first value << 32
    int64_t run_b0 = 0;                  // the pivot bucket of the table's first entry
    uint64_t run_buckets = 0, runs = 0;
};
inline void note_dense_rows_read(memo_index *ix, const RowSource &src) {
    ix->last_rows_read = src.rows;
    ix->last_view_ms = src.build_ms;
    ix->last_view_placed = src.placed;
    ix->last_view_rpg = src.rpg;
}
// The dense rows a sweep with k - 1 = km1 should read: all of them, or a k-class view of them; window: the query's length (what a
// view would save this query decides when it is built); allow_six: the caller reads views of six rows per group too (src.rpg says
// which kind it got); account = false: a query's SECOND call (its six-row view found no tile table): hands back a five-row view
// that exists, adds nothing to the class's ledgers and builds nothing -- the query has been counted once already
int dense_rows_for(memo_index *ix, int km1, int64_t window, hipStream_t st, RowSource &src, bool allow_six = false, bool account = true);
// ... the 4-byte words: their k-class view (+ their order)
int packed_rows_for(memo_index *ix, int km1, int64_t window, bool membership, hipStream_t st, RowSource &src);
int dense_compact(memo_index *ix);  // leave the rows that can never write out of the dense rows (see memo_index::boff3)
// the views of one row source: the five- and six-row views of the dense rows, or the views of the 4-byte words
template <typename Index, typename F>
void each_view(Index *ix, bool dense, F f) {
    if (dense) {
        for (auto &v : ix->views) f(v);
        for (auto &v : ix->views6) f(v);
    } else {
        for (auto &v : ix->pviews) f(v);
    }
}
// The caller has the device drained: the views are freed, not retired.  The tile tables made for a dense view go with it, to the
// retire list: none where the dense rows go too (rows_changed drops every table first), and MEMO_OPT_VIEWS = 0 flushes the list.
void drop_dense_views(memo_index *ix);
void drop_packed_views(memo_index *ix);
void retire(memo_index *ix, void *p, uint64_t bytes);  // out of service now, freed once the device has drained
void flush_retired(memo_index *ix);                    // ... which the caller guarantees (it synchronised the device)
int order_words_now(memo_index *ix, int mode);  // waits for the device, orders ix->pk in place, waits again
// one pass: run on `st` between two events, the caller's stream waited for (later queries may come on other streams)
template <typename Build>
int build_timed(hipStream_t st, float *ms, Build build) {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    HIP_TRY(hipEventCreate(&e0));
    if (hipEventCreate(&e1) != hipSuccess) {
        (void)hipEventDestroy(e0);
        return fail(MEMO_EHIP, "hipEventCreate failed");
    }
    (void)hipEventRecord(e0, st);
    const int rc = build();
    (void)hipEventRecord(e1, st);
    (void)hipEventSynchronize(e1);
    (void)hipEventElapsedTime(ms, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return rc;
}
extern thread_local int g_six_views;  // (AB library, memo_debug_six_views: -1 the library's choice, 0 five rows per group always, 1 six wherever they apply)
extern thread_local int g_view_colouring;  // 1: the dense rows' k-class views may get their rows' places inside a group chosen against bank conflicts (memo_debug_view_colouring of the AB library turns it off)
extern thread_local bool g_dense_keep_all;  // (AB library, memo_debug_dense_keep_all: dense_compact keeps every row)

}  // namespace memo

#endif  // MEMO_VIEW_H
