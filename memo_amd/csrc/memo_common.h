// memo_common.h -- shared by the translation units of libmemo_amd.so (not part of the public ABI).
#ifndef MEMO_COMMON_H
#define MEMO_COMMON_H

#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "memo_amd.h"
#include "memo_amd_dap.h"
#include "memo_amd_multi.h"
#include "memo_amd_transport.h"

namespace memo {

// error plumbing: every C-ABI function returns fail(code, ...) on error; the message is what
// memo_last_error() hands out (thread-local, defined in memo_index.hip)
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

// device -> pageable host memory through the pinned ring of memo_hostpack.hip (DMA of piece i+1 under
// the worker threads' copy of piece i); work already queued on `producer` finishes first
int download_pipelined(int device, void *host, const void *dev, size_t bytes, hipStream_t producer);
int upload_pipelined(int device, void *dev, const void *host, size_t bytes);
// memo_dap.hip: the device and column count of a DAP handle (memo_ms_push_dap checks them)
void dap_shape(const memo_dap_t *h, int *device, int *columns);
// memo_ms.hip: piece `piece` of a genome given as records, as memo_ms_add_records assembles it on the device, copied to out
// (its n bytes and the kPad zeros behind them, when out_cap holds them); returns the number of pieces (memo_debug_ms_piece_text)
int ms_piece_text(memo_ms_t *h, const uint8_t *seq, const int64_t *rec_begin, int32_t nrec, int64_t piece_bytes, int32_t piece,
                  uint8_t *out, int64_t out_cap, int64_t *out_n);
// memo_ms.hip: >= 0: the allocations of this thread's later coded columns see this many bytes of free device memory instead of the
// device's (AB library, memo_debug_ms_free_bytes: the test of a column that does not fit)
extern thread_local int64_t g_ms_free_bytes;
// memo_compact.hip: exclusive scan of ntiles uint32 tile counts into int64 bases, their sum into *d_total (one workgroup; queued on st)
hipError_t scan_tile_counts(const uint32_t *d_counts, int64_t ntiles, int64_t *d_bases, int64_t *d_total, hipStream_t st);
// ... and d_out[pl] = the base of plane pl's first tile, d_out[planes] = the total: what the host reads of a compaction over planes
hipError_t plane_bases(const int64_t *d_bases, const int64_t *d_total, int64_t tiles_per_plane, int64_t planes, int64_t *d_out, hipStream_t st);
extern thread_local int g_cooc_flush;  // memo_cooc.hip (AB library, memo_debug_cooc_flush: 1 = atomics instead of partials)
extern thread_local int g_cooc_timed;  // ... memo_debug_cooc_times: event pairs around the launches of memo_cooccurrence_dev
extern thread_local float g_cooc_ms[2];
extern thread_local int g_maxk_rows_way;  // memo_maxk.hip (AB library, memo_debug_maxk_rows: 1 = one atomic per row instead of wave-aggregated ones)
extern thread_local int g_maxk_timed;     // ... memo_debug_maxk_times: event pairs around the launches of the memo_maxk_*_dev calls
extern thread_local float g_maxk_ms[5];
extern thread_local int g_collect_timed;  // memo_collect.hip (AB library, memo_debug_collect_times: event pairs around the launches of memo_collect_dev)
extern thread_local float g_collect_ms[2];
extern thread_local int g_panel_timed;  // memo_panel.hip (AB library, memo_debug_panel_times: event pairs around the launches of the memo_panel_*_dev calls)
extern thread_local float g_panel_ms[4];
extern thread_local int g_cover_timed;  // memo_cover.hip (AB library, memo_debug_cover_times: event pairs around the launches of the memo_cover_*_dev calls)
extern thread_local float g_cover_ms[4];
extern thread_local int g_tracks_timed;  // memo_tracks.hip (AB library, memo_debug_tracks_times: an event pair around the launch of memo_tracks_dev)
extern thread_local float g_tracks_ms;
extern thread_local int g_breaks_timed;  // memo_breaks.hip (AB library, memo_debug_breaks_times: an event pair around the launch of memo_breaks_dev)
extern thread_local float g_breaks_ms;
extern thread_local int g_pairs_timed;  // memo_pairs.hip (AB library, memo_debug_pairs_times: event pairs around the launches of memo_pairs_dev)
extern thread_local float g_pairs_ms[2];
extern thread_local int g_nearest_timed;  // memo_nearest.hip (AB library, memo_debug_nearest_times: an event pair around the launch of memo_nearest_dev)
extern thread_local float g_nearest_ms;
extern thread_local int g_nearest_lds_kib;  // ... memo_debug_nearest_lds: the LDS a workgroup may take, which decides the tile
constexpr int kNearestLdsKib = 72;          // ... the product's: two workgroups a CU
extern thread_local int g_mosaic_timed;  // memo_mosaic.hip (AB library, memo_debug_mosaic_times: event pairs around the launches of its two calls)
extern thread_local float g_mosaic_ms[5];
extern thread_local int g_mosaic_tile, g_mosaic_mark;  // ... memo_debug_mosaic_shape: the positions a tile of the parse, and which mark it takes
constexpr int kMosaicTile = 32768;                     // ... the product's
constexpr int kMosaicMark = 2;                         // ... 1 the serial lane, 2 the doubling mark
extern thread_local int g_features_timed;  // memo_features.hip (AB library, memo_debug_features_times: event pairs around the launches of its two calls)
extern thread_local float g_features_ms[3];
extern thread_local int g_lengths_timed;  // memo_lengths.hip (AB library, memo_debug_lengths_times: event pairs around the launches of the memo_lengths_*_dev calls)
extern thread_local float g_lengths_ms[7];
extern thread_local int g_mems_timed;  // memo_mems.hip (AB library, memo_debug_mems_times: event pairs around the launches of memo_mems_dev)
extern thread_local float g_mems_ms[3];
extern thread_local int g_spectrum_timed;  // memo_spectrum.hip (AB library, memo_debug_spectrum_times: bit 0 event pairs around the launches, bit 1 the global atomics counted)
extern thread_local float g_spectrum_ms[2];
extern thread_local int g_spectrum_private;
extern thread_local uint64_t g_spectrum_atomics;
double pinned_alloc_ms_total();  // memo_hostcore.cpp: time this process has spent allocating pinned staging slots (MEMO_TIMING)

struct DeviceGuard {  // the caller (e.g. torch) keeps its own notion of the current device
    int prev = -1;
    bool ok = false;
    explicit DeviceGuard(int dev) {
        if (dev < 0) return;  // (no device: nothing selected, nothing to restore)
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = (prev == dev) || (hipSetDevice(dev) == hipSuccess);
    }
    ~DeviceGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

// The one owner of one hipMalloc allocation: freed when it is reset or goes (the caller has the index's device selected), and read
// as the T * it holds, so that launch sites pass it as they passed the pointer.  Not an allocator and not a base class.
template <typename T>
struct DevPtr {
    T *p = nullptr;
    DevPtr() = default;
    DevPtr(DevPtr &&b) noexcept : p(b.release()) {}
    DevPtr &operator=(DevPtr &&b) noexcept { return adopt(b.release()), *this; }
    ~DevPtr() { reset(); }
    operator T *() const { return p; }
    hipError_t alloc(size_t n) { return reset(), hipMalloc(&p, n * sizeof(T)); }
    void reset() { adopt(nullptr); }
    void adopt(T *q) {  // q: from hipMalloc, owned by nobody else
        if (p) (void)hipFree(p);
        p = q;
    }
    T *release() {  // the caller owns it now (the retire list: memo_view.hip)
        T *q = p;
        p = nullptr;
        return q;
    }
};

constexpr uint64_t kPadRows = 4096;           // sentinel rows behind the last real row
constexpr int64_t kSentinel = INT64_MAX / 4;  // start/end of a padding row: clips to "empty"
constexpr int kDefaultBucketShift = 5;        // 32 pivot positions per bucket
constexpr int64_t kCoordLimit = (int64_t)1 << 61;
constexpr int kStatusBadAnnot = 1;            // sticky device flag: the reference's IndexError case
constexpr int kStatusHugeSlice = 2;           // sticky device flag: >= 2^32 rows reach one tile
constexpr int kStatusExecNarrow = 4;          // -DMEMO_EXEC_CHECK builds: a branch-free row block was entered with lanes disabled

// The one-time passes over an index's rows that one rule decides (memo_view.hip: pass_due): a k-class view of the dense rows, of the
// 4-byte words, a dense view with the places of its rows chosen, the copy of a placed six-row view without its dead groups, the
// query order of the 4-byte rows, the copy of a live copy that holds only the rows that decide a minimum at one k - 1, the run copy
// of a deciding copy (the results of that k - 1 themselves, run-coded; per position of its buckets)
enum Pass { kPassDenseView, kPassPackedView, kPassPlaces, kPassLiveCopy, kPassRowOrder, kPassDeciding, kPassRuns, kPasses };

// What a view pass (memo_view_build.hip) hands back, and the part of a DenseView it fills: the view's rows (dense groups, or 4-byte
// words), its bucket table (nb entries), the rows of the source it holds, the rows its table counts (slots of six-row groups; five-row
// groups and words: rows rounded up + kPadRows) and, of a six-row view with places, the groups flagged as holding no live row
// (memo_view_build.hip: kDeadGroup).  p3 == nullptr: nothing built (too few rows would go).
struct BuiltView {
    uint32_t *p3 = nullptr;
    int64_t *boff = nullptr;
    uint64_t rows = 0, padded = 0, dead_groups = 0;
};

}  // namespace memo

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t err__ = (expr);                                                             \
        if (err__ != hipSuccess)                                                               \
            return memo::fail(MEMO_EHIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(err__),    \
                              __FILE__, __LINE__);                                             \
    } while (0)

namespace memo {
// The event pair around the launches of a timed call of the AB library (the memo_debug_*_times switches): start() arms it, lap(i)
// waits for the launches since the last lap, puts their device time into ms[i] (add(i): adds it) and arms it again.  While `timed`
// is 0 -- the product never sets it -- it creates no event, records nothing and waits for nothing.
struct Laps {
    hipEvent_t e[2] = {};
    hipStream_t st;
    const int &timed;
    float *ms;
    Laps(hipStream_t s, const int &on, float *out) : st(s), timed(on), ms(out) {}
    Laps(const Laps &) = delete;
    ~Laps() {
        for (hipEvent_t x : e)
            if (x) (void)hipEventDestroy(x);
    }
    int start() {
        if (!timed) return MEMO_OK;
        for (hipEvent_t &x : e)
            if (!x) HIP_TRY(hipEventCreate(&x));
        HIP_TRY(hipEventRecord(e[0], st));
        return MEMO_OK;
    }
    int lap(int i, bool adding = false) {
        if (!timed) return MEMO_OK;
        float t = 0.f;
        HIP_TRY(hipEventRecord(e[1], st));
        HIP_TRY(hipEventSynchronize(e[1]));
        HIP_TRY(hipEventElapsedTime(&t, e[0], e[1]));
        ms[i] = adding ? ms[i] + t : t;
        HIP_TRY(hipEventRecord(e[0], st));
        return MEMO_OK;
    }
    int add(int i) { return lap(i, true); }
};
}  // namespace memo

// Kernel-shape choices of one index.  All zero in the product (= the library chooses per query);
// only libmemo_amd_ab.so (memo_debug.hip, include/memo_amd_debug.h) can set them, for A/B timing and
// for the tests that walk every tile shape.  Per index, so two threads on two indexes never share
// mutable state.  Results never depend on these.
struct memo_tuning {
    int tile_w = 0;      // positions per tile (256..4096); unclipped kernels: cells per level array
    int waves = 0;       // waves per tile: 1, 4 (8: unclipped conservation only)
    int memb_algo = 0;   // membership: 2 = doubling, 3 = runs, 4 = planes
    int force_wide = 0;  // 1 = read the int64 columns even when packed rows exist
    int scatter = 0;     // conservation, packed rows: 1 = clipped, 2 = unclipped + halo
    int persistent = 0;  // dense rows: 0 = the library's choice, 5 = the table-driven kernel (sweep_conservation_halo3t_kernel),
                         //   1 = every wave works its tile out by itself (sweep_conservation_halo3_kernel)
                         //   (the name is round 3's: 2 / 3 / 4 were persistent workgroups -- profiles/r03_persistent_sweep.txt: 17 - 50 % slower)
    int no_views = 0;    // dense rows: 1 = never read a k-class view (A/B)
    int no_all_write = 0;  // dense rows: 1 = the row blocks keep their "this row writes" test on a view of exactly the writing rows (A/B)
    int force_packed = 0;  // 1 = read the 4-byte rows even when the dense rows are resident and could answer (they are
                           //     the faster source for the conservation sweep: profiles/r02_dense_rows_ab.txt)
    int chain_off = 0;     // wide-tile sweep (memo_sweep_cons3t.hip: R4), parts of its shortened chain switched OFF (A/B): 1 = the entry with
                           //     the head in registers, 2 = a wave's two fold chunks in flight together, 4 = the store without the window
                           //     test in tiles off the window's edges, 8 = two tiles per workgroup behind one head
                           //     (sweep_conservation_wide_pair_kernel)
    int row_order = 0;     // order of the 4-byte rows inside a bucket (memo_interleave.hip): 0 = the library's (kRowOrderDefault),
                           //     1 = start order as packed, 2 = chunks of four dealt over the starts, 3 = the same with the rows of a
                           //     start ordered by overlap mod 32 (the conservation order), 4 = dealt over annot mod 32 (membership)
};

// one chromosome's rows, resident in HBM (the opaque memo_index_t of the ABI)
struct memo_index {
    int device = 0;
    memo_tuning tune;
    uint64_t rows = 0;
    uint64_t padded = 0;
    memo::DevPtr<int64_t> s, e, o;
    memo::DevPtr<int64_t> boff;  // boff[b] = first row with start >= (b << bshift); boff[nb-1] == rows
    uint64_t nb = 0;
    int bshift = 0;
    int64_t bbase = 0;        // boff[0] belongs to bucket `bbase` (a region slice imported from the CLI's cache; else 0)
    int64_t min_s = 0, max_s = -1;
    int finalized = 0;
    int was_sorted = 0;
    // packed rows (memo_index_pack): one word per row, layout by the largest annot (PackedRows, memo_sweep.h)
    memo::DevPtr<uint32_t> pk;
    memo::DevPtr<uint16_t> pa;  // format 6 only: 16-bit annot per row (the word's top byte is 0)
    int packed_fmt = 0;        // 0 = none, 4 = word with 8-bit annot, 12 = word with 12-bit annot and 12-bit start,
                               //   6 = word + 16-bit annot column
    uint64_t packed_rows = 0;  // rows the pk (pa) allocation holds (reused by the next memo_index_pack)
    int row_order = 0;         // how the 4-byte rows are ordered inside a bucket: 0 = by start (as packed), 1 / 2 = interleave_words modes
    // Rows that came in through memo_builder_* or memo_index_import_packed are in start order (or in whatever order their
    // file holds): an index that answers one query -- the one-shot forms, `memo query` -- should not pay a pass over its rows
    // for an order that spares a fraction of one sweep.  They are ordered once the queries that read them have lost to the
    // start order what the ordering pass costs (keep_row_order, memo_view.hip: the same ski-rental rule as the views), by
    // memo_index_prepare, or by memo_index_pack on the finished index.
    int order_pending = 0;
    double order_lost_ns = 0;    // what the queries so far would have saved on rows in the query order (estimate)
    int order_backoff = 1;       // (x 4 after an ordering that found no room for its second copy)
    float pack_ms = 0.f;       // device time of the last memo_index_pack (census + packing kernel)
    memo::DevPtr<uint32_t> p3;  // dense rows (memo_index_pack_dense): 16 bytes per 5 rows; annot <= 255 only
    // The dense rows may be FEWER than the index's rows: a row whose 6-bit length field is saturated (overlap >= 63, or
    // end < start) can never write at k <= 64 -- all the dense rows answer -- so when more than a tenth of the rows are
    // such rows they are left out (dense_compact, memo_view.hip: 40 % of the rows of an index built from sequences,
    // profiles/r03_realistic_index*.json; none of the synthetic one).  The dense stream then has its own row numbers and
    // its own bucket table; boff3 == nullptr: the dense rows are the index's rows, numbered alike (rows3 == rows).
    memo::DevPtr<int64_t> boff3;
    uint64_t rows3 = 0, padded3 = 0;
    // k-class views of the dense rows (dense_rows_for, memo_view.hip): the rows whose overlap is below 2 / 4 / ... / 32 -- all a
    // query with k - 1 <= 2 / 4 / ... / 32 can be touched by -- with their own bucket table; built by memo_index_prepare, or by the
    // query that finds that its class's queries have by now paid more for the rows a view would have spared them than the view costs
    // (view_due: ski rental), kept within the views' budget (memo_index_set_option: MEMO_OPT_VIEW_BUDGET_PCT)
    struct DenseView : memo::BuiltView {
        int cap = 0, state = 0;  // state: 0 not looked at yet, 1 built, 2 not worth it (it would spare less than a fifth)
        double lost_ns = 0;      // what this class's queries since it was last looked at would have saved with the view (estimate)
        int backoff = 1;         // the view is due when lost_ns reaches backoff x its estimated cost: x 4 after every eviction or failed
                                 //   allocation (a service that cycles through more classes than the budget holds must not rebuild all the time)
        int seen = 0;            // queries of the class since it was last looked at ...
        int ask_after = 0;       // ... of which this many must pass before it is looked at again: 0, then 16, 64 ... after evictions (what
                                 //   keeps the back-off alive when MEMO_OPT_BUILD_COST_PCT is 0 and every cost is nothing)
        int placed = 0;          // dense views: the rows' places inside their groups were chosen against LDS bank conflicts (memo_view_build.hip):
        double unplaced_ns = 0;  //   a second pass, decided like the first -- what the class's queries on the view as it is have lost to that
        int live = 0;            // 1: the copy of a placed six-row view without its dead groups (memo_view_build.hip: live_view_copy; dead_groups 0, padded = 6 x its
                                 //   groups, rows still the class's rows: a dead row is answered by a live one that contains it) --
        double dead_lost_ns = 0; //   a third pass, decided like the others: what the queries on the flagged view have lost to its dead groups
        // The DECIDING copy of a live copy (memo_view_build.hip: deciding_view_copy), kept beside it: for ONE k - 1 of the class (dec_km1)
        // the rows that hold the least (order, slot) at some position they cover -- the minimum over them is the minimum over all the
        // rows, at that k - 1 only (dec.rows: the winners, dec.padded: 6 x its groups; none of its groups is flagged, every row writes).
        // A fourth pass, decided in memo_view.hip (deciding_rows): the live copy must have answered kDecidingAskAfter queries in a row at
        // one k (dec_run at dec_run_km1) and the ledger dec_lost_ns must be due.
        memo::BuiltView dec;
        int dec_km1 = 0;           // the k - 1 `dec` is exact for (dec.p3 != nullptr)
        int dec_never[2] = {0, 0}; // [cap - km1]: the copy of this k - 1 spared less than a fifth of the groups (or could not be made): not asked for again
        int dec_run_km1 = 0, dec_run = 0;  // conservation queries in a row the class's live copy (or its deciding copy) has answered at this k - 1
        double dec_lost_ns = 0;    // what the queries of the run have lost to the rows that decide nothing (estimate)
        int dec_backoff = 1;       // x 4 after a pass that found no room
        uint64_t dec_bytes = 0;    // of dec's groups
        // The RUN copy of a deciding copy (memo_view_build.hip: run_view_copy), kept beside it under the same k - 1 (dec_km1): the minimum
        // itself, resolved once -- per bucket of 32 positions a mask of where a run of equal results starts and the offset of the bucket's
        // first value, and a byte per run (255: no row covers it).  run.p3: the values, run.boff: mask | offset << 32 per bucket, run.rows:
        // the runs, run.padded: the buckets (whole groups of 8), the first of which is bucket run_b0 of the pivot.  A fifth pass, decided in
        // memo_view.hip (run_rows): the deciding copy must have answered kRunsAskAfter queries in a row (run_answered) and the ledger
        // run_lost_ns must be due.  It goes wherever the deciding copy goes.
        memo::BuiltView run;
        int64_t run_b0 = 0;
        int run_answered = 0;      // conservation queries in a row the deciding copy of dec_run_km1 has answered
        double run_lost_ns = 0;    // what those queries have lost to sweeping where a decode would do (estimate)
        int run_backoff = 1;       // x 4 after a pass that found no room
        int run_never[2] = {0, 0}; // [cap - km1]: no run copy at this k - 1 (it could not be made)
        uint64_t run_bytes = 0;    // of run's values and table
        uint64_t bytes = 0;      // of the rows' allocation (set where a view is installed: a six-row view is (groups + 64) x 16 B, not
                                 //   what its padded row count makes of five-row groups -- ADVICE r05: the budget charged it a fifth too much)
        float build_ms = 0.f;
        uint64_t stamp = 0;      // last use (view_clock): past the views' budget the least recently used one goes
    };
    int views_on = 1;             // memo_index_set_option(MEMO_OPT_VIEWS)
    int view_budget_pct = 200;    // memo_index_set_option(MEMO_OPT_VIEW_BUDGET_PCT)
    int build_cost_pct = 100;     // memo_index_set_option(MEMO_OPT_BUILD_COST_PCT): a view / the ordering is due at this share of its cost
    int view_rows = 0;            // memo_index_set_option(MEMO_OPT_VIEW_ROWS): 0 the library's choice, 5 / 6 rows per group of a dense view
    int view_places = 1;          // memo_index_set_option(MEMO_OPT_VIEW_PLACES): 0 the rows of a dense view keep the order they come in
    uint64_t view_placings = 0;   // dense views rebuilt with their rows placed (memo_index_info_t.view_placings)
    int view_live = 1;            // memo_index_set_option(MEMO_OPT_VIEW_LIVE): 0 placed six-row views keep their dead groups (flagged, swept with LIVE)
    int wide_tiles = 1;           // memo_index_set_option(MEMO_OPT_WIDE_TILES): 0 six-row views keep the doubling tiles where R4 would apply (A/B)
    int view_deciding = 1;        // memo_index_set_option(MEMO_OPT_VIEW_DECIDING): 0 a live copy is never copied down to the rows that decide a minimum at the query's k
    uint64_t view_deciding_copies = 0;  // deciding copies made (memo_debug_view_deciding of the AB library)
    int view_runs = 1;            // memo_index_set_option(MEMO_OPT_VIEW_RUNS): 0 a deciding copy is never resolved into the run copy of its k (one already made stays, unread)
    uint64_t view_run_copies = 0; // run copies made (memo_debug_view_runs of the AB library)
    uint64_t view_live_copies = 0;  // placed six-row views copied without their dead groups (memo_debug_view_live_copies of the AB library)
    double pass_ns[memo::kPasses] = {};  // per row of its source, as the index's last pass of each kind measured it (memo::Pass; the copy without
                                         //   dead groups: per group of the flagged view; 0: the calibrated constant, memo_view.hip: kPassNs)
    uint64_t view_clock = 0;
    uint64_t view_builds = 0;     // views built over the index's lifetime (memo_index_info_t.view_builds)
    DenseView views[16];          // classes of two: overlaps below 2, 4, 6 ... 32
    DenseView views6[16];         // the same classes as groups of SIX rows that carry their bucket (memo_view_build.hip; what the table-driven sweep reads where it can)
    DenseView pviews[24];         // the same for the 4-byte words (caps 2 .. 32 by 2, .. 64 by 8, .. 128 by 16; `p3` holds words there): packed_rows_for
    uint64_t last_rows_read = 0;  // rows of the row source the last sweep read (info.last_rows_read)
    float last_view_ms = 0.f;     // device time of the view build, when the last sweep's view was built by it (else 0)
    int last_view_placed = 0, last_view_rpg = 5;  // (memo_index_info_t: of the dense rows the last sweep read)
    uint64_t max_annot = 0;    // largest annot of the packed rows
    // Sampled histogram of the packed rows' overlap field (min(end - start, 255)): with it the length n = k - 1 -
    // overlap of a row's interval is known in distribution for any k, which is what the choice between the level
    // arrays of the unclipped conservation sweeps turns on (memo_sweep_cons.hip, pick_levels).  Filled wherever
    // 4- / 6-byte rows come into being: memo_index_pack, memo_builder_finish, memo_index_import_packed.
    uint32_t len_hist[256] = {0};
    uint64_t len_hist_rows = 0;  // rows sampled (0: no histogram)
    // ... and which overlap values occur among ALL the rows (bit v of len_seen: some row has min(end - start, 255) == v), exact:
    // with it the lengths n = k - 1 - overlap that can occur at a k are known, hence which level arrays a sweep can skip
    uint32_t len_seen[8] = {0};
    int len_seen_exact = 0;
    // Tile tables of the table-driven dense-row sweep (memo_sweep_cons3t.hip): per (tile width, k) the row slice of every
    // tile of the chromosome, 32 bytes per tile, built by the first query that needs one and kept (least recently used of
    // four replaced); dropped with the dense rows.
    struct TileTable {
        const void *rows_of = nullptr;  // the dense rows (or view) the table was made for
        int w = 0, km1 = 0;
        void *d = nullptr;
        int64_t n = 0;
        uint64_t stamp = 0;
    };
    std::vector<TileTable> ttabs;  // one per (row source, tile width, k) in use, at most kMaxTileTables (least recently used out first)
    uint64_t ttab_clock = 0;
    // Device buffers a query took out of service (an evicted view, a tile table past the limit) while sweeps queued on any of
    // the caller's streams may still read them: they wait here -- no synchronisation on the query path -- and are freed by
    // the next call that has the device drained anyway (memo_query_check, memo_index_prepare, memo_index_pack*,
    // memo_index_destroy), or, past kRetiredLimit of the index's own bytes, by a query that then does wait for the device.
    struct Retired {
        void *p = nullptr;
        uint64_t bytes = 0;
    };
    std::vector<Retired> retired;
    uint64_t retired_bytes = 0;
    int last_sweep = 0;          // level arrays of the last conservation sweep (memo_index_info_t.last_sweep)
    int last_arrays = 0;         // mixed level arrays (last_sweep 4): how many of them the sweep's level plan allocated
    int last_variant = 0;        // ... 2 table-driven on five-row groups (memo_sweep_cons3t.hip), 3 on a view of six rows per group, 4 decoded from a run copy (memo_sweep_runs.hip); 0 no table
    int last_tiles_per_group = 1;  // tiles a workgroup of the last table-driven sweep did (2: the wide tiles' pair kernel; memo_debug_last_tiles_per_group)
    // what the plan step and the pickers of the last conservation sweep decided (memo_debug_last_pick of the AB library): the template
    // arguments of the kernel launched, as the picker's lambdas saw them.  All int32, in the order memo_amd_debug.h lists; host side
    // only: no kernel reads it.  family 0: none yet, or the fill of k <= 1 / an empty index.
    struct SweepPick {
        int32_t family = 0;     // last_sweep's numbering: 1 clipped, 2 doubling, 3 radix-4, 4 mixed, 5 the dense rows
        int32_t format = 0;     // 0 int64 columns, 4, 12, 6 the 4- / 6-byte rows, 3 the dense rows
        int32_t checked = 0;    // PackedRows' CHECKED (0 for the int64 columns and the dense rows)
        int32_t top = 0;        // TOP of the unclipped families on 4-byte rows: 24, 20 or 0
        int32_t threads = 0;    // per workgroup
        int32_t width = 0;      // clipped: W; unclipped: cells of a level array; table-driven: the tile width
        int32_t arrays = 0;     // level arrays in LDS
        int32_t out_bytes = 0;  // sizeof(OutT)
        int32_t nlev = 0, aw = 0, sp = 0, six = 0, live = 0, r4 = 0, chain = 0, pairs = 0, a9 = 0;  // the table-driven sweep's (launch_halo3t)
        int32_t halo3 = 0;      // 1: sweep_conservation_halo3_kernel (no table) answered
        int32_t kernel = 0;     // table-driven: 1 halo3t, 2 wide_args, 3 wide, 4 wide_pair; 5 the run copy's decode; else 0
    } last_pick;
    int last_tile_w = 0;         // ... and its tile width (info.last_tile_width: 1568 at k = 31 on the radix-4 arrays, 928 on the doubling ones)
    // the plan of the last membership sweep (memo_debug_last_membership of the AB library): the algorithm (2 doubling, 3 runs, 4 planes on the
    // 4- / 6-byte rows, 5 planes on the dense rows; 0 none yet, or the k <= 1 fill), the tile width, threads per tile, the row block's MW
    // (-1: a kernel without one), SK, result words per launch.  Host side only: no kernel reads it.
    int last_memb[6] = {0, 0, 0, -1, 0, 0};
    int has_wide = 1;          // the three int64 columns are still resident
    // rows with end < start (never written by the reference's index builder, but legal input to
    // memo_query.py): copied aside at finalize and applied by long_rows_kernel after each sweep
    struct LongRows {
        memo::DevPtr<int64_t> cols;  // one allocation of [3 n]: the starts, the ends, the annots
        uint64_t n = 0;
        const int64_t *s() const { return cols; }
        const int64_t *e() const { return cols + n; }
        const int64_t *o() const { return cols + 2 * n; }
        hipError_t set(const int64_t *host, uint64_t rows, hipStream_t st);  // from host columns [3 rows] (read until st has been waited for)
        int collect(const memo_index *ix, uint64_t found, hipStream_t st);  // the `found` such rows of ix's int64 columns (memo_index_finalize); waits for st
        int download(int device, int64_t *host) const;                      // to the [3 n] layout of the exports
    } long_rows;
    // memo_multi.hip (resident form) sweeps a SUB-window of the caller's window on this index.  A row with end < start
    // can reach any distance left of its start, so it has to pass the reference's filter (memo_query.py:25-27) on the
    // WHOLE window, not on the sub-window: while whole_set, the long-row kernels filter by [whole_qs, whole_qe).
    int64_t whole_qs = 0, whole_qe = 0;
    int whole_set = 0;
    memo::DevPtr<int> d_status;  // sticky flags set by the sweep kernels
    memo::DevPtr<uint64_t> d_scratch;  // finalize(): [0] unsorted pairs, [1] rows with end < start
};

namespace memo {
// (the k-class views' own declarations: memo_view.h)
// What derives from what in an index, in this order: the 4-byte words (+ annot column) are made from the int64 columns and the
// bucket table, the dense rows (+ their own table) from the words, and of each of the two a query makes k-class views, of the dense
// rows and their views tile tables.  rows_changed (memo_index.hip) is the one place that says what a change at a level makes stale:
// everything BELOW it goes, and the state words that describe it are reset -- kLevelColumns: the rows themselves (finalized = 0; the
// words, packed_fmt = 0, packed_rows = 0; and on); kLevelWords: the words are about to be rewritten (the dense rows, rows3 = padded3
// = 0, every view and tile table; packed_fmt = 0); kLevelDense: the dense rows are replaced (their views, every tile table; the
// words and their views stay); kLevelDerived: every view, with the tile tables made for it.  keep_word_buffers: the pk / pa
// allocations and packed_rows stay for the next memo_index_pack.  The caller has the index's device selected.
enum Level { kLevelColumns, kLevelWords, kLevelDense, kLevelDerived };
void rows_changed(memo_index *ix, Level at, bool keep_word_buffers = false);
int need_wide(const memo_index *ix);  // MEMO_OK, or the refusal of an index whose int64 columns memo_index_pack dropped
int device_ok(int device);            // MEMO_OK, or the refusal of a device number that is not among the visible ones
// How an entry point gets onto its device: the device_ok refusal first (kSelectOnly: not made -- the entry points that never made it),
// then the selection, and the caller's device again when it goes.  rc != MEMO_OK: return it.
struct OnDevice {
    static constexpr bool kSelectOnly = true;
    int rc;
    DeviceGuard guard;
    explicit OnDevice(int dev, bool select_only = false) : rc(select_only ? MEMO_OK : device_ok(dev)), guard(rc ? -1 : dev) {
        if (!rc && !guard.ok) rc = fail(MEMO_EHIP, "cannot select HIP device %d", dev);
    }
};
inline uint64_t padded_for(uint64_t rows) { return ((rows + 15) & ~(uint64_t)15) + kPadRows; }
// The one birth of an index (memo_index.hip): an empty one of `rows` rows on a checked device, with its status and scratch words; the
// status word's clear is queued on st (the builder's ring stream, which it waits for with its copies), st == nullptr: done on return
int new_index(uint64_t rows, int device, hipStream_t st, memo_index **out);
// memo_cells.hip: the passes over planes of uint32 cells [planes][pitch], L of them a plane, that memo_maxk.hip (one plane: the pitch
// is never used) and memo_lengths.hip share.  The refusals both make, in the two groups in which both make them; the fill of [0, L) of
// every plane with the identity L - 1 + cap, on at most `most` workgroups a plane; the carries (int64 [planes], INT64_MAX: none) into
// cell L - 1; and the finish in place -- tile minima into d_mins [planes x cell_tiles(L)], their suffix-min scan, apply -- whose three
// launches are laps slot, slot + 1, slot + 2 of the caller's timer.  All queued on st; none waits for it outside a timed call.
constexpr int kCellTile = 2048;
inline int64_t cell_tiles(int64_t L) { return (L + kCellTile - 1) / kCellTile; }
struct CellPlanes {
    uint32_t *cells;
    int64_t L, pitch;
    int planes;
    uint32_t cap;
    uint32_t ident() const { return (uint32_t)(L - 1 + cap); }
};
int check_window(int64_t L, uint32_t cap);
int check_cell_pointer(const uint32_t *d_cells, int64_t L);
hipError_t cells_fill(const CellPlanes &P, int64_t most, hipStream_t st);
hipError_t cells_carry_in(const CellPlanes &P, const int64_t *d_carry, int64_t qs, hipStream_t st);
int cells_finish(const CellPlanes &P, uint32_t *d_mins, hipStream_t st, Laps &laps, int slot);
constexpr size_t kMaxTileTables = 64;
int builder_why(const memo_builder_t *b);  // memo_hostpack.hip: which rows a builder refused with MEMO_EUNPACKABLE (BlockResult::bad bits)
extern thread_local int g_one_shot_way;     // memo_oneshot.hip (AB library, memo_debug_one_shot_way: 1 = int64 columns, 2 = 4-byte words)
extern thread_local bool g_prepare_only;  // memo_sweep.hip; memo_index_prepare: the query path builds what it would build and launches nothing
// ... and hands this as the result pointer: a launch site that missed g_prepare_only refuses it instead of writing to it (launch_tiles,
// launch_halo3t, the fill and long-row launches: memo_sweep.hip: refuse_plan_pointer)
static void *const kNeverWritten = reinterpret_cast<void *>(uintptr_t(4096));
int refuse_plan_pointer(const void *d_out);
inline uint64_t dense_groups_for(uint64_t padded) { return (padded + 4) / 5 + 64; }  // (+ one wave-load of slack: a wave reads its 64 groups whole)
void drop_tile_tables(memo_index *ix);  // memo_sweep_cons3t.hip: the tables derive from the dense rows and the bucket table
// memo_interleave.hip: reorder the 4-byte rows inside every bucket (mode 0: start order, 1: chunks of four dealt round-robin
// over the bucket's starts, 2: the same with the rows of a start ordered by overlap mod 32), in place, queued on st
int interleave_words(uint32_t *words, const int64_t *boff, uint64_t nb, int bshift, int fmt, int mode, hipStream_t st, uint64_t *scratch);  // scratch: ix->d_scratch
constexpr int kRowOrderDefault = 2;  // interleave_words mode the product applies wherever 4-byte rows come into being
inline int row_order_mode(const memo_index *ix) { return ix->tune.row_order ? ix->tune.row_order - 1 : kRowOrderDefault; }
extern thread_local int g_last_one_shot_sweep;  // memo_oneshot.hip: which kernel family answered this thread's last one-shot call
}

// fills ix->len_hist from the resident 4- / 6-byte rows (a few thousand 1024-row blocks, evenly spread); NULL stream, synchronous
int memo_len_census(memo_index *ix);

#endif  // MEMO_COMMON_H
