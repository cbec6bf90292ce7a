// memo_view.hip -- k-class VIEWS of an index's rows: which classes there are, and the rule that decides when one is built.
//
// The reference (memo_query.py:45-49) recentres the rows, casts the shadow and DROPS the rows that cannot write at the
// query's k -- per query.  A resident index does the dropping once per k class: a view holds the rows whose overlap is below
// the class's cap (all a query with k - 1 <= cap can be touched by), with a bucket table of its own.  memo_view_build.hip makes
// the views (its three passes); this file says which rows a sweep reads (dense_rows_for, packed_rows_for), keeps the views within
// their memory budget, and decides WHEN a view (or the query order of the 4-byte rows) is worth its pass: the ski-rental rule of
// view_due() below.
#include "memo_view.h"

using namespace memo;

namespace memo {
// A/B switches of the AB library (memo_debug.hip sets them; per thread)
thread_local bool g_dense_keep_all = false;  // memo_debug_dense_keep_all: dense_compact keeps every row
thread_local int g_view_colouring = 1;       // memo_debug_view_colouring: 0 = no view gets the places of its rows chosen
thread_local int g_six_views = -1;           // memo_debug_six_views: -1 the library's choice, 0 five rows per group always, 1 six wherever they apply

// ix->p3 holds every row of the index (rows3 == rows, no boff3).  When more than a tenth of them can never write at
// k <= 64 (6-bit length field saturated), rebuild the dense rows without them, with a bucket table of their own.
int dense_compact(memo_index *ix) {
    if (!ix->p3 || ix->boff3 || !ix->rows || g_dense_keep_all) return MEMO_OK;
    BuiltView b;
    int rc = dense_view_build(ix->device, ix->p3, ix->boff, ix->rows, ix->nb, 63, 1, nullptr, 5, 0, b);
    if (rc == kNoRoom) rc = MEMO_OK;  // (no room for a second copy: every row stays)
    if (rc || !b.p3) return rc;
    DeviceGuard guard(ix->device);
    rows_changed(ix, kLevelDense);  // (the rows in full go; nothing can have been made of them yet)
    ix->p3.adopt(b.p3);
    ix->boff3.adopt(b.boff);
    ix->rows3 = b.rows;
    ix->padded3 = b.padded;
    return MEMO_OK;
}

void retire(memo_index *ix, void *p, uint64_t bytes) {
    if (!p) return;
    memo_index::Retired r;
    r.p = p;
    r.bytes = bytes;
    ix->retired.push_back(r);
    ix->retired_bytes += bytes;
}

void flush_retired(memo_index *ix) {
    for (memo_index::Retired &r : ix->retired) (void)hipFree(r.p);
    ix->retired.clear();
    ix->retired_bytes = 0;
}

// The back-off of a pass that found no room or whose view was evicted (DenseView::backoff, memo_index::order_backoff): x 4, up to
// 2^16; and the queries that must pass before an evicted class is looked at again (DenseView::ask_after): 0, 16, then x 4 alike.
static int backoff_step(int x) { return x < (1 << 16) ? x * 4 : x; }
static int ask_after_step(int x) { return x ? backoff_step(x) : 16; }

// evicted: by the budget -- the class starts again, later (back-off: see DenseView); else the view is being replaced by another of
// the same class (its places, its live copy, a new row order), which is as due as it was
// the tile tables made for a view go with it (a later allocation may land on its address)
static void retire_tables_of(memo_index *ix, const memo_index::DenseView &v) {
    for (size_t i = 0; i < ix->ttabs.size();) {
        if (ix->ttabs[i].rows_of == v.p3 || (v.dec.p3 && ix->ttabs[i].rows_of == v.dec.p3)) {  // (never of a view that was not built: a table is made for rows)
            retire(ix, ix->ttabs[i].d, (uint64_t)ix->ttabs[i].n * 32);
            ix->ttabs.erase(ix->ttabs.begin() + (long)i);
        } else {
            ++i;
        }
    }
}

// the run copy of a deciding copy, out of service; its count and ledger start again
static void retire_runs(memo_index *ix, memo_index::DenseView &v) {
    if (v.run.p3) {
        retire(ix, v.run.p3, v.run_bytes - v.run.padded * 8);
        retire(ix, v.run.boff, v.run.padded * 8);
    }
    v.run = BuiltView();
    v.run_bytes = 0;
    v.run_answered = 0;
    v.run_lost_ns = 0;
}

// the deciding copy of a live copy, out of service: with the tile tables made for it; the class's ledgers for it start again
static void retire_deciding(memo_index *ix, memo_index::DenseView &v) {
    retire_runs(ix, v);  // (it is the deciding copy's k - 1 resolved: it goes where that goes)
    if (!v.dec.p3) return;
    for (size_t i = 0; i < ix->ttabs.size();) {
        if (ix->ttabs[i].rows_of == v.dec.p3) {
            retire(ix, ix->ttabs[i].d, (uint64_t)ix->ttabs[i].n * 32);
            ix->ttabs.erase(ix->ttabs.begin() + (long)i);
        } else {
            ++i;
        }
    }
    retire(ix, v.dec.p3, v.dec_bytes);
    retire(ix, v.dec.boff, ix->nb * 8);
    v.dec = BuiltView();
    v.dec_km1 = 0;
    v.dec_bytes = 0;
}

static void retire_view(memo_index *ix, memo_index::DenseView &v, bool evicted) {
    retire_tables_of(ix, v);
    retire_runs(ix, v);
    retire(ix, v.p3, v.bytes);
    retire(ix, v.dec.p3, v.dec_bytes);  // (the deciding copy goes with the live copy it was made of)
    if (v.dec.p3) retire(ix, v.dec.boff, ix->nb * 8);
    retire(ix, v.boff, ix->nb * 8);
    const int backoff = evicted ? backoff_step(v.backoff) : v.backoff, ask = evicted ? ask_after_step(v.ask_after) : v.ask_after;
    v = memo_index::DenseView();
    v.backoff = backoff;
    v.ask_after = ask;
}

static void free_view(memo_index::DenseView &v) {  // (the caller has the device drained)
    (void)hipFree(v.p3);
    (void)hipFree(v.boff);
    (void)hipFree(v.dec.p3);
    (void)hipFree(v.dec.boff);
    (void)hipFree(v.run.p3);
    (void)hipFree(v.run.boff);
    v = memo_index::DenseView();
}
void drop_dense_views(memo_index *ix) {
    each_view(ix, true, [&](memo_index::DenseView &v) {
        retire_tables_of(ix, v);
        free_view(v);
    });
}
void drop_packed_views(memo_index *ix) { each_view(ix, false, free_view); }

// All the views of one row source together may take view_budget_pct percent (200 by default: memo_index_set_option) of the bytes
// of the rows they are views of (sixteen classes of the dense rows would come to 4.5 times on BASELINE's generator); past that
// the least recently used view is RETIRED -- with the tile tables made for it -- and its class starts from nothing again,
// towards a threshold four times the last one (a service that cycles through more classes than the budget holds settles on
// the classes that fit and reads all the rows for the others, instead of rebuilding a view every few queries: ADVICE r03).
// Nothing is waited for here: a sweep queued on any of the caller's streams may still read the view, so its buffers go to
// the index's retire list (memo_common.h) -- unless that list has itself grown past the budget: then the device is drained.
static void keep_views_in_budget(memo_index *ix, const memo_index::DenseView *fresh, uint64_t base_bytes, bool dense) {
    const uint64_t budget = base_bytes / 100 * (uint64_t)ix->view_budget_pct;
    for (;;) {  // (the five- and six-row views of the dense rows share one budget)
        uint64_t total = 0;
        memo_index::DenseView *lru = nullptr;
        each_view(ix, dense, [&](memo_index::DenseView &v) {
            if (!v.p3) return;
            total += v.bytes + ix->nb * 8 + (v.dec.p3 ? v.dec_bytes + ix->nb * 8 : 0) + v.run_bytes;
            if (&v != fresh && (!lru || v.stamp < lru->stamp)) lru = &v;
        });
        if (total <= budget || !lru) break;
        retire_view(ix, *lru, true);
    }
    if (ix->retired_bytes > budget + base_bytes) {  // (rare: many evictions and no memo_query_check in between)
        (void)hipDeviceSynchronize();
        flush_retired(ix);
    }
}

// ---- when is a pass over the rows worth it? ---------------------------------------------------------------------------------
// memo_query.py:45-49 drops the rows that cannot write at the query's k in every query; a view drops them once -- at the price
// of a pass over the rows.  Rounds 3-4 paid that price inside the fifth query of a class, whatever the queries were: on BASELINE
// config 3 a view paid for itself after 65 whole-chromosome queries, so queries 5 .. 69 of a class were a net loss, and a host
// that sweeps 1-Mbp windows paid 8 ms for a view that saves it a microsecond per query.  Now every query of a
// class that runs without its view adds what the view would have saved it -- the rows of its window the view leaves out x
// what a sweep pays per row -- and the view is built by the query that finds the sum has reached the view's estimated cost:
// the ski-rental rule (never more than twice the cost of having known the future).  memo_index_prepare builds at once;
// MEMO_OPT_BUILD_COST_PCT scales the threshold (0: the class's first query builds).  The same rule decides when rows that
// came in start order are brought into the query order (keep_row_order).
// Calibration (MI355X, profiles/r05_view_pass.txt): a sweep's time per row it reads; a pass's time per row of its source --
// replaced by what the index's own last pass measured -- plus what allocations and the two waits cost whatever the size.
constexpr double kSweepNsPerRow = 0.00048;      // config 3, k = 31: (0.298 - 0.179 ms) / 2.5e8 rows a view spares
constexpr double kDenseViewNsPerRow = 0.0036;   // count + scan + the fused pass, rows in the order they come (2.0 ms for config 3's 5e8 rows)
constexpr double kPlacedViewNsPerRow = 0.0078;  // ... with the places of the rows chosen (4.1 ms)
constexpr double kPlacedGainPerKm1 = 0.0013;    // what places buy a sweep on the view: 4.4 % at k = 31, 2 % at k = 21 (profiles/r04_view_levels.txt)
constexpr double kPackedViewNsPerRow = 0.03;    // keep, scan, scatter, and the order inside the view's buckets
constexpr double kOrderNsPerRow = 0.014;        // copy + the order inside the buckets (more on indexes of many rows per start)
constexpr double kLiveCopyNsPerGroup = 0.008;   // live_view_copy, per group of the flagged view: two reads of it, a write of its live groups
constexpr double kDecidingNsPerGroup = 0.12;    // deciding_view_copy, per group of the live copy (profiles/deciding_rows.txt: 1.62 ms for config 3's 1.14e7 groups at k = 31)
constexpr double kDecidingSparedShare = 0.5;    // ... the share of the live copy's slots a deciding copy is assumed to spare a sweep, before one is made
constexpr int kDecidingAskAfter = 32;           // ... queries in a row at one k the live copy must have answered first (bench.py's warm-up makes 200: <= 64)
constexpr double kRunsNsPerPosition = 0.011;    // run_view_copy, per position of the copy's buckets (profiles/run_copy.txt: 1.3 ms for config 3's 10^8 positions at k = 31)
constexpr double kDecodeSparedNsPerPosition = 0.00013;  // ... what a decode spares a sweep of the deciding copy, per position of the window (62.7 -> 49.3 us for 10^8 at k = 31; 67.7 -> 50.7 at k = 17)
constexpr int kRunsAskAfter = 32;               // ... queries in a row the deciding copy must have answered first (above the 15 tests/test_deciding_rows_gpu.py asks of one)
constexpr double kPassFixedNs = 200e3;
// per unit of every pass (Pass, memo_common.h: a row of its source; the live copy: a group of the flagged view), until the index has measured one
constexpr double kPassNs[kPasses] = {kDenseViewNsPerRow, kPackedViewNsPerRow, kPlacedViewNsPerRow, kLiveCopyNsPerGroup, kOrderNsPerRow, kDecidingNsPerGroup, kRunsNsPerPosition};

static double rows_in_window(const memo_index *ix, double src_rows, int64_t window, int km1) {
    const double span = (double)ix->max_s - (double)ix->min_s + 1.0;
    const double w = (double)window + (double)km1 + (double)((int64_t)1 << ix->bshift);
    return span <= w ? src_rows : src_rows * w / span;
}

// the share of the index's rows whose overlap is below cap, from the census taken when the rows came into being (a sample;
// 0.5 where there is none)
static double share_below(const memo_index *ix, int cap) {
    if (!ix->len_hist_rows) return 0.5;
    double below = 0;
    for (int v = 0; v < cap && v < 256; ++v) below += ix->len_hist[v];
    return below / (double)ix->len_hist_rows;
}

// The rule: a pass over `units` rows (groups) is due when its ledger -- what the queries so far have lost to its absence -- has
// reached its estimated cost, `backoff` times over.  What a query adds to a ledger is its caller's estimate (below).
static bool pass_due(const memo_index *ix, double lost_ns, int backoff, Pass pass, double units) {
    const double per_unit = ix->pass_ns[pass] > 0 ? ix->pass_ns[pass] : kPassNs[pass];
    return lost_ns >= (units * per_unit + kPassFixedNs) * (double)backoff * (double)ix->build_cost_pct / 100.0;
}

static void pass_measured(memo_index *ix, Pass pass, float ms, double units) {  // what the pass cost, for the next estimate
    const double ns = (double)ms * 1e6 - kPassFixedNs;
    // within a factor of four of the calibrated constant: the pass is timed with its allocations, and a hipMalloc that stalls (350 ms
    // for 0.85 GB seen on one box: gpurun r5valid) must not make every later view of the index look two hundred times as dear
    const double floor = 0.25 * kPassNs[pass], ceil = 4.0 * kPassNs[pass];
    if (units > 0) ix->pass_ns[pass] = ns / units > floor ? (ns / units < ceil ? ns / units : ceil) : floor;
}

// A class without its view (pass: kPassDenseView or kPassPackedView).  spared: the share of src_rows the view would leave out.
static bool view_due(memo_index *ix, memo_index::DenseView &v, Pass pass, double src_rows, double spared, int64_t window, int km1) {
    if (g_prepare_only) return true;
    if (spared > 0) v.lost_ns += rows_in_window(ix, src_rows, window, km1) * spared * kSweepNsPerRow;
    if (++v.seen <= v.ask_after) return false;
    return pass_due(ix, v.lost_ns, v.backoff, pass, src_rows);
}

// A dense view that exists with its rows in the order they came: is it time to build it again with their places chosen
// (memo_view_build.hip: view_place_bucket)?  The places buy a sweep a few percent; the pass that chooses them costs twice the pass
// without -- so a class gets its view when the view has paid for itself (view_due), and the places when THEY have.
static bool places_due(memo_index *ix, memo_index::DenseView &v, double src_rows, int64_t window, int km1, bool six) {
    if (g_prepare_only) return true;
    const double read = rows_in_window(ix, (double)(six ? v.padded : v.rows), window, km1);
    v.unplaced_ns += read * 1.5 * kSweepNsPerRow * kPlacedGainPerKm1 * (double)km1;  // (a sweep on a view: 0.72 ps per row it reads)
    return pass_due(ix, v.unplaced_ns, v.backoff, kPassPlaces, src_rows);
}

// A placed six-row view whose dead groups are flagged: is it time for the copy without them (live_view_copy)?  The sweep on the
// flagged view loads every group, so a query loses the slots of its window in dead groups x what a sweep pays per row it reads;
// the copy costs a read of the view.  The same rule again -- and never inside memo_index_prepare, which hands out the flagged view
// (a whole-window query on config 3 loses ~0.09 ms against a pass of ~0.5 ms: a few such queries build it).
static bool live_due(memo_index *ix, memo_index::DenseView &v, int64_t window, int km1) {
    if (g_prepare_only || v.padded < 6) return false;
    const double groups = (double)(v.padded / 6), share = (double)v.dead_groups / groups;
    v.dead_lost_ns += rows_in_window(ix, (double)v.padded, window, km1) * share * kSweepNsPerRow;
    return pass_due(ix, v.dead_lost_ns, v.backoff, kPassLiveCopy, groups);
}

// A live copy that answers a conservation query at k - 1 = km1: the deciding copy of that k - 1 (memo_view_build.hip: deciding_view_copy)
// in its place, when it exists or is due.  The copy is exact for ONE k - 1, so the library wants evidence that the host stays at this
// k before it pays the pass: the live copy (or the deciding copy of this k - 1) must have answered kDecidingAskAfter queries in a
// row at it -- a query of the class at its other k starts the run again, and this holds at MEMO_OPT_BUILD_COST_PCT 0 too -- and
// the ledger of the run (the slots of the window x an assumed spared share x what a sweep pays per row) must have reached the pass's
// cost.  Never inside memo_index_prepare.  One deciding copy per class: a copy for the class's other k - 1 stays until this one's
// is made, and answers again without a pass when the host goes back.  A copy that spares less than a fifth of the groups is
// dropped and this k - 1 not looked at again (the precedent of state 2); no room: the live copy answers and the back-off grows.
// src: the live copy's, rewritten for the deciding copy -- every row of which writes at km1 (cap = km1: the launcher drops the test).
static int deciding_rows(memo_index *ix, memo_index::DenseView &v, int km1, int64_t window, hipStream_t st, uint64_t base_bytes,
                         RowSource &src) {
    if (!ix->view_deciding || km1 > v.cap || km1 < v.cap - 1 || km1 > 31) return MEMO_OK;
    auto hand_out = [&]() {
        src.p3 = v.dec.p3;
        src.boff = v.dec.boff;
        src.rows = v.dec.padded;
        src.cap = km1;
        src.dead_share = 0.0;
    };
    if (g_prepare_only) {  // (plans on what there is; counts nothing, builds nothing)
        if (v.dec.p3 && v.dec_km1 == km1) hand_out();
        return MEMO_OK;
    }
    if (v.dec_run_km1 != km1) {
        v.dec_run_km1 = km1;
        v.dec_run = 0;
        v.dec_lost_ns = 0;
        v.run_answered = 0;  // (run_rows: its count is of this run)
        v.run_lost_ns = 0;
    }
    const int answered = v.dec_run++;  // queries of this run before this one
    // (the run copy's ledger, run_rows: every query of the run loses at least what a decode spares a sweep of the deciding copy)
    if (ix->view_runs && !v.run.p3) v.run_lost_ns += (double)window * kDecodeSparedNsPerPosition;
    if (v.dec.p3 && v.dec_km1 == km1) {
        hand_out();
        return MEMO_OK;
    }
    if (v.dec_never[v.cap - km1] || v.padded < 6) return MEMO_OK;
    v.dec_lost_ns += rows_in_window(ix, (double)v.padded, window, km1) * kDecidingSparedShare * kSweepNsPerRow;
    const double groups = (double)(v.padded / 6);
    if (answered < kDecidingAskAfter || !pass_due(ix, v.dec_lost_ns, v.dec_backoff, kPassDeciding, groups)) return MEMO_OK;
    DeviceGuard guard(ix->device);
    BuiltView b;
    float ms = 0.f;
    const int rc = build_timed(st, &ms, [&]() {
        return deciding_view_copy(ix->device, v, ix->nb, ix->bbase, ix->min_s, ix->max_s, km1, st, b);
    });
    if (rc && rc != kNoRoom) return rc;
    v.dec_lost_ns = 0;
    if (rc == kNoRoom) {  // (the pressure may pass: the run goes on, the threshold is four times as far)
        v.dec_backoff = backoff_step(v.dec_backoff);
        return MEMO_OK;
    }
    pass_measured(ix, kPassDeciding, ms, groups);
    if (!b.p3 || b.padded * 5 > v.padded * 4) {  // gave up, or spares less than a fifth: nobody has read it (the pass waited for st)
        (void)hipFree(b.p3);
        (void)hipFree(b.boff);
        v.dec_never[v.cap - km1] = 1;
        return MEMO_OK;
    }
    const double run_lost_ns = v.run_lost_ns;
    retire_deciding(ix, v);  // (the class's other k - 1: sweeps queued on other streams may still read it)
    v.run_lost_ns = run_lost_ns;  // (of this run: it goes on)
    v.dec = b;
    v.dec_km1 = km1;
    v.dec_bytes = dense_view_bytes(b.padded, 6);
    ++ix->view_deciding_copies;
    src.build_ms = ms;
    hand_out();
    keep_views_in_budget(ix, &v, base_bytes, true);
    return MEMO_OK;
}

// A deciding copy that answers a conservation query at its k - 1 = km1 (src: as deciding_rows left it): the RUN copy of that k - 1
// (memo_view_build.hip: run_view_copy) in its place, when it exists or is due -- the sweep's launcher then decodes results instead of
// sweeping rows (src.run_tab; memo_sweep_runs.hip).  Every row of the deciding copy wins somewhere, but the rows still overlap, and a
// sweep learns again with every query which of them wins where; for one k that never changes.  The same bargain as the deciding copy's,
// under the same two conditions: the deciding copy must have answered kRunsAskAfter queries in a row at this k - 1 (a query at the class's
// other k starts the count again, and so does memo_index_set_option with an option that changes which rows or which kernel answer
// -- all but the budget and the cost share: a host that switches those between its queries, as every A/B of the sweep kernels does, has
// not settled; at MEMO_OPT_BUILD_COST_PCT 0 too) and the ledger -- the window's positions x what a decode spares a
// sweep per position, over every query of the run at this k - 1 (deciding_rows adds it: the queries the live copy answered lost no
// less) -- must have reached the pass's cost.  Never inside memo_index_prepare; only where every order is below 255 (the
// byte that says "no row").  One per class, retired with its deciding copy; no room: the deciding copy answers and the back-off grows;
// a copy of half a value per position or more (its bytes come to three quarters of the result's: the decode was never measured there) is
// dropped and this k - 1 not looked at again.
static int run_rows(memo_index *ix, memo_index::DenseView &v, int km1, int64_t window, hipStream_t st, uint64_t base_bytes, RowSource &src) {
    if (!ix->view_runs || ix->max_annot > 254 || !v.dec.p3 || v.dec_km1 != km1 || src.p3 != v.dec.p3) return MEMO_OK;
    auto hand_out = [&]() {
        src.run_vals = v.run.p3;
        src.run_tab = v.run.boff;
        src.run_b0 = v.run_b0;
        src.run_buckets = v.run.padded;
        src.runs = v.run.rows;
    };
    if (g_prepare_only) {  // (plans on what there is; counts nothing, builds nothing)
        if (v.run.p3) hand_out();
        return MEMO_OK;
    }
    const int answered = v.run_answered++;  // queries the deciding copy of this run has answered before this one
    if (v.run.p3) {
        hand_out();
        return MEMO_OK;
    }
    if (src.build_ms != 0.f || v.run_never[v.cap - km1]) return MEMO_OK;  // (at most one pass a query)
    const double cells = 32.0 * (double)((ix->max_s >> 5) - (ix->min_s >> 5) + 2);
    if (answered < kRunsAskAfter || !pass_due(ix, v.run_lost_ns, v.run_backoff, kPassRuns, cells)) return MEMO_OK;
    DeviceGuard guard(ix->device);
    BuiltView b;
    int64_t b0 = 0;
    uint64_t value_bytes = 0;
    float ms = 0.f;
    const int rc = build_timed(st, &ms, [&]() {
        return run_view_copy(ix->device, v.dec, ix->nb, ix->bbase, ix->min_s, ix->max_s, km1, st, b, &b0, &value_bytes);
    });
    if (rc && rc != kNoRoom) return rc;
    v.run_lost_ns = 0;
    if (rc == kNoRoom) {  // (the pressure may pass: the count goes on, the threshold is four times as far)
        v.run_backoff = backoff_step(v.run_backoff);
        return MEMO_OK;
    }
    pass_measured(ix, kPassRuns, ms, cells);
    if (!b.p3 || b.rows * 2 >= b.padded * 32) {  // gave up, or too many runs: nobody has read it (the pass waited for st)
        (void)hipFree(b.p3);
        (void)hipFree(b.boff);
        v.run_never[v.cap - km1] = 1;
        return MEMO_OK;
    }
    v.run = b;
    v.run_b0 = b0;
    v.run_bytes = run_view_bytes(b.padded, value_bytes);
    ++ix->view_run_copies;
    src.build_ms = ms;
    hand_out();
    keep_views_in_budget(ix, &v, base_bytes, true);
    return MEMO_OK;
}

// The 4-byte rows brought into a query order (memo_interleave.hip: 2 = the conservation order, 3 = the membership order, 0 =
// start order).  In place: no sweep may be reading them, so the device is drained first (memo_index_pack, the A/B switch).
int order_words_now(memo_index *ix, int mode) {
    ix->order_pending = 0;
    if (mode == 3 && ix->bshift != 5) mode = 2;
    if (!ix->pk || !ix->rows || (ix->packed_fmt != 4 && ix->packed_fmt != 12) || mode == ix->row_order) return MEMO_OK;
    DeviceGuard guard(ix->device);
    HIP_TRY(hipDeviceSynchronize());
    drop_packed_views(ix);  // (views are subsets in the old order)
    if (int rc = interleave_words(ix->pk, ix->boff, ix->nb, ix->bshift, ix->packed_fmt, mode, nullptr, ix->d_scratch)) return rc;
    HIP_TRY(hipDeviceSynchronize());
    ix->row_order = mode;
    return MEMO_OK;
}

// The same from inside a query: OUT of place, on the caller's stream -- sweeps queued on the caller's other streams may still
// read the rows as they are, so nothing is overwritten and nothing waits for the device: a second copy is ordered,
// the call waits for ITS stream (like the query that builds a view), the index switches to the copy, the old rows and their
// views go to the retire list.  No room for the copy: the rows stay as they are (kNoRoom).
static int order_words_on(memo_index *ix, int mode, hipStream_t st) {
    if (mode == 3 && ix->bshift != 5) mode = 2;
    if (!ix->pk || !ix->rows || (ix->packed_fmt != 4 && ix->packed_fmt != 12) || mode == ix->row_order) {
        ix->order_pending = 0;
        return MEMO_OK;
    }
    DeviceGuard guard(ix->device);
    uint32_t *copy = nullptr;
    const size_t bytes = ix->packed_rows * sizeof(uint32_t);
    const hipError_t aerr = side_alloc((void **)&copy, bytes);
    if (aerr == hipErrorOutOfMemory) return kNoRoom;
    HIP_TRY(aerr);
    float ms = 0.f;
    const int rc = build_timed(st, &ms, [&]() {
        const hipError_t err = hipMemcpyAsync(copy, ix->pk, bytes, hipMemcpyDeviceToDevice, st);
        if (err != hipSuccess) return fail(MEMO_EHIP, "ordering the rows: %s", hipGetErrorString(err));
        return interleave_words(copy, ix->boff, ix->nb, ix->bshift, ix->packed_fmt, mode, st, ix->d_scratch);
    });
    if (rc) {
        (void)hipStreamSynchronize(st);  // (what was queued may still be writing the copy)
        (void)hipFree(copy);
        return rc;
    }
    for (memo_index::DenseView &v : ix->pviews)  // (views are subsets in the old order)
        if (v.p3) retire_view(ix, v, false);
    retire(ix, ix->pk.release(), bytes);
    ix->pk.adopt(copy);
    ix->row_order = mode;
    ix->order_pending = 0;
    pass_measured(ix, kPassRowOrder, ms, (double)ix->rows);
    return MEMO_OK;
}

// Is it time to bring the 4-byte rows into the query order?  Rows that came in through the builder or an import are in start
// order; what that costs a sweep depends on how many rows share a start (a half-wave's atomics on one cell: profiles/
// r04_row_order.txt -- 1.5 % of a sweep at 5 rows per start, 7 % at 25, 20 % at 25 and k = 101), and the ordering pass costs
// a dozen sweeps or more: the queries so far must have lost that much (pass_due), or memo_index_prepare asks for it.
// WHICH order follows from the kind of query that has paid for the pass: conservation deals a bucket's rows over its starts
// (interleave mode 2), membership over annot mod 32 (mode 3: the lanes of a half-wave on different genomes' plane rows).  Round 4
// had measured the two level on config 4 -- under a planes kernel whose every row waited for the LDS (memo_sweep_memb.hip:
// planes_put); since round 5 it does not, and on the sequence-built index the membership order is 6-7 % ahead at k = 31 and 101
// (config 4: level; profiles/r05_large_k.txt).  Rows that are in the OTHER kind's order (memo_index_pack orders for conservation:
// it cannot know) are re-ordered by the same rule with that gain, each time four times later: kinds that alternate settle.
constexpr double kMembershipOrderGain = 0.06;
static int keep_row_order(memo_index *ix, int64_t window, int km1, bool membership, hipStream_t st) {
    if (!ix->pk || (ix->packed_fmt != 4 && ix->packed_fmt != 12)) return MEMO_OK;
    int want = ix->tune.row_order ? ix->tune.row_order - 1 : (membership ? 3 : kRowOrderDefault);
    if (want == 3 && ix->bshift != 5) want = 2;  // (as order_words_on maps it)
    if (want == ix->row_order) return MEMO_OK;
    const bool pending = ix->order_pending != 0;  // the rows are in start order
    if (!pending && (ix->tune.row_order || ix->row_order == 0)) return MEMO_OK;  // (an order asked for by name, or none wanted: stays)
    if (!g_prepare_only) {
        const double span = (double)ix->max_s - (double)ix->min_s + 1.0, per_start = (double)ix->rows / (span > 1 ? span : 1);
        double gain = 0.003 * per_start * (km1 >= 64 ? 3.0 : 1.0);
        gain = gain > 0.2 ? 0.2 : gain;
        if (!pending && membership) gain = kMembershipOrderGain;
        ix->order_lost_ns += rows_in_window(ix, (double)ix->rows, window, km1) * 1.3 * kSweepNsPerRow * gain;
        if (!pass_due(ix, ix->order_lost_ns, ix->order_backoff, kPassRowOrder, (double)ix->rows)) return MEMO_OK;
    }
    const int rc = order_words_on(ix, want, st);
    if (rc && rc != kNoRoom) return rc;
    ix->order_lost_ns = 0;
    // no room: the pressure may pass -- look again, later; a change of kinds: the next one has to be worth more
    if (rc == kNoRoom || !pending) ix->order_backoff = backoff_step(ix->order_backoff);
    return MEMO_OK;
}

// the class of k - 1 = km1 for the 4-byte words: caps in steps of 2 up to 32 (an odd k -- 21, 31 -- gets exactly the rows that
// can write), of 8 up to 64, of 16 up to 128 (twenty-four classes)
static int view_slot(int km1, int *cap) {
    if (km1 <= 32) {
        *cap = 2 * ((km1 + 1) / 2);
        return *cap / 2 - 1;
    }
    if (km1 <= 64) {
        *cap = 8 * ((km1 + 7) / 8);
        return 16 + (*cap - 40) / 8;
    }
    if (km1 <= 128) {
        *cap = 16 * ((km1 + 15) / 16);
        return 20 + (*cap - 80) / 16;
    }
    return -1;
}

// the class of k - 1 = km1 for the dense rows: classes of two, k - 1 <= 2, 4, 6 ... 32 (an odd k: exactly its rows); cap = 2 * (slot + 1)
static int dense_slot(int km1) { return (km1 + 1) / 2 - 1; }

// What a pass handed back becomes a view's rows here and nowhere else (rpg: 5 / 6 rows per group, 0 the 4-byte words).
static void adopt(memo_index::DenseView &v, const BuiltView &b, int rpg) {
    static_cast<BuiltView &>(v) = b;
    v.bytes = rpg ? dense_view_bytes(b.padded, rpg) : b.padded * 4;
}

// The first view of a class: `build` runs the pass (timed, on st), then the view is installed -- or the class is marked as not
// worth a view (state 2: too few rows would go), or, with no room on the device, starts again, later (the sweep reads all the rows).
// pass: what was built (kPassPlaces: a dense view with its rows placed at once); rpg: 5 / 6 rows per group, 0 the 4-byte words.
// pass_ms: the pass's device time, when it left the class a view (RowSource::build_ms).
template <typename Build>
static int install_view(memo_index *ix, memo_index::DenseView &v, hipStream_t st, int cap, Pass pass, double units, int rpg, uint64_t base_bytes,
                        float &pass_ms, Build build) {
    DeviceGuard guard(ix->device);
    BuiltView b;
    const int rc = build_timed(st, &v.build_ms, [&]() { return build(b); });
    if (rc && rc != kNoRoom) return rc;
    adopt(v, b, rpg);
    v.cap = cap;
    v.state = v.p3 ? 1 : (rc == kNoRoom ? 0 : 2);
    if (rc == kNoRoom) {  // (the pressure may pass: look again, but not with every query)
        v.lost_ns = 0;
        v.seen = 0;
        v.backoff = backoff_step(v.backoff);
        v.ask_after = ask_after_step(v.ask_after);
    }
    if (v.state == 1) {
        ++ix->view_builds;
        v.placed = pass == kPassPlaces ? 1 : 0;
        if (v.placed) ++ix->view_placings;
        pass_ms = v.build_ms;
        pass_measured(ix, pass, v.build_ms, units);
        keep_views_in_budget(ix, &v, base_bytes, rpg != 0);
    }
    return MEMO_OK;
}

// A resident dense view replaced by another of its class (pass: kPassPlaces -- the same rows, placed; kPassLiveCopy -- the placed
// six-row view without its dead groups): `build` makes a second view beside the one in use (sweeps queued on the caller's other
// streams may still read that one), then the class switches over and the old copy waits on the retire list with its tile tables.
// No room for the second copy: the view stays as it is and `ledger`, the pass's sum, starts again towards four times the cost.
template <typename Build>
static int replace_view(memo_index *ix, memo_index::DenseView &v, hipStream_t st, Pass pass, double units, int rpg, uint64_t base_bytes,
                        double &ledger, float &pass_ms, Build build) {
    DeviceGuard guard(ix->device);
    BuiltView b;
    memo_index::DenseView nv;
    const int rc = build_timed(st, &nv.build_ms, [&]() { return build(b); });
    if (rc && rc != kNoRoom) return rc;
    if (rc == kNoRoom || !b.p3) {
        ledger = 0;
        v.backoff = backoff_step(v.backoff);
        return MEMO_OK;
    }
    // The new view keeps its class's cap and is as due as the old one was (not an eviction); both passes leave a placed view, with
    // the class's rows (the live copy: a dead row is answered by a live one that contains it) and every ledger at nothing.
    adopt(nv, b, rpg);
    nv.cap = v.cap;
    nv.backoff = v.backoff;
    nv.ask_after = v.ask_after;
    nv.state = 1;
    nv.placed = 1;
    nv.live = pass == kPassLiveCopy ? 1 : 0;
    if (nv.live)  // not a view of its own: view_builds, view_placings and views_resident stay
        ++ix->view_live_copies;
    else
        ++ix->view_placings;
    retire_view(ix, v, false);
    v = nv;
    pass_ms = v.build_ms;
    pass_measured(ix, pass, v.build_ms, units);
    keep_views_in_budget(ix, &v, base_bytes, true);
    return MEMO_OK;
}

// The same k-class views for the 4-byte words (formats 4 and 12; what membership queries, k > 64 and indexes of more than 511
// genomes read): the rows whose overlap is below the class's cap (2, 4 ... 32, 40 ... 64, 80 ... 128), with their own bucket table, built
// when it has become worth it (view_due) and spares a fifth of the rows.  BASELINE config 5 at k = 101 sweeps ... its 8.4 * 10^8 rows that way.
int packed_rows_for(memo_index *ix, int km1, int64_t window, bool membership, hipStream_t st, RowSource &src) {
    if (int rc = keep_row_order(ix, window, km1, membership, st)) return rc;
    src = {ix->pk, ix->boff, ix->rows};  // (the index's own rows; no view: the other fields' defaults)
    if (!ix->views_on || ix->tune.no_views || km1 < 1 || !ix->pk || (ix->packed_fmt != 4 && ix->packed_fmt != 12)) return MEMO_OK;
    int cap = 0;
    const int slot = view_slot(km1, &cap);
    if (slot < 0) return MEMO_OK;
    memo_index::DenseView &v = ix->pviews[slot];
    if (v.state == 0 && !view_due(ix, v, kPassPackedView, (double)ix->rows, 1.0 - share_below(ix, cap), window, km1)) return MEMO_OK;
    if (v.state == 0) {
        const int rc = install_view(ix, v, st, cap, kPassPackedView, (double)ix->rows, 0, ix->rows * 4, src.build_ms, [&](BuiltView &b) {
            int r = packed_filter(ix->device, ix->pk, ix->boff, ix->rows, ix->nb, cap, 2, st, ix->packed_fmt == 12 ? 0 : 16, b);
            // (what the filter leaves of an interleaved bucket is no longer dealt evenly: the view's buckets are ordered again)
            if (!r && b.p3 && ix->row_order) r = interleave_words(b.p3, b.boff, ix->nb, ix->bshift, ix->packed_fmt, ix->row_order, st, ix->d_scratch);
            return r;
        });
        if (rc) return rc;
    }
    if (v.state == 1) {
        v.stamp = ++ix->view_clock;
        src.p3 = v.p3;
        src.boff = v.boff;
        src.rows = v.rows;
    }
    return MEMO_OK;
}

// The dense rows a conservation / membership sweep with k - 1 = km1 should read: the k-class VIEW that leaves out the rows
// whose overlap is cap or more (cap = 2, 4, 6 ... 32, the smallest that is >= km1: such a row cannot write at this k --
// memo_query.py:49 drops it per query; here it is dropped once per index and class) when that spares a fifth of the rows or
// more, else the dense rows themselves.  A view is built when its class's queries have lost more to its absence than it costs
// (view_due), or by memo_index_prepare, and kept with the index.
// allow_six: the caller can read groups of SIX rows that carry their bucket (the table-driven conservation sweep: 2.67 B per row
// instead of 3.2; profiles/r04_view_levels.txt: -3 % at k = 31, -7 % at k = 17 against five-row views).  Such a view is what the
// library builds where it applies -- buckets of 32 positions, annots of eight bits, overlaps below 32 -- and where the padding of
// every bucket to whole groups (2.5 rows on average) stays small against the bucket; src.rpg says which kind was handed out.
int dense_rows_for(memo_index *ix, int km1, int64_t window, hipStream_t st, RowSource &src, bool allow_six, bool account) {
    src = {ix->p3, ix->boff3 ? ix->boff3 : ix->boff, ix->boff3 ? ix->rows3 : ix->rows};  // (no view: the other fields' defaults)
    if (!ix->views_on || ix->tune.no_views || km1 > 32 || km1 < 1) return MEMO_OK;
    const int slot = dense_slot(km1), cap = 2 * (slot + 1);
    const double src_rows = (double)src.rows, kept = (double)ix->rows * share_below(ix, cap);
    const double spared = src_rows > kept ? 1.0 - kept / src_rows : 0.0;
    // six rows per group?  (5-bit starts and overlaps, 8-bit annots; the sweep's form for them has at most five level arrays)
    bool six = allow_six && ix->bshift == 5 && ix->max_annot <= 255 && km1 <= 31 && ix->view_rows != 5 && g_six_views != 0;
    // The buckets the rows lie in, not the table's: the table starts at bucket 0 however far from the origin the first row is, and
    // the buckets before it hold nothing to pad.  A table has nb = (last bucket) + 3 entries (memo_index_finalize), so for rows that
    // begin in bucket 0 this is nb - 1 = (last bucket) + 2, what was counted before; never more than the table holds (an imported
    // slice's nb is its caller's), never less than 1 (no rows: max_s = -1).
    const int64_t table_buckets = ix->nb > 1 ? (int64_t)(ix->nb - 1) : 1;
    int64_t spanned = (ix->max_s >> ix->bshift) - (ix->min_s >> ix->bshift) + 2;
    if (spanned < 1 || spanned > table_buckets) spanned = table_buckets;
    if (six && ix->view_rows != 6 && g_six_views != 1) six = kept >= 40.0 * (double)spanned;
    memo_index::DenseView *vp = six ? &ix->views6[slot] : &ix->views[slot];
    if (ix->view_rows == 0 && g_six_views < 0) {  // (the library's choice: whichever kind is there already)
        if (vp->state != 1 && allow_six && ix->bshift == 5 && km1 <= 31 && ix->views6[slot].state == 1) vp = &ix->views6[slot], six = true;
        if (vp->state != 1 && ix->views[slot].state == 1) vp = &ix->views[slot], six = false;
    }
    memo_index::DenseView &v = *vp;
    if (!account) {  // (the same query asking again: what is there, no ledger, no build)
        if (v.state != 1) return MEMO_OK;
    } else if (v.state == 0 && !view_due(ix, v, kPassDenseView, src_rows, spared, window, km1)) {
        return MEMO_OK;
    }
    const bool can_place = ix->view_places && g_view_colouring != 0;
    const uint64_t base_bytes = dense_groups_for(ix->boff3 ? ix->padded3 : ix->padded) * 16;
    const int rpg = six ? 6 : 5;
    auto view_pass = [&](int min_tenths, int colour_km1, BuiltView &b) {  // (src: still the dense rows themselves)
        return dense_view_build(ix->device, src.p3, src.boff, src.rows, ix->nb, cap, min_tenths, st, rpg, colour_km1, b);
    };
    int rc = MEMO_OK;  // at most one pass a query
    if (v.state == 0) {
        const bool place = can_place && g_prepare_only;  // (asked for: everything at once; a query: first the view)
        rc = install_view(ix, v, st, cap, place ? kPassPlaces : kPassDenseView, src_rows, rpg, base_bytes, src.build_ms,
                          [&](BuiltView &b) { return view_pass(2, place ? cap : 0, b); });
    } else if (account && v.state == 1 && !v.placed && can_place && places_due(ix, v, src_rows, window, km1, six)) {
        rc = replace_view(ix, v, st, kPassPlaces, src_rows, rpg, base_bytes, v.unplaced_ns, src.build_ms,
                          [&](BuiltView &b) { return view_pass(0, cap, b); });
    } else if (account && v.state == 1 && v.placed && six && !v.live && v.dead_groups > 0 && ix->view_live && live_due(ix, v, window, km1)) {
        // (measured per group of the flagged view; its tile tables go with it, the sweep below makes the copy's)
        rc = replace_view(ix, v, st, kPassLiveCopy, (double)(v.padded / 6), 6, base_bytes, v.dead_lost_ns, src.build_ms, [&](BuiltView &b) {
            return live_view_copy(ix->device, v, ix->nb, st, b);
        });
    }
    if (rc) return rc;
    if (v.state == 1) {
        v.stamp = ++ix->view_clock;
        src.p3 = v.p3;
        src.boff = v.boff;
        src.rows = six ? v.padded : v.rows;  // (six rows per group: the places a bucket leaves empty are read and swept like rows)
        src.cap = v.cap;
        src.rpg = rpg;
        src.placed = v.placed;
        src.dead_share = six && v.padded ? 6.0 * (double)v.dead_groups / (double)v.padded : 0.0;
        if (account && six && v.live && src.build_ms == 0.f) {  // (at most one pass a query)
            if ((rc = deciding_rows(ix, v, km1, window, st, base_bytes, src))) return rc;
            return run_rows(ix, v, km1, window, st, base_bytes, src);
        }
    }
    return MEMO_OK;
}
}  // namespace memo

extern "C" {

int memo_index_export_view(memo_index_t *ix, int32_t k, int32_t rows_per_group, void *groups, int64_t *boff, uint64_t *rows,
                           uint64_t *group_count, int32_t *cap) {
    if (!ix) return fail(MEMO_EINVAL, "index is NULL");
    if (rows_per_group != 5 && rows_per_group != 6) return fail(MEMO_EINVAL, "rows_per_group is 5 or 6");
    if (rows) *rows = 0;
    if (group_count) *group_count = 0;
    if (cap) *cap = 0;
    const int km1 = k - 1;
    if (km1 < 1 || km1 > 32) return MEMO_OK;  // (no class: nothing to export)
    const memo_index::DenseView &v = (rows_per_group == 6 ? ix->views6 : ix->views)[dense_slot(km1)];
    if (v.state != 1 || !v.p3) return MEMO_OK;  // (not built: memo_index_prepare does that)
    const uint64_t ng = rows_per_group == 6 ? v.padded / 6 : (v.rows + 4) / 5;
    if (rows) *rows = v.rows;
    if (group_count) *group_count = ng;
    if (cap) *cap = v.cap;
    if (!groups && !boff) return MEMO_OK;
    if (!groups || !boff) return fail(MEMO_EINVAL, "groups and boff: both or neither");
    int rc;
    if ((rc = download_pipelined(ix->device, groups, v.p3, (size_t)ng * 16, nullptr))) return rc;
    return download_pipelined(ix->device, boff, v.boff, ix->nb * 8, nullptr);
}

}  // extern "C"
