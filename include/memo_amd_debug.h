/*
 * memo_amd_debug.h -- A/B switches and profiling aids.  NOT part of the product ABI: these are
 * exported only by libmemo_amd_ab.so (the product objects + memo_amd/csrc/memo_debug.hip), which
 * tests/, tests/fuzz_gpu.py, tools/ab.py and the PMC calibration pass load instead of
 * libmemo_amd.so.  Results never depend on any of them; they replace nothing in the reference.
 */
#ifndef MEMO_AMD_DEBUG_H
#define MEMO_AMD_DEBUG_H

#include "memo_amd.h"
#include "memo_amd_dap.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Kernel-shape choices of ONE index (0 = let the library choose, which is all the product does).
 * tile_w: positions per tile (256..4096; unclipped conservation: cells per level array, halo included);
 * waves: 1 or 4 waves share a tile (8: the unclipped conservation kernel only);
 * membership_algo: 2 = doubling, 3 = runs (clipped bit planes per genome + register transpose),
 *   4 = planes (unclipped, result staged through LDS; packed rows, <= 512 genomes; else 3);
 * row_source: 0 = the library's choice (conservation: the dense rows where they are resident and can answer,
 *   else the 4- / 6-byte rows, else the int64 columns), 1 = the int64 columns even when packed rows exist,
 *   2 = same as 0 (kept for older scripts), 3 = the 4- / 6-byte rows even where the dense rows could answer,
 *   5 = the dense rows with one workgroup per tile, every wave working its tile out (round 2's kernel: what a negative window start
 *   or a device without room for a tile table gets), 8 = the dense rows with one workgroup per tile that reads its row slice from the
 *   index's tile table (memo_sweep_cons3t.hip); 5 reads all the dense rows,
 *   0 and 8 the k-class view of them where one pays (memo_index_info_t.last_rows_read), 9 = as 0 without views, 10 = as 5
 *   with views, 13 = as 0 with the "this row writes" test kept in the row blocks even where the
 *   view holds exactly the rows that write (cap = k - 1; round 4);
 * scatter (conservation, packed rows): 1 = clip every interval to the tile, 2 = unclipped into doubling
 *   level arrays with a halo, 3 = unclipped into radix-4 level arrays, 4 = unclipped into mixed level arrays
 *   (blocks of 1, 4, 16, then doubling; k - 1 >= 16) with every array a k - 1 of that size can need (rounds 2-3), 5 = the mixed
 *   arrays with the library's level plan (only the arrays some row of the index can write to) -- 2 .. 5 only when every annot of
 *   the index is inside the result matrix, else 1.  Bits 8 .. 10 of scatter, added to any of these, switch parts of the wide-tile
 *   sweep's shortened chain OFF (memo_sweep_cons3t.hip; profiles/tile_chain.txt): 256 = the kernel entry whose head arrives in
 *   registers, 512 = a wave's two fold chunks in flight together, 1024 = the store without the window test in tiles off the
 *   window's edges; all three off is the kernel as it was before them.  Bit 11 (2048) switches OFF the wide tiles' pair kernel (two
 *   tiles per workgroup behind one head, sweep_conservation_wide_pair_kernel; profiles/tile_pairs.txt): every workgroup then
 *   does one tile, as before it. */
int memo_debug_set_tuning(memo_index_t *ix, int32_t tile_w, int32_t waves, int32_t membership_algo,
                          int32_t row_source, int32_t scatter);
/* Order of the 4-byte rows inside a start bucket (memo_amd/csrc/memo_interleave.hip): 0 = the library's choice (3 for conservation, 4 for membership: whichever kind of query pays for the pass), 1 = start order (as the packers write them), 2 = chunks of four rows dealt round-robin
 * over the bucket's starts, 3 = the same with the rows of a start ordered by overlap mod 32, 4 = chunks dealt over annot mod 32,
 * the rows of a class by their end (the order made for the membership planes: 6-7 % on a sequence-built index, level on config 4 -- profiles/r05_large_k.txt).  Applied at once to resident 4-byte rows (their k-class views are dropped) and by every
 * later memo_index_pack of this index.  Results never depend on it. */
int memo_debug_row_order(memo_index_t *ix, int32_t order);
/* 1 = this index's sweeps read all the rows of their format even where a k-class view is resident (views already built stay:
 * bench.py times the same index with and without); 0 = back to the library's choice.  (The product switch is
 * memo_index_set_option(MEMO_OPT_VIEWS), which also drops the views.) */
int memo_debug_no_views(memo_index_t *ix, int32_t on);
/* this THREAD's later builds of a dense k-class view: 0 = the rows keep the order they come in, whoever asks; 1 (the default) = the place
 * of a row inside its 16-byte group may be chosen against LDS bank conflicts (memo_view_build.hip: view_place_bucket; MEMO_OPT_VIEW_PLACES of
 * the index decides).  Results never depend on it. */
int memo_debug_view_colouring(int32_t on);
/* this THREAD's later conservation queries on dense rows: which kind of k-class view they build and read where views of SIX rows per
 * group apply (k - 1 <= 31, up to 255 genomes, buckets of 32 positions; memo_view.hip; info.last_variant 3): 1 = six wherever they apply,
 * 0 = five always, -1 (the default) = the library's choice (MEMO_OPT_VIEW_ROWS of the index, else six where the view holds enough rows
 * per bucket for the padding of every bucket to whole groups not to matter). */
int memo_debug_six_views(int32_t on);
/* placed six-row views of this index copied without their dead groups so far (MEMO_OPT_VIEW_LIVE; memo_view_build.hip: live_view_copy), and
 * whether the six-row view of k's class is such a copy: 1, or 0 (not a copy, or no six-row view of that class is resident) */
int memo_debug_view_live(const memo_index_t *ix, int32_t k, uint64_t *copies);
/* deciding copies this index has made so far (MEMO_OPT_VIEW_DECIDING; memo_view_build.hip: deciding_view_copy), and whether the class of k
 * holds one for exactly this k: 1, or 0 (none, one for the class's other k, or no live copy of that class is resident) */
int memo_debug_view_deciding(const memo_index_t *ix, int32_t k, uint64_t *made);
/* ... and that copy to host memory, as groups of 6 rows that carry their bucket, like memo_index_export_view(..., 6, ...) hands out the
 * live copy it was made of: *rows: the rows that decide a minimum (0: no such copy is resident for this k), *group_count: its groups,
 * boff: info.buckets entries in units of padded row numbers.  groups == boff == NULL: the sizes only. */
int memo_debug_export_deciding(memo_index_t *ix, int32_t k, void *groups, int64_t *boff, uint64_t *rows, uint64_t *group_count);
/* run copies this index has made so far (MEMO_OPT_VIEW_RUNS; memo_view_build.hip: run_view_copy), and whether the class of k holds one
 * for exactly this k: 1, or 0 */
int memo_debug_view_runs(const memo_index_t *ix, int32_t k, uint64_t *made);
/* ... and that copy to host memory: *buckets entries of masks (bit i: position i of the bucket starts a run; bit 0 always) and of offsets
 * (the byte of the bucket's first value; every eighth is a multiple of four), *value_bytes bytes of values (a byte a run, 255: no row; the
 * bytes between one group of eight buckets' last value and the next group's first are 0), *runs of them runs; *first_bucket: the pivot
 * bucket of entry 0.  masks == offsets == values == NULL: the sizes only (all 0: no such copy is resident for this k). */
int memo_debug_export_runs(memo_index_t *ix, int32_t k, uint32_t *masks, uint32_t *offsets, uint8_t *values, uint64_t *buckets,
                           uint64_t *value_bytes, uint64_t *runs, int64_t *first_bucket);
/* this THREAD's later calls: every device allocation for a view or a tile table fails (the test of the no-memory path) */
int memo_debug_fail_side_allocations(int32_t on);
/* this thread's later memo_index_pack_dense / dense builders keep the rows that can never write at k <= 64 in the dense rows */
int memo_debug_dense_keep_all(int32_t on);
/* this thread's later one-shot calls (memo_conservation / memo_membership): 0 = the library's way in, 1 = int64 columns
 * uploaded as they are, 2 = 4-byte words even where the dense rows could answer */
int memo_debug_one_shot_way(int32_t way);
/* memo_index_info_t.last_sweep of the index this thread's last memo_conservation / memo_membership call built and
 * swept (the one-shot forms destroy their index before they return): which kernel family -- hence which row format --
 * answered it */
int memo_debug_last_one_shot_sweep(void);
/* the plan of this index's last memo_query_membership_dev, as its launcher recorded it on the host: out6[0] the algorithm (2 = doubling,
 * 3 = runs, 4 = planes on the 4- / 6-byte rows, 5 = planes on the dense rows; 0 = none yet, or the fill of k <= 1 / an empty index),
 * [1] the tile width in positions, [2] threads per tile, [3] the MW of the planes' row block (0, 2, 3, 4 or 8: the most words a run reaches
 * past its first; -1 where the kernel has none), [4] 1 where the planes' group skew (SK) is on, [5] result words per launch (the
 * slice of genome words; all of them except where the runs kernel sweeps more than 64).  memo_index_info_t.last_sweep says 7 for
 * doubling, runs and planes alike. */
int memo_debug_last_membership(const memo_index_t *ix, int32_t *out6);
/* tiles per workgroup of this index's last table-driven conservation sweep: 2 where the wide tiles' pair kernel answered it, else 1 */
int memo_debug_last_tiles_per_group(const memo_index_t *ix, int32_t *out);
/* what the plan step and the kernel pickers of this index's last conservation query decided, as the launchers recorded it on the host
 * (memo_sweep_cons.hip: query_conservation; memo_sweep_cons3t.hip: launch_halo3t): the first min(n, 19) of
 *   [0] the kernel family, numbered as memo_index_info_t.last_sweep (0: none yet, or the fill of k <= 1 / an empty index),
 *   [1] the row format (0 int64 columns, 4, 12, 6 the 4- / 6-byte rows, 3 the dense rows), [2] CHECKED, [3] TOP (24, 20 or 0),
 *   [4] threads per workgroup, [5] the clipped tile width / cells of a level array / width of a table-driven tile, [6] level arrays,
 *   [7] sizeof(OutT); of the table-driven sweep [8] nlev, [9] AW (all rows write), [10] SP (few groups per tile), [11] six, [12] live,
 *   [13] r4, [14] the chain value, [15] pairs, [16] A9 (256 .. 511 genomes); [17] 1 where sweep_conservation_halo3_kernel (no table)
 *   answered; [18] which table-driven kernel: 1 halo3t, 2 wide_args, 3 wide, 4 wide_pair, 0 none.
 * Returns how many values the record has (19). */
int memo_debug_last_pick(const memo_index_t *ix, int32_t *out, int32_t n);
/* one pass that reads the three int64 columns exactly once (24 B/row) with the sweep's access
 * shape, to calibrate the FETCH_SIZE counter on a known byte count */
int memo_debug_stream_rows(memo_index_t *ix, void *stream);
/* -DMEMO_STAMPS builds of the conservation sweep: a device buffer of 8 uint64 per workgroup that
 * receives the cycles wave 0 spent in each phase (NULL = off) */
int memo_debug_set_stamp_buffer(uint64_t *d_buffer);
/* piece `piece` of a genome text as memo_ms_add_records assembles it on the device (same arguments, same plan), copied to out:
 * its *out_n bytes and the 64 zero bytes behind them, when out_cap holds them.  Returns the number of pieces.  The handle's
 * DAP matrix is not touched. */
int memo_debug_ms_piece_text(memo_ms_t *h, const uint8_t *seq, const int64_t *rec_begin, int32_t nrec, int64_t piece_bytes,
                             int32_t piece, uint8_t *out, int64_t out_cap, int64_t *out_n);
/* this THREAD's later additions to coded matching-statistics handles (memo_ms_create_layout): every allocation of a coded column
 * sees `bytes` of free device memory instead of what the device reports (< 0: off) -- the test of a column that does not fit */
int memo_debug_ms_free_bytes(int64_t bytes);
/* this THREAD's later memo_cooccurrence_dev calls: how the workgroups' 32-bit counts reach the 64-bit matrix: 0 (the default, the
 * product's way) = a partials buffer and a reduce launch, 1 = one 64-bit atomic per pair, mirror and workgroup (the A/B of
 * DESIGN.md 10.4).  The matrix is the same either way. */
int memo_debug_cooc_flush(int32_t way);
/* this THREAD's later memo_cooccurrence_dev calls put event pairs around their launches (on = 1; each launch is then waited for)
 * or do not (0); out2 (may be NULL) receives the device milliseconds of the last timed call: [0] the sweep launches, [1] the
 * reduce launches (0 with atomics: the flush is part of the sweep).  tools/matrix_timing.py reads them. */
int memo_debug_cooc_times(int32_t on, float *out2);
/* this THREAD's later memo_tracks_dev calls put an event pair around their launch (on = 1) or do not (0); out1 (may be NULL)
 * receives the device milliseconds of the last timed call's kernel (the upload of the edges is not in them).
 * tools/tracks_timing.py reads them. */
int memo_debug_tracks_times(int32_t on, float *out1);
/* this THREAD's later memo_breaks_dev calls put an event pair around their launch (on = 1) or do not (0); out1 (may be NULL)
 * receives the device milliseconds of the last timed call's kernel (the upload of the edges is not in them).
 * tools/breaks_timing.py reads them. */
int memo_debug_breaks_times(int32_t on, float *out1);
/* this THREAD's later memo_pairs_dev calls put event pairs around their launches (on = 1; each launch is then waited for) or do not
 * (0); out2 (may be NULL) receives the device milliseconds of the last timed call: [0] the sweep launches, [1] the reduce launches.
 * tools/pairs_timing.py reads them. */
int memo_debug_pairs_times(int32_t on, float *out2);
/* this THREAD's later memo_nearest_dev calls put an event pair around their launch (on = 1) or do not (0); out1 (may be NULL)
 * receives the device milliseconds of the last timed call's kernel (the uploads of the edges and the candidate words are not in
 * them).  tools/nearest_timing.py reads them. */
int memo_debug_nearest_times(int32_t on, float *out1);
/* this THREAD's later memo_nearest_dev and memo_nearest_tile calls: the LDS a workgroup may take, in KiB of [16, 160]; 0 = the
 * library's 72 (two workgroups per CU).  It decides the positions per tile and how many workgroups share a CU (the A/B of
 * DESIGN.md 10.17); 2048 planes take their 113 KiB whatever is set.  The results are the same. */
int memo_debug_nearest_lds(int32_t kib);
/* this THREAD's later memo_mosaic_fold_dev and memo_mosaic_parse_dev calls put event pairs around their launches (on = 1; each is then
 * waited for) or do not (0); out5 (may be NULL) receives the device milliseconds of the last timed launches: [0] the fold, [1] the
 * exits, [2] the walk, [3] the mark, [4] the lines (count, scan and scatter together).  tools/mosaic_timing.py reads them. */
int memo_debug_mosaic_times(int32_t on, float *out5);
/* this THREAD's later memo_mosaic_parse_dev and memo_mosaic_tile calls: the positions a tile (4096, 8192, 16384 or 32768; 0 = the
 * library's 32768) and the mark (1 = one lane walks the staged steps, 2 = the mark rides the pointer doubling; 0 = the library's 2) --
 * the A/B of DESIGN.md 10.18.  The lines are the same. */
int memo_debug_mosaic_shape(int32_t tile, int32_t mark);
/* this THREAD's later memo_segment_conservation_dev and memo_feature_sums_dev calls put event pairs around their launches (on = 1;
 * each is then waited for) or do not (0); out3 (may be NULL) receives the device milliseconds of the last timed launches: [0] the
 * segment kernel, [1] the three scan launches, [2] the gather (the uploads are not in them).  tools/features_timing.py reads them. */
int memo_debug_features_times(int32_t on, float *out3);
/* this THREAD's later memo_maxk_rows_dev calls: how the rows' bounds reach the cells: 0 (the default, the product's way) =
 * wave-aggregated: a segmented min over the lanes that hit the same cell leaves one atomic min per run of equal cells and wave,
 * 1 = one atomic min per row (the A/B of DESIGN.md 10.5).  The cells are the same either way. */
int memo_debug_maxk_rows(int32_t way);
/* this THREAD's later memo_maxk_*_dev calls put event pairs around their launches (on = 1; each launch is then waited for) or do
 * not (0); out5 (may be NULL) receives the device milliseconds of the last timed launch of each kind: [0] the fill of begin, [1] the
 * row pass, [2] the tile minima, [3] their scan, [4] the apply launch of finish.  tools/maxk_timing.py reads them. */
int memo_debug_maxk_times(int32_t on, float *out5);
/* this THREAD's later memo_collect_dev calls put event pairs around their launches (on = 1; each launch is then waited for) or do
 * not (0); out2 (may be NULL) receives the device milliseconds of the last timed call: [0] the sweep launches, [1] the reduce
 * launches.  tools/collect_timing.py reads them. */
int memo_debug_collect_times(int32_t on, float *out2);
/* this THREAD's later memo_panel_planes_dev / _score_dev / _take_dev calls put event pairs around their launches (on = 1; each launch
 * is then waited for) or do not (0); out4 (may be NULL) receives the device milliseconds of the last timed call of each kind: [0] the
 * planes launch, [1] the score sweep, [2] its reduce launch, [3] the take launch with its reduce.  tools/panel_timing.py reads them. */
int memo_debug_panel_times(int32_t on, float *out4);
/* this THREAD's later memo_cover_weights_dev / _score_dev / _take_dev calls put event pairs around their launches (on = 1; each launch
 * is then waited for) or do not (0); out4 (may be NULL) receives the device milliseconds of the last timed call of each kind: [0] the
 * weights launch, [1] the score sweep, [2] its reduce launch, [3] the take launch with its reduce.  tools/cover_timing.py reads them. */
int memo_debug_cover_times(int32_t on, float *out4);
/* this THREAD's later memo_lengths_*_dev calls put event pairs around their launches (on = 1; each launch is then waited for) or do
 * not (0); out7 (may be NULL) receives the device milliseconds of the last timed launch of each kind: [0] the fill of begin (with the
 * carry's cells), [1] the row pass, [2] the carry pass, [3] the tile minima, [4] their scan, [5] the apply launch of finish, [6] the
 * selection.  tools/lengths_timing.py reads them. */
int memo_debug_lengths_times(int32_t on, float *out7);
/* this THREAD's later memo_spectrum_add_dev / memo_spectrum_finish_dev calls put event pairs around their launches (on & 1; each launch
 * is then waited for) and count the global atomics of an add in a device counter (on & 2: one more atomic beside each), or do neither
 * (0).  out2 (may be NULL) receives the device milliseconds of the last timed add and finish; *private_table (may be NULL) whether the
 * last add of this thread accumulated in the workgroup-private table in LDS (1) or merged equal updates per wave before global atomics
 * (0; -1: no add yet); *atomics (may be NULL) the global atomics the last counted add issued.  tools/spectrum_timing.py reads them. */
int memo_debug_spectrum_times(int32_t on, float *out2, int32_t *private_table, uint64_t *atomics);
/* this THREAD's later memo_mems_dev calls put event pairs around their launches (on = 1; each launch is then waited for) or do not
 * (0); out3 (may be NULL) receives the device milliseconds of the last timed call: [0] the count pass, [1] the scan and the gather of
 * the plane bases, [2] the scatter pass.  tools/mems_timing.py reads them. */
int memo_debug_mems_times(int32_t on, float *out3);

#ifdef __cplusplus
}
#endif
#endif /* MEMO_AMD_DEBUG_H */
