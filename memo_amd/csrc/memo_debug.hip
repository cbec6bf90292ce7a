// memo_debug.hip -- A/B switches and profiling aids (include/memo_amd_debug.h).  Linked only into
// libmemo_amd_ab.so, which is the product library plus this file: the tests that walk every tile
// shape, tests/fuzz_gpu.py, tools/ab.py and the PMC calibration pass load that one.  The product
// library exports none of this and its kernel-shape choices cannot be changed from outside.
#include "memo_amd_debug.h"
#include "memo_sweep.h"

using namespace memo;

namespace {

// PMC calibration: reads every row of the three columns exactly once with the sweep's own
// access shape (16 B per lane, 1 KiB per wave-instruction) and nothing else, so that
// FETCH_SIZE can be checked against a known byte count (24 B x padded rows) in the same run.
__global__ void stream_rows_kernel(const int64_t *s, const int64_t *e, const int64_t *o,
                                   uint64_t rows, unsigned long long *sink) {
    long long acc = 0;
    for (uint64_t i = 2 * (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x); i < rows;
         i += 2 * (uint64_t)gridDim.x * blockDim.x) {
        const longlong2 a = *reinterpret_cast<const longlong2 *>(s + i);
        const longlong2 b = *reinterpret_cast<const longlong2 *>(e + i);
        const longlong2 c = *reinterpret_cast<const longlong2 *>(o + i);
        acc += a.x ^ a.y ^ b.x ^ b.y ^ c.x ^ c.y;
    }
    if (acc == 0x7fffffffffffffffll) atomicAdd(sink, 1ull);  // keeps the loads alive
}

}  // namespace

extern "C" {

int memo_debug_set_tuning(memo_index_t *ix, int32_t tile_w, int32_t waves, int32_t membership_algo,
                          int32_t row_source, int32_t scatter) {
    if (!ix) return fail(MEMO_EINVAL, "index is NULL");
    if (tile_w != 0 && (tile_w < 256 || tile_w > 8192 || tile_w % 64))
        return fail(MEMO_EINVAL, "tile_w must be 0 or a multiple of 64 in [256, 8192] (powers of two for the clipped kernels)");
    if (waves != 0 && waves != 1 && waves != 4 && waves != 8) return fail(MEMO_EINVAL, "waves must be 0, 1, 4 or 8");
    if (membership_algo != 0 && (membership_algo < 2 || membership_algo > 4))
        return fail(MEMO_EINVAL, "membership_algo must be 0 (choose), 2 (doubling), 3 (runs) or 4 (planes)");
    if (row_source < 0 || row_source > 13 || row_source == 4 || row_source == 6 || row_source == 7 || row_source == 11 || row_source == 12)
        return fail(MEMO_EINVAL, "row_source must be 0 (library's choice: dense rows where they are resident and can answer, else "
                                 "the 4- / 6-byte rows, else the int64 columns), 1 (int64 columns), 2 (same as 0), 3 (4- / 6-byte "
                                 "rows even where the dense rows could answer), 5 (dense rows, every wave works its tile out), 8, 9, 10 or 13 "
                                 "(include/memo_amd_debug.h; 4, 6, 7, 11, 12 were round 3's persistent sweeps: profiles/r03_persistent_sweep.txt)");
    const int32_t chain_off = (scatter >> 8) & 15;  // (bits 8 .. 11: the wide-tile sweep's parts, include/memo_amd_debug.h)
    scatter &= ~(15 << 8);
    if (scatter < 0 || scatter > 5)
        return fail(MEMO_EINVAL, "scatter must be 0 (choose), 1 (clipped), 2 (unclipped, doubling levels), 3 (unclipped, radix-4 levels) "
                                 "4 (unclipped, mixed levels, every array) or 5 (mixed levels, the arrays of the library's level plan)");
    ix->tune.tile_w = tile_w;
    ix->tune.waves = waves;
    ix->tune.memb_algo = membership_algo;
    ix->tune.force_wide = row_source == 1;
    ix->tune.force_packed = row_source == 3;
    ix->tune.persistent = row_source == 5 || row_source == 10 ? 1 : row_source == 8 ? 5 : 0;
    ix->tune.no_views = row_source == 9 || row_source == 5;
    ix->tune.no_all_write = row_source == 13;
    ix->tune.scatter = scatter;
    ix->tune.chain_off = chain_off;
    return MEMO_OK;
}

int memo_debug_row_order(memo_index_t *ix, int32_t order) {
    if (!ix) return fail(MEMO_EINVAL, "index is NULL");
    if (order < 0 || order > 4)
        return fail(MEMO_EINVAL, "row order must be 0 (the library's), 1 (start order), 2 (chunks dealt over the starts), 3 (+ by overlap mod 32) "
                                 "or 4 (dealt over annot mod 32: the membership order)");
    ix->tune.row_order = order;
    return order_words_now(ix, row_order_mode(ix));  // (resident 4-byte rows: now; every later memo_index_pack: as asked)
}

int memo_debug_no_views(memo_index_t *ix, int32_t on) {
    if (!ix) return fail(MEMO_EINVAL, "index is NULL");
    ix->tune.no_views = on ? 1 : 0;  // (views already built stay resident: bench.py times the same index with and without)
    return MEMO_OK;
}

int memo_debug_view_colouring(int32_t on) {  // (views already built keep the order they have)
    g_view_colouring = on ? 1 : 0;
    return MEMO_OK;
}

int memo_debug_six_views(int32_t on) {
    g_six_views = on < 0 ? -1 : (on ? 1 : 0);
    return MEMO_OK;
}

int memo_debug_view_live(const memo_index_t *ix, int32_t k, uint64_t *copies) {
    if (!ix) return fail(MEMO_EINVAL, "index is NULL");
    if (copies) *copies = ix->view_live_copies;
    if (k < 2 || k > 32) return 0;  // (no class)
    const memo_index::DenseView &v = ix->views6[k / 2 - 1];  // (the class of k - 1: memo_view.hip, dense_rows_for)
    return v.p3 && v.live ? 1 : 0;
}

int memo_debug_view_deciding(const memo_index_t *ix, int32_t k, uint64_t *made) {
    if (!ix) return fail(MEMO_EINVAL, "index is NULL");
    if (made) *made = ix->view_deciding_copies;
    if (k < 2 || k > 32) return 0;  // (no class)
    const memo_index::DenseView &v = ix->views6[k / 2 - 1];  // (the class of k - 1: memo_view.hip, dense_rows_for)
    return v.p3 && v.live && v.dec.p3 && v.dec_km1 == k - 1 ? 1 : 0;
}

int memo_debug_export_deciding(memo_index_t *ix, int32_t k, void *groups, int64_t *boff, uint64_t *rows, uint64_t *group_count) {
    if (!ix) return fail(MEMO_EINVAL, "index is NULL");
    if (rows) *rows = 0;
    if (group_count) *group_count = 0;
    const int km1 = k - 1;
    if (km1 < 1 || km1 > 31) return MEMO_OK;  // (no class of six-row views: nothing to export)
    const memo_index::DenseView &v = ix->views6[k / 2 - 1];
    if (v.state != 1 || !v.live || !v.dec.p3 || v.dec_km1 != km1) return MEMO_OK;  // (not made, or made for the class's other k)
    const uint64_t ng = v.dec.padded / 6;
    if (rows) *rows = v.dec.rows;
    if (group_count) *group_count = ng;
    if (!groups && !boff) return MEMO_OK;
    if (!groups || !boff) return fail(MEMO_EINVAL, "groups and boff: both or neither");
    if (int rc = download_pipelined(ix->device, groups, v.dec.p3, (size_t)ng * 16, nullptr)) return rc;
    return download_pipelined(ix->device, boff, v.dec.boff, ix->nb * 8, nullptr);
}

int memo_debug_view_runs(const memo_index_t *ix, int32_t k, uint64_t *made) {
    if (!ix) return fail(MEMO_EINVAL, "index is NULL");
    if (made) *made = ix->view_run_copies;
    if (k < 2 || k > 32) return 0;  // (no class)
    const memo_index::DenseView &v = ix->views6[k / 2 - 1];
    return v.p3 && v.live && v.dec.p3 && v.dec_km1 == k - 1 && v.run.p3 ? 1 : 0;
}

int memo_debug_export_runs(memo_index_t *ix, int32_t k, uint32_t *masks, uint32_t *offsets, uint8_t *values, uint64_t *buckets,
                           uint64_t *value_bytes, uint64_t *runs, int64_t *first_bucket) {
    if (!ix) return fail(MEMO_EINVAL, "index is NULL");
    for (uint64_t *p : {buckets, value_bytes, runs})
        if (p) *p = 0;
    if (first_bucket) *first_bucket = 0;
    const int km1 = k - 1;
    if (km1 < 1 || km1 > 31) return MEMO_OK;  // (no class of six-row views: nothing to export)
    const memo_index::DenseView &v = ix->views6[k / 2 - 1];
    if (v.state != 1 || !v.live || !v.dec.p3 || v.dec_km1 != km1 || !v.run.p3) return MEMO_OK;
    const uint64_t nbk = v.run.padded, vbytes = v.run_bytes - run_view_bytes(nbk, 0);
    if (buckets) *buckets = nbk;
    if (value_bytes) *value_bytes = vbytes;
    if (runs) *runs = v.run.rows;
    if (first_bucket) *first_bucket = v.run_b0;
    if (!masks && !offsets && !values) return MEMO_OK;
    if (!masks || !offsets || !values) return fail(MEMO_EINVAL, "masks, offsets and values: all or none");
    std::vector<uint64_t> tab(nbk);
    if (int rc = download_pipelined(ix->device, tab.data(), v.run.boff, (size_t)nbk * 8, nullptr)) return rc;
    for (uint64_t b = 0; b < nbk; ++b) {
        masks[b] = (uint32_t)tab[b];
        offsets[b] = (uint32_t)(tab[b] >> 32);
    }
    return download_pipelined(ix->device, values, v.run.p3, (size_t)vbytes, nullptr);
}

int memo_debug_fail_side_allocations(int32_t on) {
    g_side_alloc_fails = on != 0;
    return MEMO_OK;
}

int memo_debug_dense_keep_all(int32_t on) {
    g_dense_keep_all = on != 0;
    return MEMO_OK;
}

int memo_debug_one_shot_way(int32_t way) {
    if (way < 0 || way > 2) return fail(MEMO_EINVAL, "one-shot way: 0 the library's, 1 int64 columns, 2 4-byte words");
    g_one_shot_way = way;
    return MEMO_OK;
}

int memo_debug_stream_rows(memo_index_t *ix, void *stream) {
    if (!ix) return fail(MEMO_EINVAL, "index is NULL");
    if (int rc = need_wide(ix)) return rc;
    DeviceGuard guard(ix->device);
    hipLaunchKernelGGL(stream_rows_kernel, dim3(256 * 8), dim3(256), 0, static_cast<hipStream_t>(stream),
                       ix->s, ix->e, ix->o, ix->rows & ~(uint64_t)1,
                       reinterpret_cast<unsigned long long *>(ix->d_scratch.p));
    HIP_TRY(hipGetLastError());
    return MEMO_OK;
}

int memo_debug_last_one_shot_sweep(void) { return g_last_one_shot_sweep; }

int memo_debug_last_membership(const memo_index_t *ix, int32_t *out6) {
    if (!ix || !out6) return fail(MEMO_EINVAL, "index or out6 is NULL");
    for (int i = 0; i < 6; ++i) out6[i] = ix->last_memb[i];
    return MEMO_OK;
}

int memo_debug_last_tiles_per_group(const memo_index_t *ix, int32_t *out) {
    if (!ix || !out) return fail(MEMO_EINVAL, "index or out is NULL");
    *out = ix->last_tiles_per_group;
    return MEMO_OK;
}

int memo_debug_last_pick(const memo_index_t *ix, int32_t *out, int32_t n) {
    constexpr int32_t kFields = (int32_t)(sizeof(memo_index::SweepPick) / sizeof(int32_t));
    static_assert(kFields == 19 && sizeof(memo_index::SweepPick) == 19 * sizeof(int32_t), "memo_amd_debug.h lists the fields");
    if (!ix || !out || n < 0) return fail(MEMO_EINVAL, "index or out is NULL, or n < 0");
    const int32_t *p = reinterpret_cast<const int32_t *>(&ix->last_pick);
    for (int32_t i = 0; i < n && i < kFields; ++i) out[i] = p[i];
    return kFields;
}

int memo_debug_set_stamp_buffer(uint64_t *d_buffer) {
#ifdef MEMO_STAMPS
    g_stamp_buffer = reinterpret_cast<unsigned long long *>(d_buffer);
    return MEMO_OK;
#else
    (void)d_buffer;
    return fail(MEMO_EINVAL, "this build carries no phase stamps (compile with EXTRA=-DMEMO_STAMPS)");
#endif
}

int memo_debug_ms_piece_text(memo_ms_t *h, const uint8_t *seq, const int64_t *rec_begin, int32_t nrec, int64_t piece_bytes,
                              int32_t piece, uint8_t *out, int64_t out_cap, int64_t *out_n) {
    return ms_piece_text(h, seq, rec_begin, nrec, piece_bytes, piece, out, out_cap, out_n);
}

int memo_debug_ms_free_bytes(int64_t bytes) {
    g_ms_free_bytes = bytes < 0 ? -1 : bytes;
    return MEMO_OK;
}

int memo_debug_cooc_flush(int32_t way) {
    if (way < 0 || way > 1) return fail(MEMO_EINVAL, "co-occurrence flush: 0 partials and a reduce launch, 1 atomics");
    g_cooc_flush = way;
    return MEMO_OK;
}

int memo_debug_cooc_times(int32_t on, float *out2) {
    g_cooc_timed = on ? 1 : 0;
    if (out2) out2[0] = g_cooc_ms[0], out2[1] = g_cooc_ms[1];
    return MEMO_OK;
}

int memo_debug_tracks_times(int32_t on, float *out1) {
    g_tracks_timed = on ? 1 : 0;
    if (out1) out1[0] = g_tracks_ms;
    return MEMO_OK;
}

int memo_debug_breaks_times(int32_t on, float *out1) {
    g_breaks_timed = on ? 1 : 0;
    if (out1) out1[0] = g_breaks_ms;
    return MEMO_OK;
}

int memo_debug_pairs_times(int32_t on, float *out2) {
    g_pairs_timed = on ? 1 : 0;
    if (out2) out2[0] = g_pairs_ms[0], out2[1] = g_pairs_ms[1];
    return MEMO_OK;
}

int memo_debug_nearest_times(int32_t on, float *out1) {
    g_nearest_timed = on ? 1 : 0;
    if (out1) out1[0] = g_nearest_ms;
    return MEMO_OK;
}

int memo_debug_nearest_lds(int32_t kib) {
    if (kib != 0 && (kib < 16 || kib > 160)) return fail(MEMO_EINVAL, "LDS of a memo_nearest_dev workgroup: 0 (the library's %d) or [16, 160] KiB", kNearestLdsKib);
    g_nearest_lds_kib = kib ? kib : kNearestLdsKib;
    return MEMO_OK;
}

int memo_debug_mosaic_times(int32_t on, float *out5) {
    g_mosaic_timed = on ? 1 : 0;
    if (out5)
        for (int i = 0; i < 5; ++i) out5[i] = g_mosaic_ms[i];
    return MEMO_OK;
}

int memo_debug_mosaic_shape(int32_t tile, int32_t mark) {
    if (tile != 0 && tile != 4096 && tile != 8192 && tile != 16384 && tile != 32768)
        return fail(MEMO_EINVAL, "positions a tile of memo_mosaic_parse_dev: 0 (the library's %d), 4096, 8192, 16384 or 32768", kMosaicTile);
    if (mark < 0 || mark > 2) return fail(MEMO_EINVAL, "the mark of memo_mosaic_parse_dev: 0 (the library's %d), 1 (the serial lane) or 2 (doubling)", kMosaicMark);
    g_mosaic_tile = tile ? tile : kMosaicTile;
    g_mosaic_mark = mark ? mark : kMosaicMark;
    return MEMO_OK;
}

int memo_debug_features_times(int32_t on, float *out3) {
    g_features_timed = on ? 1 : 0;
    if (out3) out3[0] = g_features_ms[0], out3[1] = g_features_ms[1], out3[2] = g_features_ms[2];
    return MEMO_OK;
}

int memo_debug_maxk_rows(int32_t way) {
    if (way < 0 || way > 1) return fail(MEMO_EINVAL, "maxk row pass: 0 wave-aggregated atomics, 1 one atomic per row");
    g_maxk_rows_way = way;
    return MEMO_OK;
}

int memo_debug_maxk_times(int32_t on, float *out5) {
    g_maxk_timed = on ? 1 : 0;
    if (out5)
        for (int i = 0; i < 5; ++i) out5[i] = g_maxk_ms[i];
    return MEMO_OK;
}

int memo_debug_collect_times(int32_t on, float *out2) {
    g_collect_timed = on ? 1 : 0;
    if (out2) out2[0] = g_collect_ms[0], out2[1] = g_collect_ms[1];
    return MEMO_OK;
}

int memo_debug_panel_times(int32_t on, float *out4) {
    g_panel_timed = on ? 1 : 0;
    if (out4)
        for (int i = 0; i < 4; ++i) out4[i] = g_panel_ms[i];
    return MEMO_OK;
}

int memo_debug_cover_times(int32_t on, float *out4) {
    g_cover_timed = on ? 1 : 0;
    if (out4)
        for (int i = 0; i < 4; ++i) out4[i] = g_cover_ms[i];
    return MEMO_OK;
}

int memo_debug_lengths_times(int32_t on, float *out7) {
    g_lengths_timed = on ? 1 : 0;
    if (out7)
        for (int i = 0; i < 7; ++i) out7[i] = g_lengths_ms[i];
    return MEMO_OK;
}

int memo_debug_spectrum_times(int32_t on, float *out2, int32_t *private_table, uint64_t *atomics) {
    g_spectrum_timed = on & 3;
    if (out2) out2[0] = g_spectrum_ms[0], out2[1] = g_spectrum_ms[1];
    if (private_table) *private_table = g_spectrum_private;
    if (atomics) *atomics = g_spectrum_atomics;
    return MEMO_OK;
}

int memo_debug_mems_times(int32_t on, float *out3) {
    g_mems_timed = on ? 1 : 0;
    if (out3)
        for (int i = 0; i < 3; ++i) out3[i] = g_mems_ms[i];
    return MEMO_OK;
}

}  // extern "C"
