// memo_oneshot.hip -- the one-shot host forms: host rows in, host result out, in one call (memo_conservation, memo_membership and
// their *_rows forms).  Host code only: it builds an index the fastest way the rows allow (the builder of memo_hostpack.hip, else
// memo_index_create / upload / finalize), runs one query on it and destroys it.
#include <chrono>
#include <exception>

#include "memo_common.h"
#include "memo_hostcore.h"

using namespace memo;

namespace memo {
thread_local int g_last_one_shot_sweep = 0;  // memo_index_info_t.last_sweep of this thread's last one-shot call (memo_debug.hip)
thread_local int g_one_shot_way = 0;         // which way in one_shot() takes (AB library, memo_debug_one_shot_way: 1 = int64 columns, 2 = 4-byte words)
}  // namespace memo

extern "C" {

// The drop-in for memo_query.py:103-104 + :70: host columns in, host result out.  Rows that can be packed
// (start-sorted, start >= 0, annot in [0, 65535]: every index dap_to_bed.py writes) and k <= 256 take the
// fast way in -- narrowed on the host into pinned memory, 4-6 B/row over PCIe, PackedRows kernels
// (memo_hostpack.hip); anything else is uploaded as int64 columns and finalized on the device.
// stride 1: three columns; 3: ROWS -- filter_pq's own [M, 3] array, row-major (start = the array, end = start + 1, annot = start + 2)
static int one_shot(const int64_t *start, const int64_t *end, const int64_t *annot, uint64_t rows,
                    int64_t qs, int64_t qe, int32_t k, int32_t num_docs, void *out, int32_t device,
                    bool membership, int stride = 1) {
    if (rows && (!start || !end || !annot)) return fail(MEMO_EINVAL, "column pointer is NULL");
    const uint64_t st = (uint64_t)stride;
    memo_index_t *ix = nullptr;
    int rc = MEMO_OK;
    // MEMO_TIMING=1: phase times of the call on stderr (host clock; every phase ends synchronised)
    const bool timing = getenv("MEMO_TIMING") != nullptr;
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
        return std::chrono::duration<double, std::milli>(b - a).count();
    };
    const auto t0 = now();
    const double pinned0 = pinned_alloc_ms_total();
    double in_ms[3] = {0, 0, 0};  // the last builder's device allocation / packing + copies / finish (table, census, destroy)
    if (rows && k > 1 && k - 1 <= 255 && g_one_shot_way != 1) {
        // the dense rows first (3.2 B per row over PCIe and in HBM, sweep_conservation_halo3_kernel) when they can
        // answer THIS query -- judged from the first and last start before the rows are touched, and again from the
        // largest annot once they have been packed; else (or when a row does not fit them) the 4-byte words
        const bool try_dense = g_one_shot_way != 2 &&
                               memo_dense_rows_can_answer(rows, start[0], start[(rows - 1) * st], 0, k, num_docs, membership);
        for (int dense = try_dense ? 1 : 0; dense >= 0 && !ix; --dense) {
            memo_builder_t *b = nullptr;
            const auto ta = now();
            if ((rc = memo_builder_create_rows(rows, device, 0, dense ? MEMO_ROWS_DENSE : MEMO_ROWS_PACKED, &b))) return rc;
            const auto tb = now();
            rc = stride == 1 ? memo_builder_push(b, start, end, annot, rows) : memo_builder_push_rows(b, start, rows);
            const auto tc = now();
            if (!rc) rc = memo_builder_finish(b, &ix);
            const int why = builder_why(b);
            memo_builder_destroy(b);
            in_ms[0] = ms(ta, tb), in_ms[1] = ms(tb, tc), in_ms[2] = ms(tc, now());
            if (rc == MEMO_EUNPACKABLE) {
                rc = MEMO_OK;
                ix = nullptr;
                if (dense && (why & ~16)) break;  // (unsorted, negative start, wild annot: the 4-byte words would refuse them too)
            } else if (rc) {
                return rc;
            } else if (dense && !memo_dense_rows_can_answer(ix->rows, ix->min_s, ix->max_s, ix->max_annot, k, num_docs, membership)) {
                // (the rule query_conservation applies: ALL the index's rows against its span -- rows that can never write
                // may have left the dense rows, memo_common.h: boff3 -- and the largest annot against the result matrix)
                memo_index_destroy(ix);  // (an annot outside the result matrix: the 4-byte kernels flag the reference's IndexError)
                ix = nullptr;
            }
        }
    }
    if (!ix) {
        // (rows that could not be packed on the host -- unsorted, wild annots, k > 256: the int64 columns go up and the device validates
        // and sorts.  From ROWS the three columns are made here first: the rare way, one more pass over the host's memory)
        std::vector<int64_t> cols;
        if (stride != 1 && rows) {
            try {
                cols.resize(3 * rows);
            } catch (const std::exception &) {
                return fail(MEMO_EHIP, "out of host memory for the columns of %llu rows", (unsigned long long)rows);
            }
            int64_t *cs = cols.data(), *ce = cs + rows, *ca = ce + rows;
            HostPool::get().run((int)((rows + 65535) / 65536), [&](int t) {
                const uint64_t i0 = (uint64_t)t * 65536, i1 = i0 + 65536 < rows ? i0 + 65536 : rows;
                for (uint64_t i = i0; i < i1; ++i) cs[i] = start[3 * i], ce[i] = start[3 * i + 1], ca[i] = start[3 * i + 2];
            });
            start = cs, end = ce, annot = ca;
        }
        if ((rc = memo_index_create(rows, device, &ix))) return rc;
        rc = memo_index_upload(ix, start, end, annot, rows);
        if (!rc) rc = memo_index_finalize(ix, 0, 1);
        if (rc) {
            memo_index_destroy(ix);
            return rc;
        }
    }
    const auto t1 = now();
    auto t2 = t1;
    void *d_out = nullptr;
    size_t bytes = 0;
    do {
        if (qe < qs) { rc = fail(MEMO_EINVAL, "ValueError: negative dimensions are not allowed (window end < start)"); break; }
        const int64_t L = qe - qs;
        if (L > 0 && !out) { rc = fail(MEMO_EINVAL, "output pointer is NULL"); break; }
        bytes = membership ? (size_t)L * ((num_docs + 31) / 32) * 4 : (size_t)L * 2;
        DeviceGuard guard(device);
        if (bytes) {
            hipError_t err = hipMalloc(&d_out, bytes);
            if (err != hipSuccess) { rc = fail(MEMO_EHIP, "hipMalloc(%zu): %s", bytes, hipGetErrorString(err)); break; }
        }
        rc = membership ? memo_query_membership_dev(ix, qs, qe, k, num_docs, (uint32_t *)d_out, nullptr)
                        : memo_query_conservation_dev(ix, qs, qe, k, num_docs, (uint16_t *)d_out, nullptr);
        if (rc) break;
        if ((rc = memo_query_check(ix, nullptr))) break;
        g_last_one_shot_sweep = ix->last_sweep;
        t2 = now();
        if (bytes) rc = download_pipelined(device, out, d_out, bytes, nullptr);
    } while (0);
    if (timing && !rc) {
        const auto t3 = now();
        fprintf(stderr,
                "memo one-shot: %llu rows %s: rows in %.1f ms (%.1f GB/s of int64 columns; allocation %.1f, packing + copies %.1f "
                "with %d host threads, finish %.1f; pinned slots allocated in this call %.1f), result alloc + sweep + check %.1f ms, result out %.1f ms (%.1f GB/s), total %.1f ms\n",
                (unsigned long long)rows, ix->has_wide ? "as int64 columns" : (ix->packed_fmt == 6 ? "packed to 6 B" : ix->pk ? "packed to 4 B" : "packed to 3.2 B (dense rows)"),
                ms(t0, t1), rows * 24.0 / 1e6 / (ms(t0, t1) + 1e-9), in_ms[0], in_ms[1], memo_host_threads(nullptr, nullptr), in_ms[2], pinned_alloc_ms_total() - pinned0, ms(t1, t2), ms(t2, t3),
                bytes / 1e6 / (ms(t2, t3) + 1e-9), ms(t0, t3));
    }
    if (d_out) {
        DeviceGuard guard(device);
        (void)hipFree(d_out);
    }
    memo_index_destroy(ix);
    return rc;
}

int memo_conservation(const int64_t *start, const int64_t *end, const int64_t *annot, uint64_t rows,
                      int64_t qs, int64_t qe, int32_t k, int32_t num_docs, uint16_t *out,
                      int32_t device) {
    return one_shot(start, end, annot, rows, qs, qe, k, num_docs, out, device, false);
}

int memo_membership(const int64_t *start, const int64_t *end, const int64_t *annot, uint64_t rows,
                    int64_t qs, int64_t qe, int32_t k, int32_t num_docs, uint32_t *out_bits,
                    int32_t device) {
    return one_shot(start, end, annot, rows, qs, qe, k, num_docs, out_bits, device, true);
}

int memo_conservation_rows(const int64_t *rows3, uint64_t rows, int64_t qs, int64_t qe, int32_t k, int32_t num_docs, uint16_t *out,
                           int32_t device) {
    if (rows && !rows3) return fail(MEMO_EINVAL, "rows pointer is NULL");
    return one_shot(rows3, rows3 + 1, rows3 + 2, rows, qs, qe, k, num_docs, out, device, false, 3);
}

int memo_membership_rows(const int64_t *rows3, uint64_t rows, int64_t qs, int64_t qe, int32_t k, int32_t num_docs, uint32_t *out_bits,
                         int32_t device) {
    if (rows && !rows3) return fail(MEMO_EINVAL, "rows pointer is NULL");
    return one_shot(rows3, rows3 + 1, rows3 + 2, rows, qs, qe, k, num_docs, out_bits, device, true, 3);
}

}  // extern "C"
