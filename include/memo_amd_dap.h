/*
 * memo_amd_dap.h -- index-row construction (the dap_to_bed.py step of `memo index`), off the query path.
 * Part of the C ABI of libmemo_amd.so (see memo_amd.h for conventions: plain C types, 0 or a negative
 * code, memo_last_error()).
 */
#ifndef MEMO_AMD_DAP_H
#define MEMO_AMD_DAP_H

#include "memo_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- index-row construction: dap_to_bed.py:55-134 (--mem [--order] [--overlap]) -------------
 * A DAP (src/index.sh:83) has one row per pivot position: the matching statistic of every
 * non-pivot genome at that position.  Rows go in as a HOST int32 matrix [positions][columns],
 * consecutive positions starting at 0, in as many pushes as the caller likes (state carries over);
 * each push produces, on `device`, the (record, start, end, annot) rows the reference would print
 * for those positions, in its order.  rec_begin: nrec + 1 cumulative record offsets of the pivot
 * (from its .fai).  DAP values must lie in [0, 2^31); they are not checked (a negative value gives
 * undefined rows).  Every such value is exact: MEM ends (start + value, up to 2^30 + 2^31) are
 * int64.  memo_dap_fetch copies the rows of the last push; memo_dap_finish returns the
 * chr-end rows of a DAP that stops inside a record (at most `columns` rows). */
typedef struct memo_dap memo_dap_t;
int memo_dap_create(int32_t columns, const int64_t *rec_begin, int32_t nrec, int32_t sort_order,
                    int32_t overlaps, int32_t device, memo_dap_t **out);
int memo_dap_push(memo_dap_t *h, const int32_t *lcp, int64_t positions, uint64_t *out_rows);
int memo_dap_fetch(memo_dap_t *h, int32_t *rec, int64_t *start, int64_t *end, int32_t *annot);
int memo_dap_finish(memo_dap_t *h, int32_t *rec, int64_t *start, int64_t *end, int32_t *annot,
                    uint64_t *out_rows);
/* the same, with the DAP already on the handle's device (dev_lcp: int32 [positions][columns] in HBM, e.g. the
 * matrix of a memo_ms_t -- memo_ms_push_dap is that call) */
int memo_dap_push_dev(memo_dap_t *h, const int32_t *dev_lcp, int64_t positions, uint64_t *out_rows);
void memo_dap_destroy(memo_dap_t *h);
/* host-side parser for the DAP text (whitespace-separated decimal integers), multi-threaded.
 * Returns how many integers the text holds (they are written only when cap is enough), -1 on a
 * malformed character. */
int64_t memo_parse_ints(const char *text, size_t len, int64_t *out, size_t cap);
/* BED text of such rows: "name\tstart\tend\tannot\n" (dap_to_bed.py:105,109).  names: nrec
 * NUL-terminated strings back to back.  Returns the bytes needed; writes only if they fit. */
size_t memo_emit_bed(const int32_t *rec, const int64_t *start, const int64_t *end, const int32_t *annot,
                     uint64_t rows, const char *names, int32_t nrec, char *buf, size_t cap);

/* ---- matching statistics: the MONI stage of `memo index` (src/index.sh:57-80) --------------------------
 * MS_g[p] = the longest l such that pivot record R[p, p + l) is a substring of genome g's text (its records
 * and their reverse complements, separated by NUL bytes, which no pivot byte can equal); a match never runs
 * past the end of its pivot record.  Bytes compare exactly.
 * memo_ms_create: the pivot (rec_begin[nrec] bytes, no NUL; records 1 .. 2^30-1 long) and an int32 DAP matrix
 *   [positions][columns] of zeros, resident on `device` (refused when it does not fit in its free memory).
 *   chunk: pivot positions per walk thread (<= 0: the default).
 * memo_ms_add_genome: builds the suffix array, LCP and min hierarchy of `text` (n < 2^31 - 1 bytes) on the
 *   device and writes the genome's MS into DAP column `column`.  One genome at a time; buffers are reused.
 * memo_ms_add_records: the same for the genome whose records S_1 .. S_s lie back to back in seq (rec_begin: nrec + 1
 *   offsets; no separators), of any total length.  The device assembles its text S_1 $ ... S_s $ rc(S_1) $ ... rc(S_s) $
 *   (rc as `samtools faidx -i`) in pieces, each a run of whole strings under the int32 suffix-array limit; no match
 *   crosses a $, so the MS against the text is the elementwise maximum over the pieces, and that is what the column
 *   receives (the first piece stores, the later ones take the maximum; other columns are never touched).
 *   piece_bytes <= 0: the cap is min(2^30, what the free device memory allows), raised to fit the longest string where
 *   memory allows; else a hard cap in [2, 2^31 - 2].  A string longer than the cap (len + 1 bytes with its $) is
 *   refused before anything is written.  *pieces (may be NULL): how many pieces ran (0 for nrec = 0: a zero column).
 * memo_ms_plan_pieces: the plan memo_ms_add_records follows (host only, no device): strings S_1 .. S_s, rc(S_1) ..
 *   rc(S_s) of rec_len[r] + 1 bytes each, greedily into pieces of at most `cap` bytes; piece_of_string (2 nrec
 *   entries) and *pieces may be NULL.
 * memo_ms_fetch: host copy of DAP rows [first, first + positions).
 * memo_ms_push_dap: memo_dap_push_dev of those rows (same device, same column count).
 * memo_ms_timings: device milliseconds so far of {suffix arrays, LCP + hierarchy, walks}, summed over pieces.
 * memo_suffix_array: the suffix array of text[0, n) on `device` into sa_out (n int32); a suffix that is a
 *   prefix of another sorts first. */
typedef struct memo_ms memo_ms_t;
int memo_ms_create(const uint8_t *pivot, const int64_t *rec_begin, int32_t nrec, int32_t columns, int64_t chunk,
                   int32_t device, memo_ms_t **out);
int memo_ms_add_genome(memo_ms_t *h, const uint8_t *text, int64_t n, int32_t column);
int memo_ms_add_records(memo_ms_t *h, const uint8_t *seq, const int64_t *rec_begin, int32_t nrec, int32_t column,
                        int64_t piece_bytes, int32_t *pieces);
int memo_ms_plan_pieces(const int64_t *rec_len, int32_t nrec, int64_t cap, int32_t *piece_of_string, int32_t *pieces);
int memo_ms_fetch(memo_ms_t *h, int64_t first, int64_t positions, int32_t *out);
int memo_ms_push_dap(memo_ms_t *h, memo_dap_t *dap, int64_t first, int64_t positions, uint64_t *out_rows);
int memo_ms_timings(memo_ms_t *h, float *out3);
void memo_ms_destroy(memo_ms_t *h);
int memo_suffix_array(const uint8_t *text, int64_t n, int32_t *sa_out, int32_t device);


#ifdef __cplusplus
}
#endif
#endif /* MEMO_AMD_DAP_H */
