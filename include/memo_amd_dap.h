/*
 * memo_amd_dap.h -- index-row construction (the dap_to_bed.py step of `memo index`) the reader of `memo view`, the runs of `memo regions`, the matrix of `memo matrix`, the curves of `memo collect`, the lengths of `memo maxk`, the per-genome lengths of `memo lengths` and the matrices `memo convert`, `memo add` and `memo merge` make of them: off the query path.
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
 *   memory allows (a coded handle first sets aside what its largest possible column takes: the piece's buffers stay while the
 *   column is encoded); else a hard cap in [2, 2^31 - 2].  A string longer than the cap (len + 1 bytes with its $) is
 *   refused before anything is written.  *pieces (may be NULL): how many pieces ran (0 for nrec = 0: a zero column).
 * memo_ms_plan_pieces: the plan memo_ms_add_records follows (host only, no device): strings S_1 .. S_s, rc(S_1) ..
 *   rc(S_s) of rec_len[r] + 1 bytes each, greedily into pieces of at most `cap` bytes; piece_of_string (2 nrec
 *   entries) and *pieces may be NULL.
 * memo_ms_create_layout: memo_ms_create with the DAP's layout chosen.  MEMO_MS_LAYOUT_DENSE is memo_ms_create (the same checks,
 *   order and messages).  MEMO_MS_LAYOUT_CODED keeps no matrix: the walk fills one scratch column int32 [positions], and after a
 *   genome's last piece that column is run-coded.  Matching statistics fall by at most one per position (MS[i] >= MS[i-1] - 1,
 *   across record ends and after the maximum over pieces too), so with expect[i] = max(MS[i-1] - 1, 0), MS[-1] = 0, position i is
 *   FLAGGED iff MS[i] != expect[i] or i is the first position of a coding block (`block` positions, a power of two:
 *   memo_ms_layout_info), and a column is: one flag bit per position in 64-bit words (block / 64 words per coding block), the
 *   int32 MS of every flagged position in position order, and one int64 per coding block, the rank of its first flag.
 *   MS[i] = max(value[j] - (i - j), 0) with j the last flagged position <= i: exact, since every unflagged position equals its
 *   expect.  A column holds, with nblocks = ceil(positions / block),
 *       bytes = 4 * flagged + 8 * (block / 64) * nblocks + 8 * nblocks
 *   of device memory, allocated when it is added (a column added again frees and replaces them; one never added holds none and
 *   reads as zeros, as the dense matrix does).  When a column's buffers do not fit, the call fails with a message that names
 *   the column, the bytes asked for and the bytes free; the column is then as one never added and the handle stays good.
 *   MEMO_MS_LAYOUT_AUTO: dense wherever memo_ms_create would succeed, else coded; refused (before the pivot is read) when not
 *   even the coded floor fits: scratch column + pivot + the flag words and block offsets of every column + the working set of a
 *   1 MiB text that the dense check adds as well.  Everything else of the handle behaves alike in both layouts.
 * memo_ms_plan_layout: that decision, host only (no device call): which layout a pivot of `positions` positions and `columns`
 *   columns gets when `free_bytes` of device memory are free (*chosen; may be NULL) and the bytes that layout needs at creation
 *   (*floor_bytes; may be NULL).  MEMO_EINVAL with "device memory" in the message when the asked-for layout (or, for AUTO,
 *   neither) fits, and for a layout that is none of the three.
 * memo_ms_layout_info: the handle's layout, its coding block, the device bytes now held for the DAP (dense: the matrix; coded:
 *   scratch column + staging rows + what every column's three allocations hold, which equals the formula above), what the matrix would take (dense_bytes), the flagged
 *   positions of all columns, and the device milliseconds so far of the encode and decode passes (0 for a dense handle).
 * memo_ms_column_info: one column's flagged positions and the bytes its allocations hold (coded; never added: 0 and 0.  Dense: 0 and
 *   4 * positions).  Either pointer may be NULL.
 * memo_ms_fetch: host copy of DAP rows [first, first + positions) (coded: decoded on the device into a staging buffer [positions]
 *   [columns] that the handle owns and that only grows, at most 256 MiB of it per step).
 * memo_ms_push_dap: memo_dap_push_dev of those rows (same device, same column count).  A coded handle decodes them into that
 *   staging buffer first, all of them at once: keep pushes moderate.
 * memo_ms_timings: device milliseconds so far of {suffix arrays, LCP + hierarchy, walks}, summed over pieces.
 * memo_ms_set_walk_budget: how many characters the walk extends a match one at a time before it looks the rest up by seed search
 *   (a binary search over the suffix array, 8 bytes per compare), for the add calls that follow.  Long runs (N gaps, satellite
 *   arrays) cost their length / 8 text reads that way instead of two binary searches per character.  0: seed at once; 2^30 or
 *   more: never (a pivot record is shorter); negative: the default, 64.  The matching statistics are the same for every budget.
 * memo_ms_walk_info: what the walks of the last memo_ms_add_genome / memo_ms_add_records read of the genome text, summed over its
 *   pieces (all zeros before the first add).  A text read is one character fetched through the suffix array or one 8-byte word
 *   compared.
 * memo_suffix_array: the suffix array of text[0, n) on `device` into sa_out (n int32); a suffix that is a
 *   prefix of another sorts first. */
typedef struct memo_ms memo_ms_t;
enum { MEMO_MS_LAYOUT_AUTO = 0, MEMO_MS_LAYOUT_DENSE = 1, MEMO_MS_LAYOUT_CODED = 2 };
typedef struct {
    int32_t layout;         /* MEMO_MS_LAYOUT_DENSE or MEMO_MS_LAYOUT_CODED */
    int32_t block;          /* positions per coding block */
    uint64_t device_bytes;  /* held for the DAP now */
    uint64_t dense_bytes;   /* positions * columns * 4 */
    uint64_t flagged;       /* flagged positions, all columns */
    float encode_ms, decode_ms;
} memo_ms_layout_info_t;
int memo_ms_create(const uint8_t *pivot, const int64_t *rec_begin, int32_t nrec, int32_t columns, int64_t chunk,
                   int32_t device, memo_ms_t **out);
int memo_ms_create_layout(const uint8_t *pivot, const int64_t *rec_begin, int32_t nrec, int32_t columns, int64_t chunk,
                          int32_t device, int32_t layout, memo_ms_t **out);
int memo_ms_plan_layout(int64_t positions, int32_t columns, uint64_t free_bytes, int32_t layout, int32_t *chosen,
                        int64_t *floor_bytes);
int memo_ms_layout_info(memo_ms_t *h, memo_ms_layout_info_t *info);
int memo_ms_column_info(memo_ms_t *h, int32_t column, uint64_t *flagged, uint64_t *bytes);
int memo_ms_add_genome(memo_ms_t *h, const uint8_t *text, int64_t n, int32_t column);
int memo_ms_add_records(memo_ms_t *h, const uint8_t *seq, const int64_t *rec_begin, int32_t nrec, int32_t column,
                        int64_t piece_bytes, int32_t *pieces);
int memo_ms_plan_pieces(const int64_t *rec_len, int32_t nrec, int64_t cap, int32_t *piece_of_string, int32_t *pieces);
int memo_ms_fetch(memo_ms_t *h, int64_t first, int64_t positions, int32_t *out);
int memo_ms_push_dap(memo_ms_t *h, memo_dap_t *dap, int64_t first, int64_t positions, uint64_t *out_rows);
/* memo_ms_rows_dev: DAP rows [first, first + positions) where they lie on the device, int32 [positions][columns] (`memo add` reads
 *   them beside the columns it reads back from an index: memo_add_dap_dev).  A dense handle: a pointer into the matrix.  A coded handle:
 *   the rows are decoded into the staging buffer first, all of them at once, as memo_ms_push_dap does.  *d_rows is valid until the next
 *   call on the handle.  positions == 0: *d_rows = NULL and MEMO_OK; a range outside the pivot: MEMO_EINVAL, *d_rows untouched. */
int memo_ms_rows_dev(memo_ms_t *h, int64_t first, int64_t positions, const int32_t **d_rows);
int memo_ms_timings(memo_ms_t *h, float *out3);
typedef struct {
    uint64_t text_reads;            /* all walk threads */
    uint64_t max_chunk_text_reads;  /* the most any one walk chunk read, in any piece */
    uint64_t seeds;                 /* seed searches */
    uint64_t seed_text_reads;       /* text reads spent in them */
    int64_t budget;                 /* the budget the add ran with */
} memo_ms_walk_info_t;
int memo_ms_set_walk_budget(memo_ms_t *h, int64_t steps);
int memo_ms_walk_info(memo_ms_t *h, memo_ms_walk_info_t *info);
void memo_ms_destroy(memo_ms_t *h);
int memo_suffix_array(const uint8_t *text, int64_t n, int32_t *sa_out, int32_t device);


/* ---- `memo view` reading: the text a conservation query wrote, parsed where it will be binned ----
 * Stands in for src/plot_conservation.py:40-49 (fileReader + list(map(int, ...)): one integer per line).  d_text: the
 * WHOLE file, nbytes bytes on `device` (16-byte aligned); d_vec[i] receives the value of line i (values of 65535 or
 * more as 65535: memo_bin_conservation_dev counts them in no column and in the bin's width, as the reference's Counter
 * does), *lines the number of lines.  cap: values d_vec holds; cap < *lines is MEMO_EINVAL (*lines is set), and
 * cap = nbytes / 2 + 1 always suffices.
 * The device reads the grammar `memo query` writes, with the usual hand edits: a line is [ \t]*[0-9]{1,9}[ \t]* -- at
 * most 32 bytes -- ended by \n, \r\n or the end of the text.  Anything else is left to the caller, who reads the file
 * as the reference does: *first_odd_offset is then the smallest offending byte offset (-1: none), d_vec unspecified,
 * the return value still MEMO_OK.  What offends, and where: a byte that is no digit, blank, \t, \r or \n (a sign, an
 * underscore, a NUL, anything >= 0x80), at its own offset; a \r that no \n follows directly (Python's text mode breaks
 * the line there), at its own offset; and, at the offset of the line's terminator (nbytes for a last line without
 * \n): an empty line or one of blanks only, blanks between digits, ten or more digits, a line longer than 32 bytes.
 * Blocking (synchronises `stream`).  (Declared here, with the other text reader that is off the query path, memo_parse_ints: memo_amd.h
 * keeps to the query path's 44 entry points.) */
int memo_parse_conservation_text_dev(const char *d_text, int64_t nbytes, uint16_t *d_vec, int64_t cap, int64_t *lines,
                                     int64_t *first_odd_offset, int32_t device, void *stream);
/* memo_dev_upload for LARGE pageable host memory (a memory-mapped file): in pieces through the library's pinned ring, the
 * worker threads filling the next piece while one crosses PCIe.  Blocking. */
int memo_dev_upload_pipelined(int32_t device, void *dev, const void *host, size_t bytes);

/* ---- `memo regions`: a result as intervals (no counterpart in the reference) ---------------------
 * (Declared here, beside the `memo view` reader, with the other entry points that are not the query seam of memo_amd.h.)
 * The maximal runs of positions with equal key of a result that is still on `device`, compacted there (count per tile,
 * scan, scatter: memo_amd/csrc/memo_runs.hip), so that intervals instead of one line per position leave the device.
 * starts[] are int64 offsets from the window start, ascending.  d_vec / d_bits must be 16-byte aligned (MEMO_EINVAL
 * otherwise, before anything is launched) and is read from [0] to [L) ([L * W)) and nowhere else; L == 0 launches nothing.
 *
 * maximal runs of a conservation result that is on `device`.  mode 0 (value): starts[r], values[r];
 * mode 1 (band, lo <= v <= hi): starts[] holds the boundaries, values is NULL.  *d_starts / *d_values are
 * device buffers the call allocates (NULL when *runs == 0); free with memo_dev_free.  Blocking.
 * Band boundaries: 2j opens an interval, 2j + 1 closes it; the position before the window counts as outside the
 * band, and an odd *runs means that the last interval ends at L.  An allocation that fails returns MEMO_EHIP with the
 * bytes asked for in memo_last_error and leaves nothing allocated. */
int memo_runs_conservation_dev(const uint16_t *d_vec, int64_t L, int32_t mode, int32_t lo, int32_t hi,
                               int64_t **d_starts, uint16_t **d_values, uint64_t *runs, int32_t device, void *stream);
/* the same for a membership result (W = ceil(num_docs / 32) words per position; any W >= 1): a run is a stretch of equal
 * rows, d_run_bits[r * W ...] its W words */
int memo_runs_membership_dev(const uint32_t *d_bits, int64_t L, int32_t num_docs,
                             int64_t **d_starts, uint32_t **d_run_bits, uint64_t *runs, int32_t device, void *stream);
/* positions per tile of the three passes, for tests that want lengths around it: words <= 0: a conservation result;
 * else a membership result of that many words per position */
int32_t memo_runs_tile(int32_t words);
/* The text of the runs, HOST arrays in (what the two calls above returned, downloaded).  Coordinates are pivot positions
 * qs + start, 0-based and half open; fields are tab-separated, lines end in '\n'; no runs: no bytes.
 *   values != NULL   REC  start  end  value                                  (bedGraph)
 *   values == NULL   REC  start  end     per band interval                   (BED3)
 *   membership       REC  start  end  0110...   num_docs characters, genome 0 first
 * Return the number of bytes the text needs; it is written only if it fits in cap. */
size_t memo_emit_runs(const char *record, int64_t qs, int64_t L, const int64_t *starts, const uint16_t *values /* NULL: band */,
                      uint64_t runs, char *buf, size_t cap);
size_t memo_emit_membership_runs(const char *record, int64_t qs, int64_t L, const int64_t *starts, const uint32_t *run_bits,
                                 uint64_t runs, int32_t num_docs, char *buf, size_t cap);

/* ---- `memo matrix`: pairwise k-mer sharing between genomes (no counterpart in the reference) ---------------------
 * (Declared here, beside the `memo regions` block: memo_amd.h keeps to the query path's 44 entry points.)
 * The co-occurrence matrix of a membership result that is still on `device` (memo_amd/csrc/memo_cooc.hip): d_bits is uint32
 * [L][W], W = ceil(num_docs / 32), as memo_query_membership_dev writes it (bit g & 31 of word g >> 5: genome g holds the k-mer;
 * genome 0 is the pivot).  d_bits must be 16-byte aligned (MEMO_EINVAL otherwise, before anything is launched) and is read from
 * [0] to [L * W) and nowhere else; bits at or above num_docs are masked, whatever they hold.  Any num_docs >= 1.  Scratch memory
 * on the device: at most 64 MiB, freed before the call returns; an allocation that fails returns MEMO_EHIP with the bytes asked
 * for in memo_last_error and leaves nothing allocated.
 *
 * C[g][h] += #{p : bit g and bit h set} for a membership result on `device`; d_counts is uint64 [num_docs][num_docs],
 * ADDED to (the caller zeroes it; several windows or slices accumulate).  Blocking. */
int memo_cooccurrence_dev(const uint32_t *d_bits, int64_t L, int32_t num_docs, uint64_t *d_counts, int32_t device, void *stream);
/* positions per tile, for tests that want lengths around it */
int32_t memo_cooccurrence_tile(int32_t words);
/* memo_query_membership_dev of the slice [qs, qe) of the window [whole_qs, whole_qe), so that the slices of a window laid end to
 * end are the window's result: rows with end < start pass the reference's filter by the whole window, not by the slice (they
 * reach any distance left of their start; memo_amd_multi.h sweeps its sub-windows alike).  d_out: the slice's rows, uint32
 * [qe - qs][W].  Queued on `stream` as memo_query_membership_dev queues it; check with memo_query_check. */
int memo_query_membership_slice_dev(memo_index_t *ix, int64_t whole_qs, int64_t whole_qe, int64_t qs, int64_t qe, int32_t k,
                                    int32_t num_docs, uint32_t *d_out, void *stream);

/* ---- `memo collect`: core and covered k-mer curves over genome orders (no counterpart in the reference) ----------------
 * (Declared here, beside the `memo matrix` block: memo_amd.h keeps to the query path's 44 entry points.)
 * The collector's curves of a membership result that is still on `device` (memo_amd/csrc/memo_collect.hip): d_bits as
 * memo_cooccurrence_dev takes it (uint32 [L][W], 16-byte aligned, read from [0] to [L * W) and nowhere else, bits at or above
 * num_docs masked).  orders_host is a HOST pointer, uint16 [num_orders][steps], every entry a genome id below num_docs; repeats and
 * genome 0 are legal.  For order q and step j
 *     d_core   [q][j] += #{p : bit orders[q][i] of row p is set for every i <= j}
 *     d_covered[q][j] += #{p : bit orders[q][i] of row p is set for some  i <= j}          uint64 [num_orders][steps] on `device`
 * ADDED to (the caller zeroes them; several windows or slices accumulate).  MEMO_EINVAL before anything is launched: d_bits not
 * 16-byte aligned, an entry >= num_docs, steps outside [1, num_docs], num_orders outside [0, 65535], num_docs outside [1, 2048],
 * an output that is NULL or not 8-byte aligned.  L == 0 or num_orders == 0 launches nothing and leaves the outputs as they were.
 * The library uploads the orders itself.  Scratch memory on the device: the orders and at most 64 MiB, freed before the call
 * returns; an allocation that fails returns MEMO_EHIP with the bytes asked for in memo_last_error and leaves nothing allocated.
 * Blocking. */
int memo_collect_dev(const uint32_t *d_bits, int64_t L, int32_t num_docs, const uint16_t *orders_host, int32_t num_orders, int32_t steps,
                     uint64_t *d_core, uint64_t *d_covered, int32_t device, void *stream);
/* positions per tile at `words` genome words (512 up to 16 words, 256 up to 32, 128 above), for tests that want lengths around it */
int32_t memo_collect_tile(int32_t words);

/* ---- `memo panel`: the genomes that cover the pivot, chosen greedily (no counterpart in the reference) --------------------
 * (Declared here, beside the `memo collect` block: memo_amd.h keeps to the query path's 44 entry points.)
 * The greedy set cover of a window's membership bits, one step at a time (memo_amd/csrc/memo_panel.hip).  The window's rows stay on
 * `device` as genome-major bit planes: plane g is pitch_words uint32 at d_planes + g * pitch_words, and bit p & 31 of its word
 * p >> 5 is the bit of genome g at window position p.  d_planes is 16-byte aligned and pitch_words a multiple of 4 everywhere below;
 * the two masks d_core and d_covered are uint32 [words] on `device`, 16-byte aligned, laid out as one plane; `words` is a multiple of
 * 4, at most pitch_words: the window's ceil(L / 32) words and the pad words up to the next multiple of 4, which hold zeros and are
 * read.  Nothing at or past pitch_words of a plane is ever read.  All four calls are stateless and blocking; each refuses with
 * MEMO_EINVAL before anything is launched -- a pointer that is NULL or not 16-byte aligned, a pitch_words that is no positive multiple
 * of 4, words or a word range that leaves the pitch, a genome id at or above num_docs, num_docs outside [1, 2048] -- and then leaves
 * planes, masks and outputs as they were.
 *
 * memo_panel_planes_dev: one slice's rows d_bits (uint32 [L][W] as memo_cooccurrence_dev takes it: 16-byte aligned, read from [0] to
 * [L * W) and nowhere else, bits at or above num_docs masked) become the words [word0, word0 + ceil(L / 32)) of the planes
 * [0, num_docs); the bits at or past L of the last word are written as zeros; no other word of any plane is written.  L == 0
 * launches nothing. */
int memo_panel_planes_dev(const uint32_t *d_bits, int64_t L, int32_t num_docs, uint32_t *d_planes, int64_t pitch_words, int64_t word0, int32_t device,
                          void *stream);
/* what no slice writes, for a window of L positions: the pad words [ceil(L / 32), the next multiple of 4) of every plane as zeros,
 * d_core as ones below L (zeros in the last word's tail and in the pad words), d_covered as zeros.  L == 0 launches nothing. */
int memo_panel_begin_dev(uint32_t *d_planes, int64_t pitch_words, int32_t num_docs, int64_t L, uint32_t *d_core, uint32_t *d_covered, int32_t device,
                         void *stream);
/* list_host is a HOST pointer, uint16 [n_list], genome ids below num_docs, repeats legal, n_list in [0, 65535]; scores_host is a HOST
 * pointer, uint64 [n_list][2], WRITTEN (not added to):
 *     scores[i][0] = new  = #{bits of plane list[i] & ~covered}        scores[i][1] = kept = #{bits of plane list[i] & core}
 * over the words [0, words).  The library uploads the list and downloads the scores itself.  Scratch memory on the device: the list,
 * the scores and at most 64 MiB of partial sums, freed before the call returns; an allocation that fails returns MEMO_EHIP with the
 * bytes asked for in memo_last_error and leaves nothing allocated.  n_list == 0 launches nothing. */
int memo_panel_score_dev(const uint32_t *d_planes, int64_t pitch_words, int32_t num_docs, int64_t words, const uint32_t *d_core, const uint32_t *d_covered,
                         const uint16_t *list_host, int32_t n_list, uint64_t *scores_host, int32_t device, void *stream);
/* d_core &= plane `genome`, d_covered |= plane `genome`, in place over the words [0, words); counts_host is a HOST pointer, uint64 [2],
 * written: the bits of the new core, the bits of the new covered.  Scratch as memo_panel_score_dev's. */
int memo_panel_take_dev(const uint32_t *d_planes, int64_t pitch_words, int32_t num_docs, int64_t words, int32_t genome, uint32_t *d_core, uint32_t *d_covered,
                        uint64_t *counts_host, int32_t device, void *stream);
/* positions per tile of memo_panel_planes_dev (1024), and the mask words a workgroup of score and take reads per pass (1024), for
 * tests that want lengths around them */
int32_t memo_panel_tile(void);
int32_t memo_panel_pass_words(void);

/* ---- `memo cover`: the genomes that cover the pivot's matches, at every k (no counterpart in the reference) -------------------
 * `memo panel` summed over every k of [kmin, kmax], one step at a time (memo_amd/csrc/memo_cover.hip).  With span = kmax - kmin + 1
 * and w[g][p] = max(0, min(len[g][p], kmax) - (kmin - 1)) -- memo_pairs_dev's weights of memo_lengths' cells -- the window stays on
 * `device` as weight planes of the genomes a caller names: plane i is `pitch` cells of cell_bytes = 2 (span <= 65535) or 4 bytes at
 * d_weights + i * pitch * cell_bytes.  d_weights is 16-byte aligned and pitch a multiple of a quad, 16 / cell_bytes cells, everywhere
 * below; the two masks d_core and d_covered are [cells] cells on `device`, 16-byte aligned, laid out as one plane; `cells` is a
 * multiple of a quad, at most pitch: the window's L cells and the pad cells up to the next multiple of a quad, which hold zeros and
 * are read.  Nothing at or past `pitch` of a plane is ever read.  All calls are stateless and blocking; each refuses with MEMO_EINVAL
 * before anything is launched -- a pointer that is NULL or not 16-byte aligned, a pitch that is no positive multiple of a quad, cells
 * or a cell range that leaves the pitch, a cell_bytes other than 2 or 4, a span that does not fit the cell, a list entry out of range,
 * n_list outside [0, 65535], num_docs or num_planes outside [1, 2048] -- and then leaves planes, masks and outputs as they were.
 * Every sum is exact for any cell values, spans up to 2^31 - 1 and up to 2^31 - 1 cells.
 *
 * memo_cover_weights_dev: one finished slice of memo_lengths_*_dev, d_lengths (uint32 [num_docs][pitch_src] on `device`, 16-byte
 * aligned, pitch_src a multiple of 4 and at least Ls; the cells [0, Ls) of the planes the list names are read and nothing else),
 * becomes the cells [cell0, cell0 + Ls) of the planes [0, n_list): plane i receives w[list_host[i]], a length above kmax counting
 * as kmax.  list_host is a HOST pointer, uint16 [n_list], genome ids below num_docs, repeats legal.  cell0 is a multiple of 8.  No
 * other cell of any plane is written.  Ls == 0 or n_list == 0 launches nothing. */
int memo_cover_weights_dev(const uint32_t *d_lengths, int64_t Ls, int64_t pitch_src, int32_t num_docs, uint32_t kmin, uint32_t kmax, const uint16_t *list_host,
                           int32_t n_list, void *d_weights, int64_t pitch, int32_t cell_bytes, int64_t cell0, int32_t device, void *stream);
/* what no slice writes, for a window of L positions: the pad cells [L, the next multiple of a quad) of every plane as zeros, d_core
 * as span below L and zeros in the pad cells, d_covered as zeros.  L == 0 launches nothing. */
int memo_cover_begin_dev(void *d_weights, int64_t pitch, int32_t num_planes, int32_t cell_bytes, int64_t L, uint32_t span, void *d_core, void *d_covered,
                         int32_t device, void *stream);
/* list_host is a HOST pointer, uint16 [n_list], plane numbers below num_planes, repeats legal, n_list in [0, 65535]; scores_host is a
 * HOST pointer, uint64 [n_list][2], WRITTEN (not added to):
 *     scores[i][0] = new  = sum of max(0, w - covered)        scores[i][1] = kept = sum of min(w, core)        w: plane list[i]
 * over the cells [0, cells), literally, whatever the cells hold.  The library uploads the list and downloads the scores itself.
 * Scratch memory on the device: the list, the scores and at most 64 MiB of partial sums (128 MiB for lists past 32767 on masks past
 * 2^30 cells of 2 bytes), freed before the call returns; an allocation that fails returns MEMO_EHIP with the bytes asked for in
 * memo_last_error and leaves nothing allocated.  n_list == 0 launches nothing. */
int memo_cover_score_dev(const void *d_weights, int64_t pitch, int32_t num_planes, int32_t cell_bytes, int64_t cells, const void *d_core, const void *d_covered,
                         const uint16_t *list_host, int32_t n_list, uint64_t *scores_host, int32_t device, void *stream);
/* d_core = min(d_core, plane), d_covered = max(d_covered, plane), cell by cell in place over the cells [0, cells); sums_host is a HOST
 * pointer, uint64 [2], written: the sum of the new core, the sum of the new covered.  Scratch as memo_cover_score_dev's. */
int memo_cover_take_dev(const void *d_weights, int64_t pitch, int32_t num_planes, int32_t cell_bytes, int64_t cells, int32_t plane, void *d_core, void *d_covered,
                        uint64_t *sums_host, int32_t device, void *stream);
/* the cells a workgroup of score and take reads per pass (2048 of 2 bytes, 1024 of 4; 0 for any other cell_bytes), for tests that want
 * lengths around it */
int32_t memo_cover_pass_cells(int32_t cell_bytes);

/* ---- `memo tracks`: per-genome k-mer presence along the pivot, binned (no counterpart in the reference) -----------------
 * (Declared here, beside the `memo collect` block: memo_amd.h keeps to the query path's 44 entry points.)
 * The presence counts of a membership result that is still on `device` (memo_amd/csrc/memo_tracks.hip): d_bits as
 * memo_cooccurrence_dev takes it (uint32 [L][W], 16-byte aligned, read from [0] to [L * W) and nowhere else, bits at or above
 * num_docs masked); it holds the positions first .. first + L of a window.  edges_host is a HOST pointer, int64 [bins + 1], bin
 * edges in the window's coordinates, non-decreasing (two equal edges are an empty bin, which counts nothing); the library uploads
 * them itself.
 *     d_counts[g][b] += #{p in [first, first + L) : edges[b] <= p < edges[b + 1] and bit g of row p - first is set}
 * uint64 [num_docs][bins] on `device`, ADDED to (the caller zeroes it; the slices of a window and several windows accumulate, and
 * the table does not depend on where the slices are cut).  MEMO_EINVAL before anything is launched: d_bits not 16-byte aligned,
 * d_counts NULL or not 8-byte aligned, num_docs outside [1, 2048], bins outside [1, 2^20], edges that decrease somewhere,
 * first < edges[0], first + L > edges[bins].  L == 0 launches nothing and leaves the table as it was.  Scratch memory on the device:
 * the edges, (bins + 1) x 8 bytes, freed before the call returns; an allocation that fails returns MEMO_EHIP with the bytes asked
 * for in memo_last_error and leaves nothing allocated.  Blocking. */
int memo_tracks_dev(const uint32_t *d_bits, int64_t L, int32_t num_docs, int64_t first, const int64_t *edges_host, int32_t bins,
                    uint64_t *d_counts, int32_t device, void *stream);
/* positions per tile at `words` genome words (512 up to 16 words, 256 up to 32, 128 above), for tests that want lengths around it */
int32_t memo_tracks_tile(int32_t words);

/* ---- `memo breaks`: k-free match starts and length sums per genome and bin (no counterpart in the reference) ------------
 * (Declared here, beside the `memo tracks` block: memo_amd.h keeps to the query path's 44 entry points.)
 * From finished lengths that are still on `device` (memo_amd/csrc/memo_breaks.hip): d_cells is uint32 [planes][pitch], 16-byte
 * aligned, pitch a multiple of 4, L cells per plane read and nothing else -- memo_lengths_finish_dev's layout; memo_maxk_finish_dev's
 * cells are one plane of it.  halo = 1: cell 0 of every plane is only the left neighbour of cell 1 and is not counted; halo = 0:
 * cell 0 is position 0 of its record.  The counted cells are halo .. L - 1, counted cell i is position first + i - halo.  edges_host
 * is a HOST pointer, int64 [bins + 1], bin edges in the same coordinates, non-decreasing (two equal edges are an empty bin), with
 * edges[0] <= first and first + (L - halo) <= edges[bins]; the library uploads them itself.
 *     d_table[0][g][b] += #{ counted p in bin b : v[p] >= min_len and p starts a match }
 *     d_table[1][g][b] += sum of v[p] over the counted p in bin b                                    (min_len plays no part)
 * uint64 [2][planes][bins] on `device`, ADDED to (the caller zeroes it; the slices of a window accumulate, each with its halo cell,
 * and the table does not depend on where they are cut).  A cell starts a match by memo_mems_dev's rule: v[p - 1] < v[p], or
 * v[p - 1] == v[p] < cap, or it is cell 0 with halo = 0 -- so d_table[0][g] is the histogram of the starts memo_mems_dev reports
 * for plane g.  MEMO_EINVAL before anything is launched, the table as it was: d_cells not 16-byte aligned, pitch not a multiple of 4
 * or below L, L < 0 or above 2^31, planes outside [0, 2048], bins outside [1, 2^20 + 1], cap outside [1, 2^31 - 1], min_len outside
 * [1, cap], halo not 0 or 1, edges that are NULL or decrease somewhere, a slice that leaves the edges, a table that is NULL or not
 * 8-byte aligned.  L - halo <= 0 or planes == 0 launches nothing and leaves the table as it was.  Scratch memory on the device: the
 * edges, (bins + 1) x 8 bytes, freed before the call returns; an allocation that fails returns MEMO_EHIP with the bytes asked for in
 * memo_last_error and leaves nothing allocated.  Blocking. */
int memo_breaks_dev(const uint32_t *d_cells, int64_t L, int64_t pitch, int32_t planes, uint32_t cap, uint32_t min_len, int32_t halo,
                    int64_t first, const int64_t *edges_host, int32_t bins, uint64_t *d_table, int32_t device, void *stream);
/* cells per tile (1024), for tests that want lengths around it */
int32_t memo_breaks_tile(void);

/* ---- `memo pairs`: k-free pairwise shared match length between genomes (no counterpart in the reference) ----------------
 * (Declared here, beside the `memo breaks` block: memo_amd.h keeps to the query path's 44 entry points.)
 * From finished lengths that are still on `device` (memo_amd/csrc/memo_pairs.hip): d_cells is uint32 [planes][pitch], 16-byte
 * aligned, pitch a multiple of 4, L cells per plane read and nothing else -- memo_lengths_finish_dev's layout, no halo.  With
 *     w[g][p] = max(0, min(v[g][p], kmax) - (kmin - 1))          the number of k in [kmin, kmax] at which genome g holds the k-mer at p
 *     d_sums[g][h] += sum over p in [0, L) of min(w[g][p], w[h][p])
 * uint64 [planes][planes] on `device`, symmetric, ADDED to (the caller zeroes it; the slices of a window accumulate, and the matrix
 * does not depend on where they are cut).  A cell above kmax counts as kmax.  With kmin == kmax == k it is memo_cooccurrence_dev's
 * matrix of `memo query -m -k k`, for index rows with end >= start; over [kmin, kmax] the sum of those matrices.  The sums are exact
 * at every span kmax - kmin + 1: up to memo_pairs_narrow_span() the kernel adds in 32 bits per tile and widens between tiles,
 * above it in 64 bits.  More than memo_pairs_chunk() planes are taken in chunks, one launch per pair of chunks.  MEMO_EINVAL
 * before anything is launched, the matrix as it was: d_cells not 16-byte aligned, pitch not a multiple of 4 or below L, L < 0 or
 * above 2^31, planes outside [0, 2048], kmax outside [1, 2^31 - 1], kmin outside [1, kmax], a matrix that is NULL or not 8-byte
 * aligned.  L == 0 or planes == 0 launches nothing and leaves the matrix as it was.  Scratch memory on the device: at most 64 MiB,
 * freed before the call returns; an allocation that fails returns MEMO_EHIP with the bytes asked for in memo_last_error and leaves
 * nothing allocated.  Blocking. */
int memo_pairs_dev(const uint32_t *d_cells, int64_t L, int64_t pitch, int32_t planes, uint32_t kmin, uint32_t kmax, uint64_t *d_sums,
                   int32_t device, void *stream);
/* positions per tile (128), for tests that want lengths around it */
int32_t memo_pairs_tile(void);
/* the most planes one launch stages (128): above it the planes come in chunks of half as many */
int32_t memo_pairs_chunk(void);
/* the largest span kmax - kmin + 1 that takes the 32-bit form: span x tile < 2^32 */
uint32_t memo_pairs_narrow_span(void);

/* ---- `memo nearest`: which genome matches the pivot longest, per position and per bin (no counterpart in the reference) ---
 * (Declared here, beside the `memo pairs` block: memo_amd.h keeps to the query path's 44 entry points.)
 * From finished lengths that are still on `device` (memo_amd/csrc/memo_nearest.hip): d_cells is uint32 [planes][pitch], 16-byte
 * aligned, pitch a multiple of 4, L cells per plane read and nothing else -- memo_lengths_finish_dev's layout, no halo; cell i is
 * position first + i.  v[g][p] = min(cell, cap).  cand_host is a HOST pointer to 64 words, bit g = genome g is a candidate, or NULL
 * for 1 .. planes - 1; plane 0 (the pivot) is never a candidate, and neither it nor a plane outside the set is read.  edges_host is a
 * HOST pointer, int64 [bins + 1], bin edges in the positions' coordinates, non-decreasing (two equal edges are an empty bin), with
 * edges[0] <= first and first + L <= edges[bins]; the library uploads both itself.  With best[p] = the largest v[g][p] over the
 * candidates, ok[p] = best[p] >= min_len, att[g][p] = ok[p] and v[g][p] == best[p] (every tied genome attains), sole[g][p] =
 * att[g][p] and no other genome attains:
 *     d_wins[0][g][b] += #{ p in bin b : att[g][p] }       g >= 1;     d_wins[0][0][b] += #{ p in bin b : not ok[p] }      ("none")
 *     d_wins[1][g][b] += #{ p in bin b : sole[g][p] }      g >= 1;     d_wins[1][0][b] += the same "none" count
 *     d_sums[b]       += sum of best[p] over bin b                                                  (min_len plays no part)
 *     d_winner[i]      = the smallest g with att[g][i], 0 where not ok[i]                           uint16 [L], WRITTEN
 * d_wins is uint64 [2][planes][bins] and d_sums uint64 [bins] on `device`, ADDED to (the caller zeroes them; the slices of a window
 * accumulate, and the tables do not depend on where they are cut); each of the three outputs may be NULL and is then not computed.
 * With min_len == cap == K row g of d_wins[0] is row g of memo_tracks_dev at k = K.  MEMO_EINVAL before anything is launched, the
 * outputs as they were: d_cells not 16-byte aligned, pitch not a multiple of 4 or below L, L < 0 or above 2^31, planes outside
 * [2, 2048], cap outside [1, 2^31 - 1], min_len outside [1, cap], a candidate set that is empty, names bit 0 or names a bit at or
 * past planes, all three outputs NULL, a table that is not 8-byte aligned, a winner that is not 2-byte aligned; with a table: bins
 * outside [1, 2^20 + 1], edges that are NULL or decrease somewhere, a slice that leaves the edges; without a table edges may be NULL
 * with bins == 0.  L == 0 launches nothing and leaves everything as it was.  A workgroup takes a run of tiles, at most 1024 runs a
 * call.  Scratch memory on the device: the edges, (bins + 1) x 8 bytes, and the 64 candidate words, freed before the call returns;
 * an allocation that fails returns MEMO_EHIP with the bytes asked for in memo_last_error and leaves nothing allocated.  Blocking. */
int memo_nearest_dev(const uint32_t *d_cells, int64_t L, int64_t pitch, int32_t planes, uint32_t cap, uint32_t min_len,
                     const uint32_t *cand_host, int64_t first, const int64_t *edges_host, int32_t bins, uint64_t *d_wins, uint64_t *d_sums,
                     uint16_t *d_winner, int32_t device, void *stream);
/* positions per tile at that many planes (256 up to 67 planes, 128 up to 109, 64 up to 216, 32 up to 415, 16 up to 763, then 8; 0 for planes outside [2, 2048]), for tests that
 * want lengths around it */
int32_t memo_nearest_tile(int32_t planes);

/* ---- `memo mosaic`: the pivot as the fewest pieces copied whole from one genome each (no counterpart in the reference) -------------
 * (Declared here, beside the `memo nearest` block: memo_amd.h keeps to the query path's 44 entry points.)
 * The greedy parse by longest match (memo_amd/csrc/memo_mosaic.hip), in two calls.  The FOLD takes one slice of finished lengths as
 * memo_nearest_dev takes it -- d_cells uint32 [planes][pitch], 16-byte aligned, pitch a multiple of 4, L cells a plane read and
 * nothing else; v[g][p] = min(cell, cap); cand_host a HOST pointer to 64 words, bit g = genome g is a candidate, or NULL for
 * 1 .. planes - 1; plane 0 and the planes outside the set are never read -- and WRITES, with best, ok and the winner as there (ties to
 * the lowest annot),
 *     d_step[i]   = ok[i] ? best[i] : 1        uint32 [L]: a position no candidate reaches at min_len is a literal of one base
 *     d_winner[i] = the winner, 0 where not ok[i]                                                          uint16 [L]
 * on `device`; they are a slice's part of the whole window's vectors and may sit at any element offset (4- and 2-byte aligned).
 * MEMO_EINVAL before anything is launched, the outputs as they were: what memo_nearest_dev refuses of d_cells, pitch, L, planes, cap,
 * min_len and the candidate words; L above 2^31 - 1; d_step or d_winner NULL or misaligned.  L == 0 launches nothing.  Scratch: the
 * candidate list, at most 8 KiB.  Blocking. */
int memo_mosaic_fold_dev(const uint32_t *d_cells, int64_t L, int64_t pitch, int32_t planes, uint32_t cap, uint32_t min_len,
                         const uint32_t *cand_host, uint32_t *d_step, uint16_t *d_winner, int32_t device, void *stream);
/* The PARSE of a whole window: d_step uint32 [L] and d_winner uint16 [L] on `device`, both 16-byte aligned.  p_0 = 0, p_{i+1} = p_i +
 * max(d_step[p_i], 1) while p_i < L are the reached positions (a step of 0 counts as 1, a step above 2^31 - 1 as 2^31 - 1); a reached
 * p starts a line iff d_winner[p] != 0, or p == 0, or not (p - 1 is reached and d_winner[p - 1] == 0): consecutive phrases of no
 * genome are one line (the fold gives a position of no genome a step of 1; a caller's own vectors should), adjacent phrases of one
 * genome stay two.  *d_starts (int64 [*lines], ascending, the first one 0) and
 * *d_genomes (uint16 [*lines], the winner at each start) are allocated on `device` for exactly *lines entries and are the caller's,
 * to be freed with memo_dev_free; line r ends where line r + 1 starts, the last one at L.  MEMO_EINVAL before anything is launched,
 * the outputs as they were: NULL out-pointers, L < 0 or above 2^31 - 1, d_step or d_winner NULL or not 16-byte aligned.  L == 0
 * launches nothing and returns zero lines and NULL arrays.  Scratch memory on the device: 4 L bytes, one bit a position rounded up to
 * whole tiles, 4 bytes a tile and the compaction's counts, freed before the call returns; an allocation that fails returns MEMO_EHIP
 * with the bytes asked for in memo_last_error and leaves nothing allocated.  Blocking. */
int memo_mosaic_parse_dev(const uint32_t *d_step, const uint16_t *d_winner, int64_t L, int64_t **d_starts, uint16_t **d_genomes,
                          uint64_t *lines, int32_t device, void *stream);
/* positions per tile of the parse (32768), for tests that want lengths around it */
int32_t memo_mosaic_tile(void);

/* ---- `memo features`: per-feature presence and conservation from a BED file (no counterpart in the reference) -----------
 * (Declared here, beside the `memo tracks` block: memo_amd.h keeps to the query path's 44 entry points.)
 * Features overlap and nest; the elementary segments between their endpoints do not.  A table is counted per segment -- with a
 * membership index by memo_tracks_dev, the segment edges as its bins; with a conservation index by memo_segment_conservation_dev --
 * and memo_feature_sums_dev turns it into the table per feature (memo_amd/csrc/memo_features.hip).
 *
 * The sum and the count at or above a threshold of a conservation result that is still on `device`: d_vec is uint16 [L], 16-byte
 * aligned, read from [0] to [L) and nowhere else, 16 bytes a lane and load; it holds the positions first .. first + L of a window.
 * edges_host is a HOST pointer, int64 [segs + 1], segment edges in the window's coordinates, non-decreasing (two equal edges are
 * an empty segment, which counts nothing); the library uploads them itself.
 *     d_sums[0][s] += sum of v[p - first]                        over p in [first, first + L) with edges[s] <= p < edges[s + 1]
 *     d_sums[1][s] += #{such p : v[p - first] >= threshold}
 * uint64 [2][segs] on `device`, ADDED to (the caller zeroes it; the slices of a window accumulate, and the table does not depend
 * on where the slices are cut).  MEMO_EINVAL before anything is launched: d_vec not 16-byte aligned, d_sums NULL or not 8-byte
 * aligned, segs outside [1, 2^20 + 1], a threshold outside [0, 65536], edges that decrease somewhere, first < edges[0],
 * first + L > edges[segs].  L == 0 launches nothing and leaves the table as it was.  Scratch memory on the device: the edges,
 * (segs + 1) x 8 bytes, freed before the call returns; an allocation that fails returns MEMO_EHIP with the bytes asked for in
 * memo_last_error and leaves nothing allocated.  Blocking. */
int memo_segment_conservation_dev(const uint16_t *d_vec, int64_t L, int64_t first, const int64_t *edges_host, int32_t segs,
                                  int32_t threshold, uint64_t *d_sums, int32_t device, void *stream);
/* positions per tile (2048), for tests that want lengths around it */
int32_t memo_segment_conservation_tile(void);
/* From segments to features: d_sums is uint64 [rows][segs] on `device`, 8-byte aligned, and becomes SCRATCH -- the call overwrites
 * it with its prefix sums along every row.  lo_host and hi_host are HOST pointers, int32 [features]: feature f is the segments
 * lo[f] .. hi[f] - 1 (lo == hi: none); the library uploads them itself.
 *     d_out[f][r] = sum of d_sums[r][s] over lo[f] <= s < hi[f]                    uint64 [features][rows] on `device`, feature-major
 * modulo 2^64 (a prefix that wraps still gives the exact difference).  MEMO_EINVAL before anything is launched, with d_sums and d_out
 * as they were: rows outside [1, 2048], segs outside [1, 2^20 + 1], features < 0, a pointer that is NULL or not 8-byte aligned, a
 * feature with lo < 0, lo > hi or hi > segs.  features == 0 launches nothing and writes nothing.  Scratch memory on the device: lo
 * and hi, and 8 bytes per row and memo_feature_sums_tile() segments, freed before the call returns; an allocation that fails returns
 * MEMO_EHIP with the bytes asked for in memo_last_error and leaves nothing allocated.  Blocking. */
int memo_feature_sums_dev(uint64_t *d_sums, int32_t rows, int32_t segs, const int32_t *lo_host, const int32_t *hi_host, int32_t features,
                          uint64_t *d_out, int32_t device, void *stream);
/* segments per tile of the scan (2048), for tests that want segment counts around it */
int32_t memo_feature_sums_tile(void);

/* ---- `memo maxk`: the longest shared k-mer per position, every k in one pass (no counterpart in the reference) ----------
 * (Declared here, beside the `memo matrix` block: memo_amd.h keeps to the query path's 44 entry points.)
 * For the window [qs, qs + L), a cap CAP in [1, 2^31 - 1] and a row predicate -- mode 0: 0 <= annot < arg ("fewer than arg genomes
 * share it": a conservation index, arg = T), mode 1: annot == arg (a membership index, arg = the genome) --
 *     out[p - qs] = min( CAP, max( 0, min{ end_i - p : pred(annot_i), p < start_i, qs < start_i < qs + L + CAP } ) )       uint32
 * and CAP where no row bounds p.  For rows with end >= start: conservation(p, k) >= T, or bit G of the membership row of p, holds
 * exactly when k <= out[p - qs] (for k <= CAP).  Rows with end < start are legal and take the formula literally (the result can be
 * 0); for them equality with a per-k query is NOT promised.  annot is compared as the int64 it is.  Rows with start <= qs or
 * start >= qs + L + CAP are ignored by the kernel itself, whatever the caller passes; rows need not be sorted.
 *
 * d_cells is uint32 [L] on `device`, 16-byte aligned; the columns are device pointers, 8-byte aligned (MEMO_EINVAL otherwise, before
 * anything is launched; so are L > 2^31, CAP = 0 or above 2^31 - 1, |qs| > 2^61).  begin fills the cells with the identity
 * L - 1 + CAP; rows accumulates one chunk of rows into them (atomic min: any number of calls, any cut, any order -- the same cells);
 * finish turns the cells into out[] in place (scratch: 4 bytes per memo_maxk_tile() cells, freed before it returns; an allocation
 * that fails is MEMO_EHIP with the bytes asked for).  The same L and CAP go to all three.  L == 0 or rows == 0 launches nothing.
 * Nothing is read outside the `rows` elements of each column or outside d_cells[0 .. L).  Blocking (each synchronises `stream`). */
int memo_maxk_begin_dev(uint32_t *d_cells, int64_t L, uint32_t cap, int32_t device, void *stream);
int memo_maxk_rows_dev(const int64_t *d_start, const int64_t *d_end, const int64_t *d_annot, uint64_t rows, int64_t qs, int64_t L,
                       uint32_t cap, int32_t mode, int64_t arg, uint32_t *d_cells, int32_t device, void *stream);
int memo_maxk_finish_dev(uint32_t *d_cells, int64_t L, uint32_t cap, int32_t device, void *stream);
/* cells per tile of finish's scan, for tests that want lengths around it */
int32_t memo_maxk_tile(void);
/* the text of `memo maxk`: one decimal integer and '\n' per position; L <= 0 is no text at all.  Returns the number of bytes the
 * text needs; it is written only if it fits in cap (nothing is written past cap). */
size_t memo_emit_u32(const uint32_t *vec, int64_t L, char *buf, size_t cap);

/* ---- `memo lengths`: every genome's match length from a membership index, and the T-th largest (no counterpart in the reference) ----
 * (Declared here, beside the `memo maxk` block: memo_amd.h keeps to the query path's 44 entry points.)
 * For the window [qs, qs + L), num_docs = N genomes in [1, 2048] and a cap CAP in [1, 2^31 - 1] (memo_amd/csrc/memo_lengths.hip)
 *     len[g][p - qs] = min( CAP, max( 0, min{ end_i - p : annot_i = g, p < start_i, qs < start_i < qs + L + CAP } ) )     0 <= g < N
 *     sel_T[p - qs]  = the T-th largest of { len[g][p - qs] : 0 <= g < N }                                                  1 <= T <= N
 * and CAP where no row bounds p: len[g] is what the memo_maxk_*_dev calls give in mode 1 with arg = g, for every g in one pass over
 * the rows.  For rows with end >= start and k <= CAP: bit g of the membership row of p is set exactly when k <= len[g][p - qs], and
 * that row has at least T bits set exactly when k <= sel_T[p - qs].  Rows with end < start take the formula literally.  Rows whose
 * annot is outside [0, N) are ignored; rows need not be sorted.
 *
 * d_cells is uint32 [N][pitch] on `device`, genome-major: 16-byte aligned, pitch a multiple of 4 and at least L, N * pitch below 2^32.
 * The cells [L, pitch) of a plane are never read or written.  MEMO_EINVAL before anything is launched: the above, N outside [1, 2048],
 * L > 2^31, CAP = 0 or above 2^31 - 1, |qs| > 2^61, columns or a carry that are not 8-byte aligned, a threshold outside [1, N], a
 * d_out that is not 4-byte aligned.  L == 0 or rows == 0 launches nothing.  Nothing is read outside the `rows` elements of each
 * column.  Blocking (each call synchronises `stream`).
 *   begin   fills [0, L) of every plane with the identity L - 1 + CAP; with d_carry (int64 [N] on the device, INT64_MAX: none; NULL:
 *           no carry) cell L - 1 of plane g then holds carry[g] relative to qs, as if a row with that end started right of the window
 *   rows    accumulates one chunk of rows into the planes (one atomic min per row: any number of calls, any cut, any order, repeats)
 *   carry   d_carry[annot] = min(d_carry[annot], end) over the rows with lo < start < hi and 0 <= annot < N (the caller fills d_carry
 *           with INT64_MAX first).  With it a window runs in slices from the right, every row read once: seed the carry with the rows
 *           qe < start < qe + CAP; then for every slice [a, b): begin(qs = a, L = b - a, d_carry), rows with the rows a < start <= b,
 *           carry(lo = a, hi = b + 1) with the same rows, finish.  The planes of the slices laid end to end are the window's.
 *   finish  turns the cells into len[][] in place (scratch: 4 bytes per memo_lengths_tile() cells and plane, freed before it returns;
 *           an allocation that fails is MEMO_EHIP with the bytes asked for)
 *   select  d_out[i] = the threshold-th largest over g of min(d_cells[g][i], CAP), uint32 [L]; d_cells is not changed.  LDS: N rows of
 *           memo_lengths_select_tile(N) positions (with the kernel's static words at most 120 KiB). */
int memo_lengths_begin_dev(uint32_t *d_cells, int64_t L, int64_t pitch, int32_t num_docs, uint32_t cap, int64_t qs, const int64_t *d_carry,
                           int32_t device, void *stream);
int memo_lengths_rows_dev(const int64_t *d_start, const int64_t *d_end, const int64_t *d_annot, uint64_t rows, int64_t qs, int64_t L,
                          int64_t pitch, int32_t num_docs, uint32_t cap, uint32_t *d_cells, int32_t device, void *stream);
int memo_lengths_carry_dev(const int64_t *d_start, const int64_t *d_end, const int64_t *d_annot, uint64_t rows, int64_t lo, int64_t hi,
                           int32_t num_docs, int64_t *d_carry, int32_t device, void *stream);
int memo_lengths_finish_dev(uint32_t *d_cells, int64_t L, int64_t pitch, int32_t num_docs, uint32_t cap, int32_t device, void *stream);
int memo_lengths_select_dev(const uint32_t *d_cells, int64_t L, int64_t pitch, int32_t num_docs, uint32_t cap, int32_t threshold,
                            uint32_t *d_out, int32_t device, void *stream);
/* cells per tile of finish's scan, and positions per tile of select at num_docs genomes (256, 128 ... 8; 0: num_docs outside
 * [1, 2048]), for tests that want lengths around them */
int32_t memo_lengths_tile(void);
int32_t memo_lengths_select_tile(int32_t num_docs);
/* the text of `memo lengths -a`, HOST planes in (uint32 [n][pitch], genome-major; [0, L) of each is read): line p is
 * planes[0][p] ... planes[n - 1][p], blank-separated, and '\n'; L <= 0 or n <= 0 is no text at all.  Returns the number of bytes the text
 * needs; it is written only if it fits in cap (nothing is written past cap). */
size_t memo_emit_u32_rows(const uint32_t *planes, int64_t L, int64_t pitch, int32_t n, char *buf, size_t cap);
/* the threads memo_emit_u32_rows splits the lines of that shape over (one per 2^20 integers, at most the process's CPU budget or
 * MEMO_EMIT_THREADS, read per call; 0 for an empty text), for tests that want the threaded path and must know that they got it */
int32_t memo_emit_u32_rows_threads(int64_t L, int32_t n);

/* ---- `memo mems`: the maximal shared matches of a window, compacted on the device (no counterpart in the reference) -------------------
 * (Declared here, beside the `memo lengths` block: memo_amd.h keeps to the query path's 44 entry points.)
 * From finished lengths that are still on the device (memo_amd/csrc/memo_mems.hip): d_cells is uint32 [planes][pitch] on `device`, L
 * cells per plane read -- the planes of the memo_lengths_*_dev calls; the cells of the memo_maxk_*_dev calls and the output of
 * memo_lengths_select_dev are one plane.  With v the cells of one plane, a cap CAP in [1, 2^31 - 1] and min_len in [1, CAP]:
 *   key 1  cell i is reported when v[i] >= min_len and (i == 0 ? halo == 0 : v[i - 1] < v[i] || (v[i - 1] == v[i] && v[i] < CAP)):
 *          the matches that start in the plane, a run at CAP once, at its first cell.  halo = 0: cell 0 is position 0 of its record;
 *          halo = 1: cell 0 is only the neighbour of cell 1 and is never reported.  d_starts[r] = i, d_lengths[r] = v[i].
 *   key 2  the cells at which v[i] >= min_len changes, the cell before cell 0 counting as false: d_starts alone (d_lengths may be NULL
 *          and is set to NULL); in a plane 2j opens an interval, 2j + 1 closes it, an odd count leaves the last to end at L.  halo is 0.
 * The entries are plane-major and ascending within a plane; counts[pl] (a HOST array of `planes` entries) receives plane pl's number
 * of them.  *d_starts and *d_lengths are allocated on `device` to exactly the total (memo_dev_free; NULL where the total is 0); an
 * allocation that fails is MEMO_EHIP with the bytes asked for, and nothing stays allocated.  MEMO_EINVAL before anything is launched: a
 * key other than 1 or 2, a halo other than 0 or 1 or a halo with key 2, planes < 0, L < 0 or above 2^31, pitch < L, pitch % 4 != 0, CAP
 * or min_len outside their ranges, cells that are not 16-byte aligned, more than 2^31 - 1 tiles, an output that is NULL.  L == 0 or
 * planes == 0 launches nothing.  Nothing outside [0, L) of a plane is read: the cells [L, pitch) never are.  Blocking. */
int memo_mems_dev(const uint32_t *d_cells, int64_t L, int64_t pitch, int32_t planes, uint32_t cap, uint32_t min_len, int32_t key,
                  int32_t halo, uint32_t **d_starts, uint32_t **d_lengths, uint64_t *counts, int32_t device, void *stream);
/* cells per tile of the passes (a tile never crosses a plane), for tests that want lengths around it */
int32_t memo_mems_tile(void);
/* the text of `memo mems`: per entry record '\t' start '\t' end, and '\t' genome[i] where genome is not NULL, then '\n'; no entries is no
 * text at all.  Returns the number of bytes the text needs; it is written only if it fits in cap (nothing is written past cap). */
size_t memo_emit_intervals(const char *record, const int64_t *starts, const int64_t *ends, const int32_t *genome, uint64_t entries,
                           char *buf, size_t cap);

/* ---- `memo spectrum`: the conservation histogram of a window at every k, one pass (no counterpart in the reference) -----------------
 * (Declared here, beside the `memo lengths` block: memo_amd.h keeps to the query path's 44 entry points.)
 * From the finished planes of the memo_lengths_*_dev calls, run with cap = KMAX (memo_amd/csrc/memo_spectrum.hip): d_cells is uint32
 * [N][pitch] on `device`, genome-major, 16-byte aligned, pitch a multiple of 4 and at least L, N * pitch below 2^32; a cell above KMAX is
 * taken as KMAX; the cells [L, pitch) of a plane are never read.  With num_docs = N in [1, 2048] and KMAX in [1, 1024]
 *     sel_T[p]    = the T-th largest of d_cells[0 .. N)[p]                      mode 1: the planes of a membership index
 *     sel_T[p]    = min{ d_cells[a][p] : 0 <= a < T }                           mode 0: the planes of a conservation index (annot = plane)
 *     cons(p, k)  = max({ T : sel_T[p] >= k } + {0})                            1 <= k <= KMAX
 *     exact[k][v] = #{ p : cons(p, k) = v }                                     0 <= v <= N
 * For rows with end >= start exact[k] is the histogram of what `memo query -k k` writes for the window on a conservation index, and of
 * the one-bit counts of what `memo query -m -k k` writes on a membership index.
 *   scratch_bytes  the bytes of the scratch at that shape, (N + 1)(KMAX + 1) 64-bit counters (0: a shape outside the limits)
 *   begin          zeroes the scratch
 *   add            adds the L positions of one slice into the scratch; any number of calls, in any order; L == 0 launches nothing.  Every
 *                  call of one begin ... finish takes the same N, KMAX and mode.
 *   finish         writes d_exact, uint64 [KMAX][N + 1] on `device` (row k - 1 is k); the scratch is not changed, more adds may follow
 *   tile           positions per tile of add at that shape (mode 0: 256; mode 1: 256, 128, 64 or 32; 0: a shape or a mode outside the
 *                  limits), for tests that want lengths around it
 * MEMO_EINVAL before anything is launched: N outside [1, 2048], KMAX outside [1, 1024], a mode other than 0 or 1, L > 2^31, pitch < L,
 * pitch % 4 != 0, N * pitch >= 2^32, cells that are not 16-byte aligned, a scratch or a result that is NULL or not 8-byte aligned.
 * Blocking (each call synchronises `stream`). */
size_t memo_spectrum_scratch_bytes(int32_t num_docs, int32_t kmax);
int memo_spectrum_begin_dev(uint64_t *d_scratch, int32_t num_docs, int32_t kmax, int32_t device, void *stream);
int memo_spectrum_add_dev(const uint32_t *d_cells, int64_t L, int64_t pitch, int32_t num_docs, int32_t kmax, int32_t mode, uint64_t *d_scratch,
                          int32_t device, void *stream);
int memo_spectrum_finish_dev(const uint64_t *d_scratch, int32_t num_docs, int32_t kmax, uint64_t *d_exact, int32_t device, void *stream);
int32_t memo_spectrum_tile(int32_t num_docs, int32_t kmax, int32_t mode);

/* ---- `memo convert`: a conservation index from a membership index (no counterpart in the reference) ----------------------------------
 * (Declared here, after the `memo lengths` block: memo_amd.h keeps to the query path's 44 entry points.)
 * The step between the planes of the memo_lengths_*_dev calls and memo_dap_push_dev (memo_amd/csrc/memo_convert.hip): positions
 * [first, first + positions) of the genome-major planes d_cells (uint32 [N][pitch] on `device`, 16-byte aligned, pitch a multiple of 4)
 * become the position-major matrix the row builder reads, clipped at the end of the record, `remaining` positions from `first`:
 *     d_dap[i][g - 1] = min( d_cells[g][first + i], remaining - i )        0 <= i < positions, 1 <= g < N        int32 [positions][N - 1]
 * Plane 0, the pivot, is not read, and nothing outside [first, first + positions) of the other planes; nothing is written outside the
 * positions * (N - 1) integers of d_dap.  MEMO_EINVAL before anything is launched: N outside [2, 2048], pitch % 4 != 0,
 * first + positions > pitch, remaining < positions, remaining > 2^31 - 1, d_cells not 16-byte aligned, d_dap not 4-byte aligned, a
 * negative count.  positions == 0 launches nothing.  Blocking (synchronises `stream`). */
int memo_convert_dap_dev(const uint32_t *d_cells, int64_t pitch, int32_t num_docs, int64_t first, int64_t positions, int64_t remaining,
                         int32_t *d_dap, int32_t device, void *stream);
/* positions per tile of that kernel (tiles lie at multiples of it in the plane), for tests that want lengths around it */
int32_t memo_convert_tile(void);

/* ---- `memo add`: a membership index grown by new genomes, without the old ones (no counterpart in the reference) -----------------------
 * (Declared here, after the `memo convert` block: memo_amd.h keeps to the query path's 44 entry points.)
 * The row builder's matrix from two sources (memo_amd/csrc/memo_add.hip): the old genomes' columns from the planes d_cells exactly as
 * memo_convert_dap_dev takes them (uint32 [N][pitch] on `device`, 16-byte aligned, pitch a multiple of 4), the new genomes' columns from
 * d_new, int32 [positions][new_cols] on `device`, contiguous and 4-byte aligned (memo_ms_rows_dev), row i of it beside position first + i
 * of the planes.  With W = N - 1 + new_cols and room = remaining - i:
 *     d_dap[i][c] = min( d_cells[c + 1][first + i], room )                    0 <= c < N - 1         0 <= i < positions
 *     d_dap[i][c] = min( (uint32) d_new[i][c - (N - 1)], room )               N - 1 <= c < W         int32 [positions][W]
 * Plane 0 is not read, and nothing outside [first, first + positions) of the other planes; nothing is read outside d_new[0 ..
 * positions * new_cols); nothing is written outside the positions * W integers of d_dap, each of which is written once.  MEMO_EINVAL
 * before anything is launched: N outside [2, 2047], new_cols outside [1, 2047], W > 2047, pitch % 4 != 0, first + positions > pitch,
 * remaining < positions, remaining > 2^31 - 1, d_cells not 16-byte aligned, d_new or d_dap not 4-byte aligned, a negative count, a NULL
 * pointer with positions > 0.  positions == 0 launches nothing.  Blocking (synchronises `stream`). */
int memo_add_dap_dev(const uint32_t *d_cells, int64_t pitch, int32_t num_docs, int64_t first, int64_t positions, int64_t remaining,
                     const int32_t *d_new, int32_t new_cols, int32_t *d_dap, int32_t device, void *stream);
/* positions per tile of that kernel (tiles lie at multiples of it in the plane), for tests that want lengths around it */
int32_t memo_add_tile(void);

/* ---- `memo merge`: an index of chosen genomes from indexes on one pivot (no counterpart in the reference) ------------------------------
 * (Declared here, after the `memo add` block: memo_amd.h keeps to the query path's 44 entry points.)
 * The row builder's matrix through a column map (memo_amd/csrc/memo_merge.hip): d_cells holds `planes` planes stacked with one pitch
 * (uint32 [planes][pitch] on `device`, 16-byte aligned, pitch a multiple of 4: the blocks of several memo_lengths_*_dev runs one after
 * another), d_plane_of `cols` int32 on `device`, 4-byte aligned: the plane of every column.  With room = remaining - i:
 *     d_dap[i][c] = min( d_cells[d_plane_of[c]][first + i], room )            0 <= i < positions, 0 <= c < cols        int32 [positions][cols]
 * A plane may be named by any number of columns; nothing is skipped (the caller leaves the pivots' planes out of the map).  An entry
 * outside [0, planes) reads nothing and its column is 0: no content of the map makes the call read outside the planes.  Nothing is read
 * outside [first, first + positions) of a named plane or outside the `cols` entries of the map; nothing is written outside the
 * positions * cols integers of d_dap, each of which is written once.  MEMO_EINVAL before anything is launched: planes outside
 * [1, 65 536], cols outside [1, 2047], pitch % 4 != 0, first + positions > pitch, remaining < positions, remaining > 2^31 - 1, d_cells
 * not 16-byte aligned, d_plane_of or d_dap not 4-byte aligned, a negative count, a NULL pointer with positions > 0.  positions == 0
 * launches nothing.  Blocking (synchronises `stream`). */
int memo_merge_dap_dev(const uint32_t *d_cells, int64_t pitch, int32_t planes, const int32_t *d_plane_of, int32_t cols, int64_t first,
                       int64_t positions, int64_t remaining, int32_t *d_dap, int32_t device, void *stream);
/* positions per tile of that kernel (tiles lie at multiples of it in the plane), for tests that want lengths around it */
int32_t memo_merge_tile(void);

#ifdef __cplusplus
}
#endif
#endif /* MEMO_AMD_DAP_H */
