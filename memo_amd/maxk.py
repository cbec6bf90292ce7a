"""`memo maxk`: the longest shared k-mer per position, every k in one pass on the GPU.

No counterpart in the reference, which answers one k per query.  The index holds the answer for all of them: a row (s, e, a) with
e >= s makes the k-mer at p absent for order / genome a exactly when p < s and p + k - 1 >= e, so for a row predicate `pred`

    out[p - qs] = min( cap, max( 0, min{ e_i - p : pred(a_i), p < s_i, qs < s_i < qe + cap } ) )        uint32, cap where no row bounds p

is the largest k (up to cap) at which the k-mer at p still is shared: with threshold=T (a conservation index, pred: 0 <= a < T)
conservation(p, k) >= T exactly when k <= out[p - qs]; with genome=G (a membership index, pred: a == G) genome G holds the k-mer
at p exactly when k <= out[p - qs].  That is promised for rows with e >= s; rows with e < s are legal and take the formula
literally (the result can be 0), and equality with a per-k `memo query` is NOT promised for them.

memo_amd/csrc/memo_maxk.hip: the cells are filled with the identity, every chunk of rows is folded into them with atomic mins,
one per run of rows that hit the same cell (any order, any cut into chunks), a reverse min-scan turns them into the result in place; 4 L bytes leave the device.
The flags are memo_amd/maxk_cli.py.
"""
import numpy as np

from ._device import DevBuffer, RowBuffer, emit_text
from ._lib import check, lib
from ._window import parse_region

CAP_MAX = 2 ** 31 - 1


def tile():
    """cells per tile of the reverse scan: the lengths a test wants to straddle"""
    return int(lib().memo_maxk_tile())


def _predicate(threshold, genome):
    """(mode, arg) of memo_maxk_rows_dev"""
    if (threshold is None) == (genome is None):
        raise ValueError("exactly one of threshold (conservation index) and genome (membership index) must be given")
    return (0, int(threshold)) if genome is None else (1, int(genome))


def window(qs, qe, cap):
    """(qs, L, cap) as integers, or the ValueError of a reversed window and then of a cap outside [1, CAP_MAX]"""
    qs, qe, cap = int(qs), int(qe), int(cap)
    if qe < qs:
        raise ValueError("negative dimensions are not allowed")          # as `memo query` raises it
    if not 1 <= cap <= CAP_MAX:
        raise ValueError(f"cap must be in [1, {CAP_MAX}]")
    return qs, qe - qs, cap


class Cells:
    """uint32 [L] on the device between memo_maxk_begin_dev and memo_maxk_finish_dev"""

    def __init__(self, qs, L, cap, mode, arg, device):
        self.qs, self.L, self.cap, self.mode, self.arg, self.device = qs, L, cap, mode, arg, device
        self.buf = DevBuffer(device, 4 * L)
        try:
            check(lib().memo_maxk_begin_dev(self.d, L, cap, device, None))
        except BaseException:
            self.close()
            raise

    @property
    def d(self):
        return self.buf.d

    def add(self, d_start, d_end, d_annot, rows):
        """one chunk of rows, device columns"""
        check(lib().memo_maxk_rows_dev(d_start, d_end, d_annot, rows, self.qs, self.L, self.cap, self.mode, self.arg, self.d,
                                       self.device, None))

    def finish(self):
        """the result, uint32 [L] on the host"""
        check(lib().memo_maxk_finish_dev(self.d, self.L, self.cap, self.device, None))
        return self.buf.to_host(self.L, np.uint32)

    def close(self):
        self.buf.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def maxk(start, end, annot, qs, qe, *, threshold=None, genome=None, cap=CAP_MAX, device=0, chunk_rows=None):
    """The longest shared k per position of [qs, qe) from host columns (any order; rows outside qs < start < qe + cap are ignored
    by the kernel).  chunk_rows: feed the rows in calls of that many (the result does not depend on it).  Returns uint32 [qe - qs]."""
    mode, arg = _predicate(threshold, genome)
    qs, L, cap = window(qs, qe, cap)
    cols = [np.ascontiguousarray(c, np.int64) for c in (start, end, annot)]
    n = len(cols[0])
    step = n if not chunk_rows else int(chunk_rows)
    with Cells(qs, L, cap, mode, arg, device) as cells, RowBuffer(device) as buf:
        for at in range(0, n, max(step, 1)):
            cells.add(*buf.upload(*(c[at:at + step] for c in cols)))
        return cells.finish()


def index_maxk(index, qs, qe, *, threshold=None, genome=None, cap=CAP_MAX):
    """The same from a DeviceIndex that still has its int64 columns: the rows are read where they lie.  memo_index_columns hands the
    columns out as writable, which drops what the index derived from them (bucket table, packed rows, views): the index is
    finalized again before this returns, and packs again when it is asked to."""
    mode, arg = _predicate(threshold, genome)
    qs, L, cap = window(qs, qe, cap)
    d_s, d_e, d_o = index.columns()
    try:
        with Cells(qs, L, cap, mode, arg, index.device) as cells:
            cells.add(d_s, d_e, d_o, index.rows)
            return cells.finish()
    finally:
        index.finalize()


def region_maxk(index_path, region, n_docs, threshold=None, genome=None, cap=CAP_MAX, device=0):
    """The longest shared k per position of a window of a Parquet index: the rows with qs < start < qe + cap stream out of the file
    row group by row group (memo_query.region_chunks), each chunk goes into one reused device buffer and is folded into the cells.
    The device holds one chunk of rows and 4 L bytes of cells.  No sidecar cache is read or built: the packed rows do not hold
    `end`.  threshold=None and genome=None: threshold = n_docs (shared by all).  `region` is CHR:START-END as `memo query -r` takes
    it, and what is wrong with it raises what memo_query.main raises.  One device.  Returns uint32 [qe - qs]."""
    from . import memo_query
    if threshold is None and genome is None:
        threshold = n_docs
    mode, arg = _predicate(threshold, genome)
    record, qs, qe = parse_region(region)
    qs, L, cap = window(qs, qe, cap)
    with Cells(qs, L, cap, mode, arg, device) as cells, RowBuffer(device) as buf:
        if L:
            _, chunks = memo_query.region_chunks(index_path, record, qs, min(qe + cap, 2 ** 62))
            for cols in chunks:
                cells.add(*buf.upload(*cols))
        return cells.finish()


def emit(vec):
    """the text of a result, one integer per line, as a uint8 array (write it with fh.write(memoryview(buf))); empty for L = 0"""
    vec = np.ascontiguousarray(vec, np.uint32)
    return emit_text(lambda buf, cap: lib().memo_emit_u32(vec.ctypes.data, len(vec), buf, cap))
