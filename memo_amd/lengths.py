"""`memo lengths`: from a membership index, how far every genome matches the pivot from every position, and the T-th largest of
those lengths -- "up to which k do at least T genomes hold this k-mer" -- every k in one pass over the rows, on the GPU.

No counterpart in the reference.  With N genomes, a window [qs, qe) and a cap (memo_amd/csrc/memo_lengths.hip)

    len[g][p - qs] = min( cap, max( 0, min{ e_i - p : a_i = g, p < s_i, qs < s_i < qe + cap } ) )        0 <= g < N, cap where no row bounds p
    sel_T[p - qs]  = the T-th largest of { len[g][p - qs] : 0 <= g < N }                                  1 <= T <= N

len[g] is maxk.maxk(genome=g); all of them come out of ONE pass over the rows.  For rows with e >= s and k <= cap, bit g of the
`memo query -m -k k` row at p is set exactly when k <= len[g][p - qs], and that row has at least T bits set exactly when
k <= sel_T[p - qs].  Rows with e < s take the formula literally; annots outside [0, N) are ignored.  Genome 0, the pivot, has no rows
in an index that `memo index` writes: its plane is cap everywhere and counts in the selection like any other.

The device holds uint32 [N][pitch] cells for one SLICE of the window at a time.  The slices are taken from the right; an int64 carry
per genome (the smallest end among the rows right of the slice) takes the place of the rows a slice does not see, so a slice needs
only its own rows, every row is read once, and the result never depends on the slicing or on the cut into chunks.  A Parquet
window asks the file for the tail and for every slice's rows (a row group that straddles a slice bound is decoded for both
slices); host columns of a sliced window are sorted by start once and cut at the slice bounds.  The flags are memo_amd/lengths_cli.py.
"""
import numpy as np

from ._device import DevBuffer, RowBuffer, emit_text
from ._lib import check, lib
from ._window import parse_region
from .maxk import CAP_MAX, window

N_MAX = 2048
_NO_CARRY = np.iinfo(np.int64).max


def tile():
    """cells per tile of the reverse scan: the lengths a test wants to straddle"""
    return int(lib().memo_lengths_tile())


def select_tile(n_docs):
    """positions per tile of the selection at n_docs genomes"""
    return int(lib().memo_lengths_select_tile(int(n_docs)))


def pitch_of(L):
    """cells per plane of L positions: the next multiple of 4"""
    return (L + 3) & ~3


def docs(n_docs, threshold=None):
    """n_docs as an integer of [1, N_MAX], a threshold checked against it"""
    n_docs = int(n_docs)
    if not 1 <= n_docs <= N_MAX:
        raise ValueError(f"n_docs must be in [1, {N_MAX}]")
    if threshold is not None and not 1 <= int(threshold) <= n_docs:
        raise ValueError(f"threshold must be in [1, {n_docs}]")
    return n_docs


def default_slice_positions(n_docs):
    """the positions per slice that keep the cells, 4 N pitch bytes, within 2 GiB"""
    return max((2 ** 29 // int(n_docs)) & ~3, 4)


def window_slices(qs, L, n_docs, slice_positions):
    """[(a, b), ...]: the window cut at multiples of the slice length, from the right"""
    step = default_slice_positions(n_docs) if slice_positions is None else int(slice_positions)
    if step < 1:
        raise ValueError("slice_positions must be at least 1")
    return [(qs + at, qs + min(at + step, L)) for at in range(0, L, step)][::-1]


def finished_slices(feed, qs, L, n_docs, cap, device, slice_positions, halo=0):
    """Yields (a, b, d_cells, pitch) for every slice [a, b) of the window, from the right, its planes finished on the device (they
    are the next slice's cells once the consumer comes back).  feed(lo, hi) yields (d_start, d_end, d_annot, rows) chunks of device
    columns that hold at least the rows with lo < start < hi.  halo=1: every slice with a > 0 has one more cell on its left, the
    true lengths of position a - 1 (its planes begin at a - 1: the slice is begun there and fed the rows a - 1 < start <= b, the carry
    still takes the rows a < start <= b); a slice at a = 0 has nothing on its left and none."""
    if halo not in (0, 1):
        raise ValueError("halo must be 0 or 1")
    qe = qs + L
    slices = window_slices(qs, L, n_docs, slice_positions)
    if not slices:
        return
    L_ = lib()
    longest = max(b - a for a, b in slices) + halo
    with DevBuffer(device, 4 * n_docs * pitch_of(longest)) as cells, DevBuffer(device, 8 * n_docs if len(slices) > 1 else 0) as carry:
        reach = min(qe + cap, 2 ** 62)
        if len(slices) == 1:            # the whole window: the row pass itself takes qs < start < qe + cap
            h = halo if qs > 0 else 0
            check(L_.memo_lengths_begin_dev(cells.d, L + h, pitch_of(L + h), n_docs, cap, qs - h, None, device, None))
            for chunk in feed(qs - h, reach):
                check(L_.memo_lengths_rows_dev(*chunk, qs - h, L + h, pitch_of(L + h), n_docs, cap, cells.d, device, None))
            check(L_.memo_lengths_finish_dev(cells.d, L + h, pitch_of(L + h), n_docs, cap, device, None))
            yield qs, qe, cells.d, pitch_of(L + h)
            return
        none = np.full(n_docs, _NO_CARRY, np.int64)
        check(L_.memo_dev_upload(device, carry.d, none.ctypes.data, none.nbytes, None))
        for chunk in feed(qe, reach):   # the tail: the rows right of the window
            check(L_.memo_lengths_carry_dev(*chunk, qe, reach, n_docs, carry.d, device, None))
        for a, b in slices:             # before [a, b) the carry holds the rows with b < start < qe + cap
            h = halo if a > 0 else 0
            Ls, pitch = b - a + h, pitch_of(b - a + h)
            check(L_.memo_lengths_begin_dev(cells.d, Ls, pitch, n_docs, cap, a - h, carry.d, device, None))
            for chunk in feed(a - h, b + 1):
                check(L_.memo_lengths_rows_dev(*chunk, a - h, Ls, pitch, n_docs, cap, cells.d, device, None))
                check(L_.memo_lengths_carry_dev(*chunk, a, b + 1, n_docs, carry.d, device, None))
            check(L_.memo_lengths_finish_dev(cells.d, Ls, pitch, n_docs, cap, device, None))
            yield a, b, cells.d, pitch


def host_feed(start, end, annot, chunk_rows, device, whole):
    """(feed, buffer) of host columns.  Asked for `whole` = (qs, qe + cap), the bounds of a window of one slice, the feed hands over
    every row as it lies, in chunks of chunk_rows (the row pass filters; a single chunk is uploaded once).  Asked for anything
    narrower -- the tail or one slice of a sliced window -- it hands over exactly the rows with lo < start < hi: the columns are
    sorted by start once (a stable sort of a host copy), and every row is uploaded for its own slice and no other."""
    cols = [np.ascontiguousarray(c, np.int64) for c in (start, end, annot)]
    n = len(cols[0])
    if len(cols[1]) != n or len(cols[2]) != n:
        raise ValueError("start, end and annot differ in length")
    step = max(n if not chunk_rows else int(chunk_rows), 1)
    buf = RowBuffer(device)
    by_start = []

    def feed(lo, hi):
        if (lo, hi) == whole:
            first, last, source = 0, n, cols
        else:
            if not by_start:
                order = np.argsort(cols[0], kind="stable")
                by_start.extend(c[order] for c in cols)
            first, last = (int(np.searchsorted(by_start[0], v, side)) for v, side in ((lo, "right"), (hi, "left")))
            source = by_start
        for at in range(first, last, step):
            yield buf.upload(*(c[at:min(at + step, last)] for c in source))
    return feed, buf


def region_feed(index_path, record, device):
    from . import memo_query
    buf = RowBuffer(device)

    def feed(lo, hi):
        _, chunks = memo_query.region_chunks(index_path, record, lo, hi)
        for cols in chunks:
            yield buf.upload(*cols)
    return feed, buf


def _download_planes(out, qs, a, b, d_cells, pitch, n_docs, device):
    part = np.empty((n_docs, pitch), np.uint32)
    check(lib().memo_dev_download(device, part.ctypes.data, d_cells, part.nbytes, None))
    out[:, a - qs:b - qs] = part[:, :b - a]


def _planes(feed, buf, qs, L, n_docs, cap, device, slice_positions):
    out = np.empty((n_docs, L), np.uint32)
    with buf:
        for a, b, d_cells, pitch in finished_slices(feed, qs, L, n_docs, cap, device, slice_positions):
            _download_planes(out, qs, a, b, d_cells, pitch, n_docs, device)
    return out


def _kth(feed, buf, qs, L, n_docs, threshold, cap, device, slice_positions):
    with buf, DevBuffer(device, 4 * L) as d_out:
        for a, b, d_cells, pitch in finished_slices(feed, qs, L, n_docs, cap, device, slice_positions):
            check(lib().memo_lengths_select_dev(d_cells, b - a, pitch, n_docs, cap, threshold, d_out.at(4 * (a - qs)), device, None))
        return d_out.to_host(L, np.uint32)


def planes(start, end, annot, qs, qe, n_docs, *, cap=CAP_MAX, device=0, chunk_rows=None, slice_positions=None):
    """Every genome's match length per position of [qs, qe) from host columns (any order; the kernels ignore the rows outside
    qs < start < qe + cap and the annots outside [0, n_docs)).  chunk_rows: feed the rows in calls of that many; slice_positions: take
    the window in slices of that many positions (the result depends on neither; a sliced window sorts a copy of the rows by start
    and gives every slice its own).  Returns uint32 [n_docs, qe - qs]."""
    n_docs = docs(n_docs)
    qs, L, cap = window(qs, qe, cap)
    feed, buf = host_feed(start, end, annot, chunk_rows, device, (qs, min(qs + L + cap, 2 ** 62)))
    return _planes(feed, buf, qs, L, n_docs, cap, device, slice_positions)


def kth(start, end, annot, qs, qe, n_docs, *, threshold, cap=CAP_MAX, device=0, chunk_rows=None, slice_positions=None):
    """The threshold-th largest of the genomes' match lengths per position: the largest k (up to cap) at which at least `threshold`
    genomes hold the k-mer.  The planes stay on the device; 4 (qe - qs) bytes leave it.  Returns uint32 [qe - qs]."""
    n_docs = docs(n_docs, threshold)
    qs, L, cap = window(qs, qe, cap)
    feed, buf = host_feed(start, end, annot, chunk_rows, device, (qs, min(qs + L + cap, 2 ** 62)))
    return _kth(feed, buf, qs, L, n_docs, int(threshold), cap, device, slice_positions)


def select(planes, threshold, cap=CAP_MAX, device=0):
    """The selection kernel alone on host values: the threshold-th largest over the rows of `planes` (uint32 [N, L]; values above cap
    are taken as cap) per column.  Returns uint32 [L]."""
    planes = np.asarray(planes, np.uint32)
    if planes.ndim != 2:
        raise ValueError("planes must be [n_docs, positions]")
    n_docs = docs(planes.shape[0], threshold)
    L, cap = planes.shape[1], int(cap)
    if not 1 <= cap <= CAP_MAX:
        raise ValueError(f"cap must be in [1, {CAP_MAX}]")
    pitch = pitch_of(L)
    padded = np.zeros((n_docs, pitch), np.uint32)
    padded[:, :L] = planes
    with DevBuffer(device, padded.nbytes) as cells, DevBuffer(device, 4 * L) as d_out:
        if L:
            check(lib().memo_dev_upload(device, cells.d, padded.ctypes.data, padded.nbytes, None))
        check(lib().memo_lengths_select_dev(cells.d, L, pitch, n_docs, cap, int(threshold), d_out.d, device, None))
        return d_out.to_host(L, np.uint32)


def region_window(region, cap):
    """(record, qs, L, cap) of CHR:START-END and a cap: parse_region's refusals, then maxk.window's"""
    record, qs, qe = parse_region(region)
    return (record, *window(qs, qe, cap))


def region_slices(index_path, region, n_docs, cap=CAP_MAX, device=0, slice_positions=None, halo=0):
    """The planes of a window of a Parquet membership index, slice by slice FROM THE RIGHT: yields (a, b, uint32 [n_docs, b - a]);
    with halo=1 a slice with a > 0 has the lengths of position a - 1 as one more column on its left.
    The rows stream out of the file row group by row group (memo_query.region_chunks: first the tail qe < start < qe + cap, then
    every slice's own rows), each chunk through one reused device buffer.  No sidecar cache is read or built."""
    n_docs = docs(n_docs)
    record, qs, L, cap = region_window(region, cap)
    feed, buf = region_feed(index_path, record, device)
    with buf:
        for a, b, d_cells, pitch in finished_slices(feed, qs, L, n_docs, cap, device, slice_positions, halo):
            h = halo if a > 0 else 0
            part = np.empty((n_docs, b - a + h), np.uint32)
            _download_planes(part, a - h, a - h, b, d_cells, pitch, n_docs, device)
            yield a, b, part


def region_planes(index_path, region, n_docs, cap=CAP_MAX, device=0, slice_positions=None):
    """Every genome's match length per position of a window of a Parquet membership index.  `region` is CHR:START-END as
    `memo query -r` takes it, and what is wrong with it raises what memo_query.main raises.  One device.  Returns uint32 [n_docs, qe - qs]."""
    n_docs = docs(n_docs)
    record, qs, L, cap = region_window(region, cap)
    feed, buf = region_feed(index_path, record, device)
    return _planes(feed, buf, qs, L, n_docs, cap, device, slice_positions)


def region_kth(index_path, region, n_docs, threshold=None, cap=CAP_MAX, device=0, slice_positions=None):
    """The threshold-th largest match length per position of a window of a Parquet membership index (threshold=None: n_docs, held by
    all).  Returns uint32 [qe - qs]."""
    threshold = n_docs if threshold is None else threshold
    n_docs = docs(n_docs, threshold)
    record, qs, L, cap = region_window(region, cap)
    feed, buf = region_feed(index_path, record, device)
    return _kth(feed, buf, qs, L, n_docs, int(threshold), cap, device, slice_positions)


def emit_rows(planes):
    """the text of planes (uint32 [N, L]): line p is planes[0][p] ... planes[N - 1][p], blank-separated, as a uint8 array; empty for L = 0"""
    planes = np.ascontiguousarray(planes, np.uint32)
    if planes.ndim != 2:
        raise ValueError("planes must be [n_docs, positions]")
    n, L = planes.shape
    return emit_text(lambda buf, cap: lib().memo_emit_u32_rows(planes.ctypes.data, L, L, n, buf, cap))
