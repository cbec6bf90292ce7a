"""`memo breaks`: per genome and bin, how many maximal matches start there and what the match lengths sum to -- k-free.

No counterpart in the reference.  `memo tracks` and `memo features` draw which genome holds how much of a window at ONE k, and
presence saturates: at k = 31 a genome that is 99 % identical to the pivot and one that is 99.9 % look nearly alike, at k = 101 both
look empty.  The lengths v[p] that `memo lengths` and `memo maxk` leave in HBM do not saturate.  Where a genome's maximal match ends
and the next begins it differs from the pivot, so over the positions p of bin b

    table[0][g][b] = #{ p : v_g[p] >= min_len and p starts a match }      `memo mems`' rule: v[p - 1] < v[p], or v[p - 1] == v[p] < cap,
                                                                          or p is position 0 of its record
    table[1][g][b] = sum of v_g[p]                                        (divided by the bin's width: the mean match length)

table[0][g] is the histogram of the START column `memo mems -m -a -l MINLEN -K CAP` writes for genome g, table[1][g] is column g of
`memo lengths -a -K CAP` summed per bin; neither list leaves the device: memo_breaks_dev (memo_amd/csrc/memo_breaks.hip) reads the
finished planes once, where they lie, and 2 x R x B integers are downloaded.  Two sources of v:

    membership index                      the planes 0 .. N - 1 of memo_lengths_*_dev, slice by slice, each with its left neighbour
                                          (genome 0 is the pivot: nothing bounds it, its plane is the cap everywhere)
    conservation index, threshold=T       one plane, memo_maxk_*_dev mode 0: the stretches at least T genomes share

With a BED file the bins are the elementary segments between the features' endpoints (features.segments) and memo_feature_sums_dev
turns the segment table into one line per feature, as `memo features` does.  The flags are memo_amd/breaks_cli.py.
"""
import ctypes as C

import numpy as np

from ._device import DevBuffer, RowBuffer
from ._lib import check, lib
from ._window import parse_region
from .features import _feature_sums, batch_limit, segments
from .lengths import N_MAX, finished_slices, pitch_of, region_feed
from .maxk import CAP_MAX, Cells
from .tracks import region_edges

L_MAX = 2 ** 31 - 1
SUMS_ROWS = 2048                     # memo_feature_sums_dev's row limit: one call per half of the table


def tile():
    """cells per tile of the kernel: the lengths a test wants to straddle"""
    return int(lib().memo_breaks_tile())


def _edges(edges):
    edges = np.ascontiguousarray(edges, np.int64)
    if edges.ndim != 1 or len(edges) < 1:
        raise ValueError("edges must be a vector of bins + 1 positions")
    return edges


def _accumulate(d_cells, L, pitch, planes, cap, min_len, halo, first, edges, d_table, device, stream=None):
    check(lib().memo_breaks_dev(C.c_void_p(int(getattr(d_cells, "value", d_cells) or 0)), int(L), int(pitch), int(planes), int(cap), int(min_len),
                                int(halo), int(first), edges.ctypes.data, len(edges) - 1, d_table, device,
                                None if stream is None else C.c_void_p(int(stream))))


def plane_breaks(cells, edges, *, first=0, cap, min_len=1, halo=0, table=None, device=0, stream=None):
    """The kernel alone: `cells` is a host uint32 array [planes, L] (padded to the pitch and uploaded) or a (device pointer, L, pitch,
    planes) tuple of finished lengths.  With halo=1 cell 0 of every plane is only the left neighbour of cell 1; counted cell i is
    position first + i - halo, and `edges` are bins + 1 non-decreasing positions in the same coordinates that hold the slice.  Returns
    uint64 [2, planes, bins]: the match starts and the length sums; a `table` passed in is the starting value (the slices of a window
    accumulate)."""
    edges = _edges(edges)
    bins = len(edges) - 1
    padded = None
    if isinstance(cells, tuple):
        d_cells, L, pitch, planes = cells[0], int(cells[1]), int(cells[2]), int(cells[3])
    else:
        host = np.ascontiguousarray(cells, np.uint32)
        if host.ndim != 2:
            raise ValueError("cells must be [planes, L]")
        planes, L = host.shape
        pitch = pitch_of(L)
        padded = np.zeros((planes, pitch), np.uint32)
        padded[:, :L] = host
    shape = (2, max(planes, 0), bins)
    start = np.zeros(shape, np.uint64) if table is None else np.ascontiguousarray(table, np.uint64)
    if start.shape != shape:
        raise ValueError(f"table must be [2, {planes}, {bins}]")
    with DevBuffer(device, 0) if padded is None else DevBuffer.of(padded, device) as owner, DevBuffer.of(start, device) as d_table:
        _accumulate(d_cells if padded is None else owner.d, L, pitch, planes, cap, min_len, halo, first, edges, d_table.d, device, stream)
        return d_table.to_host(shape, np.uint64)


def _check(n_docs, membership, threshold, min_len, cap):
    """(n_docs, rows, threshold, min_len, cap), or a ValueError before any device call"""
    n_docs = int(n_docs)
    if not 1 <= n_docs <= N_MAX:
        raise ValueError(f"n_docs must be in [1, {N_MAX}]")
    if membership and threshold is not None:
        raise ValueError("a threshold cannot be combined with membership: the threshold-th largest of the genomes' lengths is not built")
    if not membership:
        threshold = n_docs if threshold is None else int(threshold)
        if not 1 <= threshold <= n_docs:
            raise ValueError(f"threshold must be in [1, {n_docs}]")
    cap = CAP_MAX if cap is None else int(cap)
    if not 1 <= cap <= CAP_MAX:
        raise ValueError(f"cap must be in [1, {CAP_MAX}]")
    if not 1 <= int(min_len) <= cap:
        raise ValueError(f"min_len must be in [1, {cap}]")
    return n_docs, (n_docs if membership else 1), threshold, int(min_len), cap


def _check_window(qs, L):
    if qs < 0:
        raise ValueError("the window starts before position 0 of the record")
    if L > L_MAX:
        raise ValueError(f"a window of at most {L_MAX} positions")


def _finished(index_path, record, qs, L, n_docs, membership, threshold, cap, device, slice_positions):
    """Yields (a, b, d_cells, L, pitch, planes, halo): the finished planes of every slice [a, b) of the window [qs, qs + L), L > 0,
    where they lie on the device; with halo = 1 cell 0 is position a - 1.  A membership index: all N planes, in slices from the
    right.  A conservation index: one plane for the whole window, as mems.region_mems builds it."""
    if membership:
        feed, buf = region_feed(index_path, record, device)
        with buf:
            for a, b, d_cells, pitch in finished_slices(feed, qs, L, n_docs, cap, device, slice_positions, halo=1):
                h = 1 if a > 0 else 0
                yield a, b, d_cells, b - a + h, pitch, n_docs, h
        return
    from . import memo_query
    h = 1 if qs > 0 else 0                       # the cell of position qs - 1: a neighbour only
    lo, Lh = qs - h, L + h
    with Cells(lo, Lh, cap, 0, threshold, device) as cells, RowBuffer(device) as buf:
        _, chunks = memo_query.region_chunks(index_path, record, lo, min(qs + L + cap, 2 ** 62))
        for cols in chunks:
            cells.add(*buf.upload(*cols))
        check(lib().memo_maxk_finish_dev(cells.d, Lh, cap, device, None))
        yield qs, qs + L, cells.d, Lh, pitch_of(Lh), 1, h


def _fill(d_table, index_path, record, edges, n_docs, membership, threshold, min_len, cap, device, slice_positions):
    """the window [edges[0], edges[-1]) into the device table [2][R][len(edges) - 1]; edges are absolute positions"""
    qs, L = int(edges[0]), int(edges[-1] - edges[0])
    for a, _, d_cells, Lc, pitch, planes, h in _finished(index_path, record, qs, L, n_docs, membership, threshold, cap, device, slice_positions):
        _accumulate(d_cells, Lc, pitch, planes, cap, min_len, h, a, edges, d_table, device)


def region_breaks(index_path, region, n_docs, n_bins, *, membership=False, threshold=None, min_len=1, cap=None, device=0,
                  slice_positions=None):
    """The match starts and the length sums of a window of a Parquet index, in n_bins bins (tracks.region_edges: `memo view`'s rule, so
    the columns line up with `memo tracks` and `memo view`).  With `membership` (a MEMBERSHIP index) one row per genome, genome 0
    the pivot; without it (a conservation index) one row: the stretches at least `threshold` genomes share (default n_docs).  `region`
    is CHR:START-END as `memo query -r` takes it, and what is wrong with it raises what memo_query.main raises.  cap=None: 2^31 - 1.
    slice_positions: the planes of a membership index are taken in slices of that many positions (the table does not depend on it).
    One device.  Returns (table uint64 [2, R, B], edges int64 [B + 1] from the window's start, qs); an empty window gives
    ([2, R, 0], [0], qs)."""
    n_docs, rows, threshold, min_len, cap = _check(n_docs, membership, threshold, min_len, cap)
    record, qs, qe = parse_region(region)
    _check_window(qs, qe - qs)
    if qe == qs and n_bins >= 1:
        return np.zeros((2, rows, 0), np.uint64), np.zeros(1, np.int64), qs
    edges = region_edges(qe - qs, int(n_bins))
    with DevBuffer.of(np.zeros((2, rows, n_bins), np.uint64), device) as d_table:
        _fill(d_table.d, index_path, record, edges + qs, n_docs, membership, threshold, min_len, cap, device, slice_positions)
        return d_table.to_host((2, rows, n_bins), np.uint64), edges, qs


def _batch(index_path, record, starts, ends, n_docs, rows, membership, threshold, min_len, cap, device, slice_positions):
    """the tables uint64 [2, F, R] of one batch of features with positions, all on `record`: one window, counted per segment, summed
    per feature on the device"""
    edges, lo, hi = segments(starts, ends)
    segs = len(edges) - 1
    _check_window(int(edges[0]), int(edges[-1] - edges[0]))
    out = np.empty((2, len(lo), rows), np.uint64)
    with DevBuffer.of(np.zeros((2, rows, segs), np.uint64), device) as d_table, DevBuffer(device, 8 * len(lo) * rows) as d_out:
        _fill(d_table.d, index_path, record, edges, n_docs, membership, threshold, min_len, cap, device, slice_positions)
        for half in range(2):
            _feature_sums(d_table.at(8 * half * rows * segs), rows, segs, lo, hi, d_out.d, device)
            out[half] = d_out.to_host((len(lo), rows), np.uint64)
    return out


def bed_breaks(index_path, bed, n_docs, *, membership=False, threshold=None, min_len=1, cap=None, device=0, slice_positions=None,
               batch_features=None):
    """The match starts and the length sums of a BED file's features (features.read_bed's result): (uint64 [2, F, R], positions
    int64 [F]) in file order, R as in region_breaks.  Record by record, the features with positions are sorted by start and cut into
    batches (features.batch_limit of 2 R rows); a batch is the window from its least start to its greatest end, counted per
    elementary segment between the features' endpoints where the planes lie and summed per feature on the device
    (memo_feature_sums_dev, once per half of the table).  Every feature is what region_breaks gives for it alone with one bin.  Gaps
    between the features of a batch are read like any other positions.  A feature of no positions touches no index.  One device."""
    n_docs, rows, threshold, min_len, cap = _check(n_docs, membership, threshold, min_len, cap)
    most = batch_limit(2 * rows, batch_features)
    starts, ends = bed.starts, bed.ends
    positions = ends - starts
    table = np.zeros((2, len(bed), rows), np.uint64)
    records = {}
    for f in np.flatnonzero(positions > 0).tolist():
        records.setdefault(bed.chroms[f], []).append(f)
    for record, members in records.items():
        members = np.asarray(members, np.int64)
        members = members[np.argsort(starts[members], kind="stable")]
        for at in range(0, len(members), most):
            batch = members[at:at + most]
            table[:, batch] = _batch(index_path, record, starts[batch], ends[batch], n_docs, rows, membership, threshold, min_len, cap,
                                     device, slice_positions)
    return table, positions
