"""`memo features`: for every feature of a BED file -- a gene, an exon, a sliding window -- which genomes hold it, or how conserved
it is, from one sweep per record instead of one process per feature.

No counterpart in the reference.  Features overlap, nest, repeat, come unsorted and lie on many records, so they are no bins for
`memo tracks`.  But the endpoints of a batch of F features cut their record into at most 2F - 1 elementary segments, which are:
the table is counted per segment where the sweep's result lies -- memo_tracks_dev with the segment edges as its bins for a
membership index, memo_segment_conservation_dev for a conservation index -- and memo_feature_sums_dev (both in
memo_amd/csrc/memo_features.hip) takes prefix sums along the segments and writes every feature as the difference of two of them:

    table[f][r] = sum of segment_table[r][s] over lo[f] <= s < hi[f]                                    uint64 [F, R]

R is N with a membership index (genome 0 is the pivot) and 2 with a conservation index (the sum of the values, the positions at or
above the threshold).  The segment table never leaves the device; F x R integers do.  The flags are memo_amd/features_cli.py.
"""
import ctypes as C
import re

import numpy as np

from ._device import DevBuffer, on_device
from ._lib import check, lib
from ._window import membership_slices

MAX_DOCS = 2048                      # memo_tracks_dev's
BATCH_FEATURES = 1 << 19             # at most 2^20 - 1 segments: inside memo_tracks_dev's 2^20 bins
SEGMENT_TABLE_BYTES = 2 << 30        # a batch's segment table holds at most this much (a condition, not a measurement)

_INT = re.compile(r"[+-]?[0-9]+\Z")


class Bed:
    """read_bed's result: the features of a BED file in file order"""

    def __init__(self, chroms, starts, ends, names):
        self.chroms, self.names = list(chroms), list(names)
        self.starts, self.ends = np.asarray(starts, np.int64).reshape(-1), np.asarray(ends, np.int64).reshape(-1)
        if not len(self.chroms) == len(self.names) == len(self.starts) == len(self.ends):
            raise ValueError("chroms, starts, ends and names differ in length")

    def __len__(self):
        return len(self.chroms)


def read_bed(path):
    """The features of a BED file: tab-separated `chrom start end [name ...]`, 0-based and half open.  Blank lines and lines that
    begin with `#`, `track` or `browser` are skipped, columns behind the name ignored, a missing name is `.`; start == end is a
    feature of no positions.  Fewer than three fields, a start or end that is no integer, a negative start, an end below its start:
    a ValueError that names the line."""
    chroms, starts, ends, names = [], [], [], []
    with open(path) as fh:
        for number, line in enumerate(fh, 1):
            line = line.rstrip("\r\n")
            if not line.strip() or line.startswith(("#", "track", "browser")):
                continue
            fields = line.split("\t")
            if len(fields) < 3:
                raise ValueError(f"{path}: line {number}: {len(fields)} tab-separated fields, a feature needs chrom, start and end")
            for what, text in (("start", fields[1]), ("end", fields[2])):
                if not _INT.match(text):
                    raise ValueError(f"{path}: line {number}: the {what} {text!r} is not an integer")
            start, end = int(fields[1]), int(fields[2])
            if start < 0:
                raise ValueError(f"{path}: line {number}: the start {start} is negative")
            if end < start:
                raise ValueError(f"{path}: line {number}: the end {end} is less than the start {start}")
            chroms.append(fields[0])
            starts.append(start)
            ends.append(end)
            names.append(fields[3] if len(fields) > 3 and fields[3] else ".")
    return Bed(chroms, starts, ends, names)


def segments(starts, ends):
    """(edges, lo, hi) of a batch of features [start, end): edges are the sorted distinct endpoints (int64), and feature f is the
    elementary segments lo[f] .. hi[f] - 1 between them (int32).  A feature of no positions has lo == hi."""
    starts, ends = np.asarray(starts, np.int64).reshape(-1), np.asarray(ends, np.int64).reshape(-1)
    if len(starts) != len(ends) or np.any(ends < starts):
        raise ValueError("every feature needs a start and an end that is not below it")
    edges = np.unique(np.concatenate([starts, ends]))
    return edges, np.searchsorted(edges, starts).astype(np.int32), np.searchsorted(edges, ends).astype(np.int32)


def segment_tile():
    """positions per tile of the segment kernel: the lengths a test wants to straddle"""
    return int(lib().memo_segment_conservation_tile())


def sums_tile():
    """segments per tile of the scan: the segment counts a test wants to straddle"""
    return int(lib().memo_feature_sums_tile())


def _stream(stream):
    return None if stream is None else C.c_void_p(int(stream))


def _segment_conservation(d_vec, L, first, edges, threshold, d_sums, device, stream=None):
    check(lib().memo_segment_conservation_dev(d_vec, L, first, edges.ctypes.data, len(edges) - 1, threshold, d_sums, device, _stream(stream)))


def _feature_sums(d_table, rows, segs, lo, hi, d_out, device, stream=None):
    check(lib().memo_feature_sums_dev(d_table, rows, segs, lo.ctypes.data, hi.ctypes.data, len(lo), d_out, device, _stream(stream)))


def segment_conservation(vec, edges, threshold, first=0, sums=None, device=0, stream=None):
    """The segment table of a conservation result: a host uint16 array [L], or (device pointer, L), holding the positions
    first .. first + L; `edges` are segs + 1 non-decreasing positions in the same coordinates.  Returns uint64 [2, segs]: the sum of
    the values and the number of values at or above `threshold` in every segment; a `sums` passed in is the starting value (the
    slices of a window accumulate)."""
    edges = np.ascontiguousarray(edges, np.int64)
    if edges.ndim != 1 or len(edges) < 1:
        raise ValueError("edges must be a vector of segs + 1 positions")
    segs = len(edges) - 1
    host = np.zeros((2, segs), np.uint64) if sums is None else np.ascontiguousarray(sums, np.uint64)
    if host.shape != (2, segs):
        raise ValueError(f"sums must be [2, {segs}]")
    with DevBuffer.of(host, device) as d_sums, on_device(vec, np.uint16, device) as (d_vec, L):
        _segment_conservation(d_vec, L, int(first), edges, int(threshold), d_sums.d, device, stream)
        return d_sums.to_host((2, segs), np.uint64)


def feature_sums(table, lo, hi, device=0, stream=None):
    """out[f][r] = table[r][lo[f]:hi[f]].sum() modulo 2^64, uint64 [F, rows]: `table` is a host uint64 array [rows, segs], or (device
    pointer, rows, segs) -- whose memory the call overwrites with prefix sums."""
    lo, hi = np.ascontiguousarray(lo, np.int32).reshape(-1), np.ascontiguousarray(hi, np.int32).reshape(-1)
    if len(lo) != len(hi):
        raise ValueError("lo and hi differ in length")
    if isinstance(table, tuple):
        pair, (rows, segs) = (table[0], 0), (int(table[1]), int(table[2]))
    else:
        pair = np.ascontiguousarray(table, np.uint64)
        if pair.ndim != 2:
            raise ValueError("table must be [rows, segs]")
        rows, segs = pair.shape
        pair = pair.reshape(-1)
    with on_device(pair, np.uint64, device) as (d_table, _), DevBuffer(device, max(8 * len(lo) * rows, 8)) as d_out:
        _feature_sums(d_table, rows, segs, lo, hi, d_out.d, device, stream)
        return d_out.to_host((len(lo), rows), np.uint64)


def feature_ranges(bed, k, inside=False):
    """(starts, ends) of the k-mer starts a feature counts: [start, end), or with `inside` the k-mers that lie wholly inside it,
    [start, max(start, end - k + 1))"""
    ends = np.maximum(bed.starts, bed.ends - (k - 1)) if inside else bed.ends
    return bed.starts, ends


def batch_limit(rows, batch_features=None):
    """features a batch holds at most: batch_features (default 2^19), and no more than keep the segment table of rows x 2F x 8 bytes
    inside SEGMENT_TABLE_BYTES"""
    most = BATCH_FEATURES if batch_features is None else int(batch_features)
    if not 1 <= most <= BATCH_FEATURES:
        raise ValueError(f"batch_features must be between 1 and {BATCH_FEATURES}")
    return max(1, min(most, SEGMENT_TABLE_BYTES // (16 * rows)))


def _batch(index_path, record, starts, ends, k, n_docs, membership, threshold, device, slice_positions):
    """the table uint64 [F, R] of one batch of features with positions, all on `record`: swept as one window, counted per segment,
    summed per feature on the device"""
    from . import memo_query
    edges, lo, hi = segments(starts, ends)
    qs, qe, segs = int(edges[0]), int(edges[-1]), len(edges) - 1
    rows = n_docs if membership else 2
    index = memo_query.region_index(index_path, record, qs, qe + k, device=device, k=k, num_docs=n_docs, membership=membership)
    with index, DevBuffer.of(np.zeros((rows, segs), np.uint64), device) as d_table, DevBuffer(device, 8 * len(lo) * rows) as d_out:
        if membership:
            for d_bits, s, e in membership_slices(index, qs, qe, k, n_docs, slice_positions, device):
                check(lib().memo_tracks_dev(d_bits, e - s, n_docs, s, edges.ctypes.data, segs, d_table.d, device, None))
        else:
            with DevBuffer(device, 2 * (qe - qs)) as vec:
                index.conservation_dev(qs, qe, k, n_docs, vec.d.value)
                index.check()
                _segment_conservation(vec.d, qe - qs, qs, edges, threshold, d_table.d, device)
        _feature_sums(d_table.d, rows, segs, lo, hi, d_out.d, device)
        return d_out.to_host((len(lo), rows), np.uint64)


def bed_features(index_path, bed, k, n_docs, membership=False, threshold=None, inside=False, device=0, slice_positions=1 << 24,
                 batch_features=None):
    """The table of a BED file's features (read_bed's result) from a Parquet index: uint64 [F, R] and the positions int64 [F] every
    feature counts, in file order.  With `membership` (a MEMBERSHIP index) R = N and table[f][g] is the number of the feature's
    positions at which genome g holds the pivot's k-mer; without it (a conservation index) R = 2: the sum of the conservation
    values over the feature's positions, and the positions whose value is at least `threshold` (default N).

    Record by record, the features with positions are sorted by start and cut into batches (batch_limit).  A batch is swept as the
    window [its least start, its greatest end) -- in slices of at most `slice_positions` through one reused buffer with
    `membership`, in one conservation sweep without -- so the answers are what `memo query [-m] -k K` writes for that window,
    restricted to each feature, and what is wrong with it raises what memo_query.main raises.  Gaps between the features of a batch
    are swept like any other positions.  A feature of no positions touches no index.  One device."""
    if k < 1:
        raise ValueError(f"k must be at least 1 (got {k})")
    if membership and not 1 <= n_docs <= MAX_DOCS:
        raise ValueError(f"a membership table holds at most {MAX_DOCS} genomes (got {n_docs})")
    if membership and threshold is not None:
        raise ValueError("a threshold has no meaning with a membership index")
    threshold = n_docs if threshold is None else int(threshold)
    if not membership and not 1 <= threshold <= n_docs:
        raise ValueError(f"the threshold must be between 1 and {n_docs} (got {threshold})")
    rows = n_docs if membership else 2
    most = batch_limit(rows, batch_features)
    starts, ends = feature_ranges(bed, k, inside)
    positions = ends - starts
    table = np.zeros((len(bed), rows), np.uint64)
    records = {}
    for f in np.flatnonzero(positions > 0).tolist():
        records.setdefault(bed.chroms[f], []).append(f)
    for record, members in records.items():
        members = np.asarray(members, np.int64)
        members = members[np.argsort(starts[members], kind="stable")]
        for at in range(0, len(members), most):
            batch = members[at:at + most]
            table[batch] = _batch(index_path, record, starts[batch], ends[batch], k, n_docs, membership, threshold, device, slice_positions)
    return table, positions


def shares(table, positions):
    """table / positions, float64 [F, R]; nan where a feature has no positions"""
    positions = np.asarray(positions, np.float64)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(positions > 0, np.asarray(table).astype(np.float64) / positions, np.nan)


def calls(table, positions, fraction):
    """the presence/absence matrix uint8 [F, R]: 1 where positions > 0 and count >= fraction * positions, in float64"""
    positions = np.asarray(positions, np.float64)[:, None]
    return ((positions > 0) & (np.asarray(table).astype(np.float64) >= float(fraction) * positions)).astype(np.uint8)


def format_features(bed, positions, table, membership, labels=None):
    """tab-separated text, one line per feature in file order behind a header: `chrom start end name positions`, then the table's
    columns -- with `membership` one per genome, named by annot number (0 is the pivot) or by label; without it `sum shared`, or
    `mean shared_fraction` for a table of floats -- integers as they are, floats by repr (nan: `nan`).  The table is bed_features',
    or shares() or calls() of it."""
    table = np.asarray(table)
    if table.ndim != 2 or len(table) != len(bed) or len(positions) != len(bed):
        raise ValueError(f"a table of {table.shape} and {len(positions)} positions for {len(bed)} features")
    floats = table.dtype.kind == "f"
    if membership:
        columns = [str(g) for g in range(table.shape[1])] if labels is None else list(labels)
        if len(columns) != table.shape[1]:
            raise ValueError(f"{len(columns)} labels for {table.shape[1]} genomes")
    else:
        if labels is not None:
            raise ValueError("labels name genomes: a conservation table has none")
        if table.shape[1] != 2:
            raise ValueError(f"a conservation table has two columns, not {table.shape[1]}")
        columns = ["mean", "shared_fraction"] if floats else ["sum", "shared"]
    cell = (lambda v: repr(float(v))) if floats else (lambda v: str(int(v)))
    lines = ["\t".join(["chrom", "start", "end", "name", "positions"] + columns)]
    for f, row in enumerate(table.tolist()):
        lines.append("\t".join([bed.chroms[f], str(int(bed.starts[f])), str(int(bed.ends[f])), bed.names[f], str(int(positions[f]))]
                               + [cell(v) for v in row]))
    return "".join(line + "\n" for line in lines)
