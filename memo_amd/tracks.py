"""`memo tracks`: every genome's k-mer presence along the pivot, binned on the GPU.

No counterpart in the reference, whose one picture (`memo view`) is drawn from a conservation index, every genome folded into
one number per position.  This is the membership counterpart: the sweep's result stays in HBM, memo_tracks_dev
(memo_amd/csrc/memo_tracks.hip) counts, for every genome and every bin, the positions of the bin at which the genome holds the
pivot's k-mer, and only N x B integers leave the device:

    counts[g][b] = #{ p in [edges[b], edges[b + 1]) : bit[p][g] = 1 }        uint64 [N, B]

Genome 0 is the pivot (dap_to_bed.py:113 numbers the others from 1).  The bins are `memo view`'s (view.bin_edges: the reference's
linspace rule), so the columns line up with its bars for the same window and bin count.  A whole window is swept in slices into
one reused result buffer and accumulated (region_tracks), so its membership result never exists as a whole.  The flags are
memo_amd/tracks_cli.py.
"""
import ctypes as C

import numpy as np

from ._device import DevBuffer, on_device
from ._lib import check, lib
from ._window import membership_slices, parse_region
from .index import words
from .view import bin_edges


def tile(words_per_position=1):
    """positions per tile of the kernel: the lengths a test wants to straddle"""
    return int(lib().memo_tracks_tile(int(words_per_position)))


def _accumulate(d_bits, L, num_docs, first, edges, d_counts, device, stream=None):
    check(lib().memo_tracks_dev(d_bits, L, num_docs, first, edges.ctypes.data, len(edges) - 1, d_counts, device,
                                None if stream is None else C.c_void_p(int(stream))))


def _edges(edges):
    edges = np.ascontiguousarray(edges, np.int64)
    if edges.ndim != 1 or len(edges) < 1:
        raise ValueError("edges must be a vector of bins + 1 positions")
    return edges


def _table(num_docs, bins, counts):
    """`counts` as a host table uint64 [N, B] (None: zeros)"""
    host = np.zeros((num_docs, bins), np.uint64) if counts is None else np.ascontiguousarray(counts, np.uint64)
    if host.shape != (num_docs, bins):
        raise ValueError(f"counts must be [{num_docs}, {bins}]")
    return host


def bin_tracks(bits, num_docs, edges, first=0, counts=None, device=0, stream=None):
    """The presence counts of a membership result: a host uint32 array [L, W], or (device pointer, L), holding the positions
    first .. first + L; `edges` are bins + 1 non-decreasing positions in the same coordinates.  Returns uint64 [N, B]; a `counts`
    passed in is the starting value (the slices of a window accumulate)."""
    W = words(num_docs)
    edges = _edges(edges)
    if not isinstance(bits, tuple):
        bits = np.ascontiguousarray(bits, np.uint32).reshape(-1, W)
    bins = len(edges) - 1
    with DevBuffer.of(_table(num_docs, bins, counts), device) as d_counts, on_device(bits, np.uint32, device) as (d_bits, L):
        _accumulate(d_bits, L, num_docs, int(first), edges, d_counts.d, device, stream)
        return d_counts.to_host((num_docs, bins), np.uint64)


class Tracks(tuple):
    """region_tracks' result: the pair (counts, edges), and the window's start as .qs"""

    def __new__(cls, counts, edges, qs):
        self = super().__new__(cls, (counts, edges))
        self.qs = qs
        return self


def region_edges(positions, n_bins):
    """the bin edges of a window of `positions` positions, from 0: `memo view`'s; fewer than one bin or more bins than positions is
    a ValueError (an empty bin has no fraction)"""
    if n_bins < 1 or n_bins > positions:
        raise ValueError(f"{n_bins} bins for a window of {positions} positions: the number of bins must be between 1 and the positions")
    return bin_edges(positions, n_bins)


def region_tracks(index_path, region, k, n_docs, n_bins, device=0, slice_positions=1 << 24):
    """The presence counts of a window of a Parquet MEMBERSHIP index, in n_bins bins: the window is swept in slices of at most
    `slice_positions` into one reused device buffer of slice_positions x W x 4 bytes, each slice is accumulated into one device
    table, and N x B x 8 bytes are downloaded at the end.  A slice is swept as part of its window (membership_slice_dev), so the
    table does not depend on the slices.  `region` is CHR:START-END as `memo query -r` takes it, and what is wrong with it raises
    what memo_query.main raises.  One device.  Returns Tracks: (counts uint64 [N, B], edges int64 [B + 1] from the window's start),
    which is .qs; an empty window gives (uint64 [N, 0], [0])."""
    from . import memo_query
    record, qs, qe = parse_region(region)
    edges = region_edges(qe - qs, n_bins) if qe > qs or n_bins < 1 else np.zeros(1, np.int64)
    index = memo_query.region_index(index_path, record, qs, qe + k, device=device, k=k, num_docs=n_docs, membership=True)
    with index:
        if qe == qs:                                       # (nothing to sweep, as in region_matrix)
            return Tracks(np.zeros((n_docs, 0), np.uint64), edges, qs)
        with DevBuffer.of(_table(n_docs, n_bins, None), device) as d_counts:
            for d_bits, s, e in membership_slices(index, qs, qe, k, n_docs, slice_positions, device):
                _accumulate(d_bits, e - s, n_docs, s - qs, edges, d_counts.d, device)
            return Tracks(d_counts.to_host((n_docs, n_bins), np.uint64), edges, qs)


def fractions(counts, edges):
    """count / bin width, float64 [N, B]: the share of a bin's k-mers each genome holds (an empty bin raises ZeroDivisionError, as
    `memo view`'s table does)"""
    width = np.diff(np.asarray(edges, np.int64))
    if np.any(width == 0):
        raise ZeroDivisionError("division by zero")
    return np.asarray(counts).astype(np.float64) / width[None, :].astype(np.float64)


def format_tracks(table, qs, edges, labels=None):
    """tab-separated text: a header line `genome` and one field START-END per bin (absolute pivot coordinates, half open), then one
    line per genome: its annot number (0 is the pivot) or its label, and its values -- integers as they are, floats by repr (the
    convention of `memo view`'s .tsv)"""
    table = np.asarray(table)
    edges = [int(e) + int(qs) for e in edges]
    if table.ndim != 2 or table.shape[1] != len(edges) - 1:
        raise ValueError(f"a table of {table.shape} for {len(edges) - 1} bins")
    cell = (lambda v: repr(float(v))) if table.dtype.kind == "f" else (lambda v: str(int(v)))
    if labels is not None:
        labels = list(labels)
        if len(labels) != len(table):
            raise ValueError(f"{len(labels)} labels for {len(table)} genomes")
    lines = ["\t".join(["genome"] + [f"{a}-{b}" for a, b in zip(edges[:-1], edges[1:])])]
    for g, row in enumerate(table.tolist()):
        lines.append("\t".join([labels[g] if labels is not None else str(g)] + [cell(v) for v in row]))
    return "".join(line + "\n" for line in lines)
