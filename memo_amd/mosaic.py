"""`memo mosaic`: the pivot as the fewest pieces, each copied whole from one genome of a membership index -- the greedy relative
Lempel-Ziv parse by longest match.

No counterpart in the reference.  `memo nearest -i` paints every position with its own winner, and the winner flips wherever two
genomes' lengths cross; the question "which haplotypes is my assembly made of, and where are the breakpoints" wants the opposite:
start at the window's left end, take the genome that matches longest from there, jump to the end of that match, repeat.  With
best[p], ok[p] and winner[p] exactly as `memo nearest` defines them (v[g][p] = min(length, cap), candidates C, min_len; ties to the
lowest annot, the pivot never a candidate), for a window [qs, qe)

    step[p] = best[p] where ok[p], else 1         a position no candidate reaches at min_len is a literal of one base
    p_0 = qs;   p_{i+1} = p_i + step[p_i]   while p_i < qe                                    the REACHED positions

and phrase i is [p_i, min(p_{i+1}, qe)) copied from winner[p_i] (0: none).  A line is one phrase; consecutive none-phrases are one
line; adjacent phrases of one genome stay two lines, because they are two copies.  The lines partition the window.

The lengths an index yields fall by at most one a position, so p + best[p] never decreases, and with min_len = 1 the greedy parse
has the fewest phrases of any cover of the window by pieces [p, p + l) with l <= max(best[p], 1); with min_len > 1
it is still defined but not promised minimal.  It depends on where the window starts and not on the slicing.

memo_mosaic_fold_dev (memo_amd/csrc/memo_mosaic.hip) reads every candidate plane once, where it lies, slice by slice, and leaves
step and winner of the whole window on the device (6 bytes a position); memo_mosaic_parse_dev follows the chain there -- pointer
jumping inside LDS tiles, one short serial walk over the tiles' entries, a parallel mark, a compaction -- and only the lines leave the
device.  The flags are memo_amd/mosaic_cli.py.  One device; not built: several GPUs, a BED of features, a plot, the genome-side
coordinates of a piece (the index does not hold them), a parse that prefers to stay on the current genome, a conservation index.
"""
import ctypes as C

import numpy as np

from ._device import DevBuffer
from ._lib import check, lib
from ._window import parse_region
from .breaks import _check_window
from .lengths import pitch_of
from .nearest import _check, _slices, candidate_words


def tile():
    """positions per tile of the parse: the lengths a test wants to straddle"""
    return int(lib().memo_mosaic_tile())


def _fold(d_cells, L, pitch, planes, cap, min_len, words, d_step, d_winner, device, stream=None):
    check(lib().memo_mosaic_fold_dev(C.c_void_p(int(getattr(d_cells, "value", d_cells) or 0)), int(L), int(pitch), int(planes), int(cap), int(min_len),
                                     None if words is None else words.ctypes.data, d_step, d_winner, device,
                                     None if stream is None else C.c_void_p(int(stream))))


def _parse(d_step, d_winner, L, device, stream=None):
    """(starts int64 [R], genomes uint16 [R]) of whole-window vectors on the device"""
    d_starts, d_genomes, n = C.c_void_p(), C.c_void_p(), C.c_uint64(0)
    check(lib().memo_mosaic_parse_dev(d_step, d_winner, int(L), C.byref(d_starts), C.byref(d_genomes), C.byref(n), device,
                                      None if stream is None else C.c_void_p(int(stream))))
    with DevBuffer.adopt(d_starts, device) as b_starts, DevBuffer.adopt(d_genomes, device) as b_genomes:
        return b_starts.to_host(n.value, np.int64), b_genomes.to_host(n.value, np.uint16)


def parse(step, winner, device=0, stream=None):
    """The parse alone on host vectors step uint32 [L] and winner uint16 [L]: (starts int64 [R], genomes uint16 [R]).  The lines of
    no genome merge by the device's local rule, which is the phrases' rule where a position of no genome has a step of 1 (or 0),
    as the fold leaves it."""
    step, winner = np.ascontiguousarray(step, np.uint32), np.ascontiguousarray(winner, np.uint16)
    if step.ndim != 1 or winner.shape != step.shape:
        raise ValueError("step and winner must be vectors of one length")
    with DevBuffer.of(step, device) as d_step, DevBuffer.of(winner, device) as d_winner:
        return _parse(d_step.d, d_winner.d, len(step), device, stream)


def plane_mosaic(cells, *, cap, min_len=1, candidates=None, vectors=False, device=0, stream=None):
    """Fold and parse of one slice that is the whole window: `cells` is a host uint32 array [planes, L] (padded to the pitch and
    uploaded) or a (device pointer, L, pitch, planes) tuple of finished lengths.  `candidates`: a selection as `memo merge -s` writes
    it, a list of annots, 64 uint32 words, or None for all.  Returns (starts int64 [R], genomes uint16 [R]); with vectors=True also
    (step uint32 [L], winner uint16 [L])."""
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
    words = None if candidates is None else candidate_words(candidates, planes)
    with DevBuffer(device, 0) if padded is None else DevBuffer.of(padded, device) as owner, DevBuffer(device, max(4 * L, 8)) as d_step, \
            DevBuffer(device, max(2 * L, 8)) as d_winner:
        _fold(d_cells if padded is None else owner.d, L, pitch, planes, cap, min_len, words, d_step.d, d_winner.d, device, stream)
        lines = _parse(d_step.d, d_winner.d, L, device, stream)
        return (*lines, d_step.to_host(L, np.uint32), d_winner.to_host(L, np.uint16)) if vectors else lines


def region_mosaic(index_path, region, n_docs, *, candidates=None, min_len=1, cap=None, device=0, slice_positions=None):
    """The greedy parse of a window of a Parquet MEMBERSHIP index: step and winner of the whole window stay on the device (6 bytes a
    position), every slice writes its part, from the right, and one parse follows the last slice; only the lines leave the device.
    `region` is CHR:START-END as `memo query -r` takes it, and what is wrong with it raises what memo_query.main raises; candidates,
    min_len, cap and slice_positions as nearest.region_winners takes them (the lines do not depend on the slicing).  One device.
    Returns (starts int64 [R] from the window's start, genomes uint16 [R], 0 = none, qs, qe), the shape of nearest.region_winners:
    line r is [qs + starts[r], qs + starts[r + 1]) and the last one ends at qe.  An empty window gives no lines."""
    n_docs, words, min_len, cap = _check(n_docs, candidates, min_len, cap)
    record, qs, qe = parse_region(region)
    L = qe - qs
    _check_window(qs, L)
    if not L:
        return np.zeros(0, np.int64), np.zeros(0, np.uint16), qs, qe
    with DevBuffer(device, 4 * L) as d_step, DevBuffer(device, 2 * L) as d_winner:
        for a, b, d_cells, pitch in _slices(index_path, record, qs, L, n_docs, cap, device, slice_positions):
            _fold(d_cells, b - a, pitch, n_docs, cap, min_len, words, d_step.at(4 * (a - qs)), d_winner.at(2 * (a - qs)), device)
        starts, genomes = _parse(d_step.d, d_winner.d, L, device)
    return starts, genomes, qs, qe


def bin_phrases(starts, genomes, L, edges, n_docs):
    """The lines of a window of L positions cut at the bin edges (bins + 1 non-decreasing positions from the window's start, the first
    0 and the last L), on the host: (bases uint64 [N, B], lines uint64 [B]).  Row 0 of bases is none, row g the bases of bin b that
    lie inside lines of genome g; lines counts the lines that START in the bin.  Every column of bases sums to its bin's width."""
    starts, genomes = np.asarray(starts, np.int64), np.asarray(genomes, np.int64)
    edges = np.asarray(edges, np.int64)
    n_docs, bins = int(n_docs), len(edges) - 1
    if starts.shape != genomes.shape or starts.ndim != 1:
        raise ValueError("starts and genomes must be vectors of one length")
    if bins < 0 or (bins and (edges[0] != 0 or edges[-1] != L)) or np.any(np.diff(edges) < 0):
        raise ValueError("the edges must run from 0 to L and not decrease")
    if len(genomes) and (genomes.min() < 0 or genomes.max() >= n_docs):
        raise ValueError(f"a genome outside [0, {n_docs})")
    bases, lines = np.zeros((n_docs, bins), np.uint64), np.zeros(bins, np.uint64)
    if not len(starts) or not bins:
        return bases, lines
    ends = np.append(starts[1:], np.int64(L))
    first = np.searchsorted(edges, starts, "right") - 1                    # the bin a line starts in (the last of equal edges)
    first = np.minimum(first, bins - 1)
    last = np.maximum(np.searchsorted(edges, ends, "left") - 1, first)     # the bin its last base lies in
    np.add.at(lines, first, np.uint64(1))
    # a line's pieces: one per bin it touches
    pieces = last - first + 1
    line = np.repeat(np.arange(len(starts)), pieces)
    b = np.arange(int(pieces.sum())) - np.repeat(np.cumsum(pieces) - pieces, pieces) + first[line]
    width = np.minimum(ends[line], edges[b + 1]) - np.maximum(starts[line], edges[b])
    np.add.at(bases, (genomes[line], b), np.maximum(width, 0).astype(np.uint64))
    return bases, lines


def format_mosaic(bases, lines, qs, edges, labels=None):
    """tab-separated text: tracks.format_tracks' header of bins, a row `none`, the rows 1 .. N - 1 (their annot numbers, or their
    labels: `labels` names all N genomes, the pivot first), and a last row `phrases`.  `bases` is [N, B] (row 0 the none bases),
    integers or floats; `lines` [B] likewise."""
    from .tracks import format_tracks
    bases, lines = np.asarray(bases), np.asarray(lines)
    if bases.ndim != 2 or lines.shape != bases.shape[1:]:
        raise ValueError(f"a table of {bases.shape} and phrases of {lines.shape}")
    n = len(bases)
    if labels is not None and len(labels) != n:
        raise ValueError(f"{len(labels)} labels for {n} genomes")
    names = ["none"] + [str(g) if labels is None else labels[g] for g in range(1, n)] + ["phrases"]
    kind = np.float64 if bases.dtype.kind == "f" or lines.dtype.kind == "f" else np.uint64
    return format_tracks(np.concatenate([bases.astype(kind), lines.astype(kind)[None, :]]), qs, edges, names)
