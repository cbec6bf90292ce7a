"""`memo mems`: the maximal shared matches of a window, as intervals, compacted on the GPU.

No counterpart in the reference.  The lengths v[p] that `memo maxk` and `memo lengths` leave in HBM hold the maximal matches in closed
form: position p starts one exactly when the match at p - 1 does not contain it.  With a cap and a smallest length min_len, position
p of the window [qs, qe) is REPORTED, as the match [p, p + v[p]), when

    v[p] >= min_len   and   ( p == 0   or   v[p - 1] < v[p]   or   v[p - 1] == v[p] < cap )

(a run at the cap is one match of "at least cap", reported at its first position).  v[qs - 1] is the true length of the position
before the window: the pass runs on [qs - 1, qe) and its first cell is only a neighbour, so a window reports exactly the matches that
start in it, and the lists of windows laid end to end are the list of the whole (rows with end >= start).  A match is not clipped at
qe.  Between two starts the lengths fall by one per position: the list is a lossless run-coding of `memo maxk`'s output wherever no
value is the cap.  Four sources of v:

    conservation index, threshold=T       memo_maxk_*_dev mode 0              the stretches at least T genomes share
    membership, genome=G                  memo_maxk_*_dev mode 1              the stretches in which genome G follows the pivot
    membership, threshold=T               memo_lengths_select_dev             the same stretches as the conservation index gives
    membership, all_genomes               the planes 1 .. N - 1 of memo_lengths_*_dev, one list per genome (0 is the pivot: no rows)

union=True gives the covered bases instead: the union of [p, p + min_len) over the positions of the window with v[p] >= min_len, as
maximal intervals.  The cap plays no part in them, so the pass runs at cap = min_len; the device compacts the boundaries of the band
v >= min_len (memo_regions' band key) and the widening by min_len - 1 and the joining of neighbours are one vectorised comparison on
the host.

memo_amd/csrc/memo_mems.hip compacts the starts where the lengths lie: count per tile, scan, scatter; only the list leaves the
device.  The flags are memo_amd/mems_cli.py.
"""
import collections
import ctypes as C

import numpy as np

from ._device import DevBuffer, RowBuffer, emit_text
from ._lib import check, lib
from .lengths import docs, finished_slices, pitch_of, region_feed, region_window
from .maxk import CAP_MAX, Cells

L_MAX = 2 ** 31 - 1

Mems = collections.namedtuple("Mems", "record starts ends genome")
Mems.__doc__ = """region_mems' result: int64 starts and ends (0-based, half open, absolute), ascending; genome is None, or with
all_genomes the int32 genome of every entry (the entries are grouped by genome, ascending within one)"""


def tile():
    """cells per tile of the passes: the lengths a test wants to straddle"""
    return int(lib().memo_mems_tile())


def of_cells(d_cells, L, pitch, planes=1, *, cap=CAP_MAX, min_len=1, band=False, halo=0, device=0, stream=None):
    """memo_mems_dev on finished cells that lie on the device (uint32 [planes][pitch], L cells per plane read).  Returns
    (starts, lengths, counts): uint32 cell offsets and the cells' values of the reported cells, plane-major and ascending within a
    plane, and uint64 [planes] entries per plane.  band: the boundaries of v >= min_len instead (lengths is None)."""
    d_starts, d_lengths = C.c_void_p(), C.c_void_p()
    counts = np.zeros(max(int(planes), 0), np.uint64)
    check(lib().memo_mems_dev(C.c_void_p(int(getattr(d_cells, "value", d_cells) or 0)), int(L), int(pitch), int(planes), int(cap), int(min_len),
                              2 if band else 1, int(halo), C.byref(d_starts), None if band else C.byref(d_lengths), counts.ctypes.data,
                              device, None if stream is None else C.c_void_p(int(stream))))
    with DevBuffer.adopt(d_starts, device) as starts, DevBuffer.adopt(d_lengths, device) as lengths:
        entries = int(counts.sum())
        return starts.to_host(entries, np.uint32), (None if band else lengths.to_host(entries, np.uint32)), counts


def merge(begin, end):
    """Intervals sorted by begin -> the maximal intervals of their union: intervals that overlap or abut are one.  int64 (begins, ends)."""
    begin, end = np.asarray(begin, np.int64), np.asarray(end, np.int64)
    if not len(begin):
        return begin.copy(), end.copy()
    reach = np.maximum.accumulate(end)
    first = np.flatnonzero(np.concatenate([[True], begin[1:] > reach[:-1]]))
    return begin[first], np.maximum.reduceat(end, first)


def band_intervals(boundaries, L, widen=0):
    """(begins, ends) cell offsets of one plane's band from its boundaries (an odd count: the last interval ends at L), each widened by
    `widen` cells on the right and merged"""
    b = np.asarray(boundaries, np.int64)
    if len(b) & 1:
        b = np.append(b, np.int64(L))
    return merge(b[0::2], b[1::2] + int(widen))


def _split(values, counts):
    return np.split(values, np.cumsum(counts.astype(np.int64))[:-1]) if len(counts) else []


def _plane_lists(d_cells, L, pitch, planes, origin, halo, cap, min_len, union, device):
    """[(starts, ends)] absolute, per plane, of cells whose cell 0 is position `origin`"""
    if union:
        bounds, _, counts = of_cells(d_cells, L, pitch, planes, cap=cap, min_len=min_len, band=True, device=device)
        out = []
        for part in _split(bounds, counts):
            b, e = band_intervals(part, L, min_len - 1)
            out.append((b + origin, e + origin))
        return out
    starts, lengths, counts = of_cells(d_cells, L, pitch, planes, cap=cap, min_len=min_len, halo=halo, device=device)
    at = starts.astype(np.int64) + origin
    return [(s, s + v) for s, v in zip(_split(at, counts), _split(lengths.astype(np.int64), counts))]


def _check(n_docs, threshold, genome, membership, all_genomes, min_len, cap, union):
    """the mode and its numbers, or a ValueError before any device call"""
    n_docs = docs(n_docs)
    if not membership and (genome is not None or all_genomes):
        raise ValueError("genome and all_genomes are questions to a membership index")
    if genome is not None and all_genomes:
        raise ValueError("either one genome or all of them")
    if threshold is not None and (genome is not None or all_genomes):
        raise ValueError("a threshold cannot be combined with genome or all_genomes")
    if genome is None and not all_genomes:
        threshold = n_docs if threshold is None else int(threshold)
        if not 1 <= threshold <= n_docs:
            raise ValueError(f"threshold must be in [1, {n_docs}]")
    if genome is not None and not 0 <= int(genome) < n_docs:
        raise ValueError(f"genome must be in [0, {n_docs})")
    if union:
        if cap is not None:
            raise ValueError("the covered bases do not depend on a cap: cap cannot be combined with union")
        if not 1 <= int(min_len) <= CAP_MAX:
            raise ValueError(f"min_len must be in [1, {CAP_MAX}]")
        cap = int(min_len)
    cap = CAP_MAX if cap is None else int(cap)
    if not 1 <= cap <= CAP_MAX:
        raise ValueError(f"cap must be in [1, {CAP_MAX}]")
    if not 1 <= int(min_len) <= cap:
        raise ValueError(f"min_len must be in [1, {cap}]")
    return n_docs, threshold, None if genome is None else int(genome), int(min_len), cap


def region_mems(index_path, region, n_docs, *, threshold=None, genome=None, membership=False, all_genomes=False, min_len=1, cap=None,
                union=False, device=0, slice_positions=None):
    """The maximal matches that start in a window of a Parquet index (union: the covered bases), as Mems.  `region` is CHR:START-END as
    `memo query -r` takes it, and what is wrong with it raises what memo_query.main raises.  threshold (default n_docs: shared by all)
    on a conservation index, or with membership the threshold-th largest of the genomes' lengths; genome: one genome of a membership
    index; all_genomes: every genome 1 .. n_docs - 1 of it, one list each.  cap=None: 2^31 - 1.  slice_positions: the planes of
    a membership index are taken in slices of that many positions (the result does not depend on it).  One device."""
    n_docs, threshold, genome, min_len, cap = _check(n_docs, threshold, genome, membership, all_genomes, min_len, cap, union)
    record, qs, L, cap = region_window(region, cap)
    if qs < 0:
        raise ValueError("the window starts before position 0 of the record")
    if L > L_MAX:
        raise ValueError(f"a window of at most {L_MAX} positions")
    empty = np.zeros(0, np.int64)
    if not L:
        return Mems(record, empty, empty, np.zeros(0, np.int32) if all_genomes else None)
    h = 0 if union or qs == 0 else 1            # the cell of position qs - 1: a neighbour only
    lo, Lh = qs - h, L + h
    if all_genomes:
        per_genome = [[] for _ in range(n_docs - 1)]
        feed, buf = region_feed(index_path, record, device)
        with buf:
            for a, b, d_cells, pitch in finished_slices(feed, qs, L, n_docs, cap, device, slice_positions, halo=0 if union else 1):
                hs = 0 if union or a == 0 else 1
                first = C.c_void_p((d_cells.value or 0) + 4 * pitch)         # plane 1: the pivot's plane is left out
                lists = _plane_lists(first, b - a + hs, pitch, n_docs - 1, a - hs, hs, cap, min_len, union, device)
                for mine, got in zip(per_genome, lists):
                    mine.append(got)
        starts, ends, who = [empty], [empty], [np.zeros(0, np.int32)]
        for g, parts in enumerate(per_genome, 1):                            # the slices came from the right
            s = np.concatenate([p[0] for p in parts[::-1]])
            e = np.concatenate([p[1] for p in parts[::-1]])
            if union:
                s, e = merge(s, e)                                           # a run that a slice bound cut is one interval
            starts.append(s), ends.append(e), who.append(np.full(len(s), g, np.int32))
        return Mems(record, np.concatenate(starts), np.concatenate(ends), np.concatenate(who))
    if membership and genome is None:
        # the planes in slices, their threshold-th largest into one whole-window buffer that stays on the device
        feed, buf = region_feed(index_path, record, device)
        pitch = pitch_of(Lh)
        with buf, DevBuffer(device, 4 * pitch) as sel:
            for a, b, d_cells, p in finished_slices(feed, lo, Lh, n_docs, cap, device, slice_positions):
                check(lib().memo_lengths_select_dev(d_cells, b - a, p, n_docs, cap, threshold, sel.at(4 * (a - lo)), device, None))
            (s, e), = _plane_lists(sel.d, Lh, pitch, 1, lo, h, cap, min_len, union, device)
        return Mems(record, s, e, None)
    from . import memo_query
    mode, arg = (0, threshold) if genome is None else (1, genome)
    with Cells(lo, Lh, cap, mode, arg, device) as cells, RowBuffer(device) as buf:
        _, chunks = memo_query.region_chunks(index_path, record, lo, min(qs + L + cap, 2 ** 62))
        for cols in chunks:
            cells.add(*buf.upload(*cols))
        check(lib().memo_maxk_finish_dev(cells.d, Lh, cap, device, None))
        (s, e), = _plane_lists(cells.d, Lh, pitch_of(Lh), 1, lo, h, cap, min_len, union, device)
    return Mems(record, s, e, None)


def emit(result):
    """the text of a region_mems result: REC start end, and the genome as a fourth column where there is one; a uint8 array (write it
    with fh.write(memoryview(buf))); empty for no entries"""
    s, e = np.ascontiguousarray(result.starts, np.int64), np.ascontiguousarray(result.ends, np.int64)
    g = None if result.genome is None else np.ascontiguousarray(result.genome, np.int32)
    if len(e) != len(s) or (g is not None and len(g) != len(s)):
        raise ValueError("starts, ends and genome differ in length")
    args = (result.record.encode(), s.ctypes.data, e.ctypes.data, None if g is None else g.ctypes.data, len(s))
    return emit_text(lambda buf, cap: lib().memo_emit_intervals(*args, buf, cap))
