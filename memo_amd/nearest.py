"""`memo nearest`: which genome of a membership index matches the pivot longest, per bin and as intervals -- haplotype painting.

No counterpart in the reference.  `memo lengths` leaves every genome's match length with the pivot in HBM, plane by plane;
`memo breaks` and `memo pairs` reduce along the planes.  This reduces ACROSS them: with v[g][p] = min(length, cap), a candidate set C
of genomes (never genome 0, the pivot; default 1 .. N - 1) and a threshold min_len, per position p of the window

    best[p]    = max{ v[g][p] : g in C }              ok[p] = best[p] >= min_len
    att[g][p]  = g in C and ok[p] and v[g][p] == best[p]              every tied genome attains
    sole[g][p] = att[g][p] and no other genome attains at p
    winner[p]  = the smallest g with att[g][p], 0 where not ok[p]

and per bin b of `memo view`'s bins (tracks.region_edges, so the columns line up with `memo tracks` and `memo breaks`)

    wins[0][g][b] = #{ p in b : att[g][p] }    g >= 1        wins[0][0][b] = #{ p in b : not ok[p] }      ("none")
    wins[1][g][b] = #{ p in b : sole[g][p] }   g >= 1        wins[1][0][b] = the same "none" count
    sums[b]       = sum of best[p]                           (min_len plays no part)

Rows of genomes outside C are zero.  With min_len == cap == K row g of wins[0] is row g of `memo tracks -k K`; with one bin per
position sums is `memo lengths -t 2` where the pivot has no rows and C is everything; wins[1] <= wins[0].  memo_nearest_dev
(memo_amd/csrc/memo_nearest.hip) reads every candidate plane once, where it lies, slice by slice; 2 x N x B + B integers leave the
device, or the winner vector's runs (memo_runs_conservation_dev's value mode run-codes the uint16 [L] vector on the device).  The
flags are memo_amd/nearest_cli.py.  One device; not built: several GPUs, a BED of features, a plot, tie-breaking other than the lowest
annot, a conservation index.  (The greedy minimal mosaic, the relative Lempel-Ziv parse, is `memo mosaic`: memo_amd/mosaic.py.)
"""
import ctypes as C

import numpy as np

from ._device import DevBuffer
from ._lib import check, lib
from ._window import parse_region
from .breaks import _check_window, _edges
from .lengths import finished_slices, pitch_of, region_feed
from .maxk import CAP_MAX
from .merge import parse_selection
from .regions import runs
from .tracks import region_edges

N_MIN, N_MAX = 2, 2048
MAX_RUNS = 1024                      # workgroups of a call at most: each takes a run of consecutive tiles
WORDS = N_MAX // 32


def tile(n_docs):
    """positions per tile of the kernel at n_docs planes: the lengths a test wants to straddle"""
    return int(lib().memo_nearest_tile(int(n_docs)))


def tiles_per_run(L, n_docs):
    """the launcher's run rule: how many consecutive tiles one workgroup takes of a slice of L positions"""
    ntiles = -(-int(L) // tile(n_docs))
    return -(-ntiles // min(MAX_RUNS, max(ntiles, 1)))


def candidate_words(candidates, n_docs):
    """uint32 [64], bit g = genome g is a candidate, from a selection in `memo merge -s` syntax, a list of annots, or None (all);
    an array of 64 uint32 words passes as it is"""
    if isinstance(candidates, np.ndarray) and candidates.dtype == np.uint32 and candidates.shape == (WORDS,):
        return np.ascontiguousarray(candidates)
    words = np.zeros(WORDS, np.uint32)
    for g in parse_selection(candidates, n_docs):
        words[g >> 5] |= np.uint32(1 << (g & 31))
    return words


def _check(n_docs, candidates, min_len, cap):
    """(n_docs, candidate words or None, min_len, cap), or a ValueError before any device call"""
    n_docs = int(n_docs)
    if not N_MIN <= n_docs <= N_MAX:
        raise ValueError(f"n_docs must be in [{N_MIN}, {N_MAX}]: the pivot and at least one genome to compare it with")
    cap = CAP_MAX if cap is None else int(cap)
    if not 1 <= cap <= CAP_MAX:
        raise ValueError(f"cap must be in [1, {CAP_MAX}]")
    if not 1 <= int(min_len) <= cap:
        raise ValueError(f"min_len must be in [1, {cap}]")
    return n_docs, (None if candidates is None else candidate_words(candidates, n_docs)), int(min_len), cap


def _call(d_cells, L, pitch, planes, cap, min_len, words, first, edges, d_wins, d_sums, d_winner, device, stream=None):
    check(lib().memo_nearest_dev(C.c_void_p(int(getattr(d_cells, "value", d_cells) or 0)), int(L), int(pitch), int(planes), int(cap), int(min_len),
                                 None if words is None else words.ctypes.data, int(first),
                                 None if edges is None else edges.ctypes.data, 0 if edges is None else len(edges) - 1,
                                 d_wins, d_sums, d_winner, device, None if stream is None else C.c_void_p(int(stream))))


def plane_nearest(cells, edges, *, cap, min_len=1, candidates=None, first=0, wins=None, sums=None, winner=False, device=0, stream=None):
    """The kernel alone: `cells` is a host uint32 array [planes, L] (padded to the pitch and uploaded) or a (device pointer, L, pitch,
    planes) tuple of finished lengths; cell i is position first + i, and `edges` are bins + 1 non-decreasing positions in the same
    coordinates that hold the slice (None: no tables).  `wins` and `sums`: None starts from zeros, an array is the starting value
    (the slices of a window accumulate), False leaves the table out; `winner`: the vector too.  `candidates`: a selection as
    `memo merge -s` writes it, a list of annots, 64 uint32 words, or None for all.  Returns (wins uint64 [2, planes, bins], sums
    uint64 [bins], winner uint16 [L]), None for what was not asked."""
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
    if edges is None:
        wins = sums = False
        bins = 0
    else:
        edges = _edges(edges)
        bins = len(edges) - 1
    start = []
    for table, shape, name in ((wins, (2, max(planes, 0), bins), "wins"), (sums, (bins,), "sums")):
        if table is False:
            start.append(None)
            continue
        host = np.zeros(shape, np.uint64) if table is None else np.ascontiguousarray(table, np.uint64)
        if host.shape != shape:
            raise ValueError(f"{name} must be {list(shape)}")
        start.append(host)
    none = np.zeros(0, np.uint64)
    with DevBuffer(device, 0) if padded is None else DevBuffer.of(padded, device) as owner, \
            DevBuffer.of(none if start[0] is None else start[0], device) as d_wins, \
            DevBuffer.of(none if start[1] is None else start[1], device) as d_sums, DevBuffer(device, max(2 * L, 8) if winner else 0) as d_winner:
        _call(d_cells if padded is None else owner.d, L, pitch, planes, cap, min_len, words, first, edges,
              None if start[0] is None else d_wins.d, None if start[1] is None else d_sums.d, d_winner.d if winner else None, device, stream)
        return (None if start[0] is None else d_wins.to_host(start[0].shape, np.uint64),
                None if start[1] is None else d_sums.to_host(start[1].shape, np.uint64),
                d_winner.to_host(L, np.uint16) if winner else None)


def _slices(index_path, record, qs, L, n_docs, cap, device, slice_positions):
    """(a, b, d_cells, pitch) of every slice of the window, its planes finished on the device, no halo"""
    feed, buf = region_feed(index_path, record, device)
    with buf:
        yield from finished_slices(feed, qs, L, n_docs, cap, device, slice_positions, halo=0)


def region_nearest(index_path, region, n_docs, n_bins, *, candidates=None, min_len=1, cap=None, device=0, slice_positions=None):
    """The wins, the sole wins and the sums of best of a window of a Parquet MEMBERSHIP index, in n_bins bins (tracks.region_edges:
    `memo view`'s rule).  `region` is CHR:START-END as `memo query -r` takes it, and what is wrong with it raises what
    memo_query.main raises.  candidates: as `memo merge -s` takes them, or a list of annots; None: all.  cap=None: 2^31 - 1.
    slice_positions: the planes are taken in slices of that many positions (the tables do not depend on it).  One device.  Returns
    (wins uint64 [2, N, B], sums uint64 [B], edges int64 [B + 1] from the window's start, qs); an empty window gives
    ([2, N, 0], [0], [0], qs)."""
    n_docs, words, min_len, cap = _check(n_docs, candidates, min_len, cap)
    record, qs, qe = parse_region(region)
    _check_window(qs, qe - qs)
    if qe == qs and n_bins >= 1:
        return np.zeros((2, n_docs, 0), np.uint64), np.zeros(0, np.uint64), np.zeros(1, np.int64), qs
    edges = region_edges(qe - qs, int(n_bins))
    absolute = np.ascontiguousarray(edges + qs, np.int64)
    with DevBuffer.of(np.zeros((2, n_docs, n_bins), np.uint64), device) as d_wins, DevBuffer.of(np.zeros(n_bins, np.uint64), device) as d_sums:
        for a, b, d_cells, pitch in _slices(index_path, record, qs, qe - qs, n_docs, cap, device, slice_positions):
            _call(d_cells, b - a, pitch, n_docs, cap, min_len, words, a, absolute, d_wins.d, d_sums.d, None, device)
        return d_wins.to_host((2, n_docs, n_bins), np.uint64), d_sums.to_host(n_bins, np.uint64), edges, qs


def region_winners(index_path, region, n_docs, *, candidates=None, min_len=1, cap=None, device=0, slice_positions=None):
    """The winner of every position of a window of a Parquet MEMBERSHIP index as maximal runs: the vector uint16 [L] stays on the
    device, every slice writes its part, and after the last slice it is run-coded there (memo_runs_conservation_dev, value mode);
    only the runs leave the device.  Returns (starts int64 [R] from the window's start, winners uint16 [R], 0 = none, qs, qe); run r
    is [qs + starts[r], qs + starts[r + 1]) and the last one ends at qe.  An empty window gives no runs."""
    n_docs, words, min_len, cap = _check(n_docs, candidates, min_len, cap)
    record, qs, qe = parse_region(region)
    L = qe - qs
    _check_window(qs, L)
    if not L:
        return np.zeros(0, np.int64), np.zeros(0, np.uint16), qs, qe
    with DevBuffer(device, 2 * L) as d_winner:
        for a, b, d_cells, pitch in _slices(index_path, record, qs, L, n_docs, cap, device, slice_positions):
            _call(d_cells, b - a, pitch, n_docs, cap, min_len, words, a, None, None, None, d_winner.at(2 * (a - qs)), device)
        starts, winners = runs((d_winner.d.value, L), "value", device=device)
    return starts, winners, qs, qe


def format_nearest(wins, sums, qs, edges, labels=None):
    """tab-separated text: tracks.format_tracks' header of bins, a row `none`, the rows 1 .. N - 1 (their annot numbers, or their
    labels: `labels` names all N genomes, the pivot first), and a last row `best`.  `wins` is one half of the table ([N, B]: row 0
    the none count), integers or floats; `sums` [B] likewise."""
    from .tracks import format_tracks
    wins, sums = np.asarray(wins), np.asarray(sums)
    if wins.ndim != 2 or sums.shape != wins.shape[1:]:
        raise ValueError(f"a table of {wins.shape} and sums of {sums.shape}")
    n = len(wins)
    if labels is not None and len(labels) != n:
        raise ValueError(f"{len(labels)} labels for {n} genomes")
    names = ["none"] + [str(g) if labels is None else labels[g] for g in range(1, n)] + ["best"]
    kind = np.float64 if wins.dtype.kind == "f" or sums.dtype.kind == "f" else np.uint64
    return format_tracks(np.concatenate([wins.astype(kind), sums.astype(kind)[None, :]]), qs, edges, names)


def format_intervals(record, qs, qe, starts, winners, labels=None):
    """one `CHR START END GENOME` line (tab-separated) per run: the winner's annot number or its label, `.` for none"""
    starts = [int(s) + int(qs) for s in starts]
    ends = starts[1:] + [int(qe)]
    name = (lambda g: str(g)) if labels is None else (lambda g: labels[g])
    return "".join(f"{record}\t{s}\t{e}\t{name(int(g)) if g else '.'}\n" for s, e, g in zip(starts, ends, winners))
