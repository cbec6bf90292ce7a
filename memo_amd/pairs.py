"""`memo pairs`: for every pair of genomes, the match length they share with the pivot, summed over a window -- `memo matrix` at
every k at once.

No counterpart in the reference.  `memo matrix` counts the positions two genomes share at ONE k, and presence at one k saturates:
at k = 31 a genome that is 99 % identical to the pivot and one that is 99.9 % look nearly alike, at k = 101 both look empty.  The
lengths len[g][p] that `memo lengths` leaves in HBM do not saturate.  min(len[g][p], len[h][p]) is the largest k at which g and h both
still hold the pivot's k-mer at p, so with 1 <= KMIN <= KMAX and the lengths capped at KMAX

    w[g][p] = max(0, min(len[g][p], KMAX) - (KMIN - 1))        the number of k in [KMIN, KMAX] at which genome g holds the k-mer at p
    S[g][h] = sum over the window's p of min(w[g][p], w[h][p])      uint64 [N, N], symmetric

is the sum of `memo matrix -k k`'s matrices over k = KMIN .. KMAX (for index rows with end >= start), S(k, k) is `memo matrix -k k`'s
matrix itself, and with KMIN = 1 the diagonal S[g][g] is genome g's row of `memo breaks -m -s -B 1 -K KMAX`.  Genome 0 is the pivot:
nothing bounds it, its plane is the cap everywhere, so S[0][h] = S[h][h].  memo_pairs_dev (memo_amd/csrc/memo_pairs.hip) reads the
finished planes once per slice, where they lie, and N x N integers are downloaded.  The flags are memo_amd/pairs_cli.py.
"""
import ctypes as C

import numpy as np

from ._device import DevBuffer
from ._lib import check, lib
from ._window import parse_region
from .lengths import N_MAX, finished_slices, pitch_of, region_feed
from .maxk import CAP_MAX

L_MAX = 2 ** 31 - 1


def tile():
    """positions per tile of the kernel: the lengths a test wants to straddle"""
    return int(lib().memo_pairs_tile())


def chunk():
    """the most genomes one launch stages: above it the genomes come in chunks, one launch per pair of chunks"""
    return int(lib().memo_pairs_chunk())


def narrow_span():
    """the largest KMAX - KMIN + 1 the kernel adds up in 32 bits per tile; above it in 64 bits (the sums are exact either way)"""
    return int(lib().memo_pairs_narrow_span())


def _accumulate(d_cells, L, pitch, planes, kmin, kmax, d_sums, device, stream=None):
    check(lib().memo_pairs_dev(C.c_void_p(int(getattr(d_cells, "value", d_cells) or 0)), int(L), int(pitch), int(planes), int(kmin), int(kmax),
                               d_sums, device, None if stream is None else C.c_void_p(int(stream))))


def _span(kmin, kmax):
    """(kmin, kmax), or a ValueError before any device call"""
    kmax = CAP_MAX if kmax is None else int(kmax)
    if not 1 <= kmax <= CAP_MAX:
        raise ValueError(f"kmax must be in [1, {CAP_MAX}]")
    if not 1 <= int(kmin) <= kmax:
        raise ValueError(f"kmin must be in [1, {kmax}]")
    return int(kmin), kmax


def plane_sums(cells, *, kmin=1, kmax, sums=None, device=0, stream=None):
    """The kernel alone: `cells` is a host uint32 array [planes, L] (padded to the pitch and uploaded) or a (device pointer, L, pitch,
    planes) tuple of finished lengths.  Returns uint64 [planes, planes]; a `sums` passed in is the starting value (the slices of a
    window accumulate)."""
    kmin, kmax = _span(kmin, kmax)
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
    shape = (max(planes, 0), max(planes, 0))
    start = np.zeros(shape, np.uint64) if sums is None else np.ascontiguousarray(sums, np.uint64)
    if start.shape != shape:
        raise ValueError(f"sums must be [{planes}, {planes}]")
    with DevBuffer(device, 0) if padded is None else DevBuffer.of(padded, device) as owner, DevBuffer.of(start, device) as d_sums:
        _accumulate(d_cells if padded is None else owner.d, L, pitch, planes, kmin, kmax, d_sums.d, device, stream)
        return d_sums.to_host(shape, np.uint64)


def region_pairs(index_path, region, n_docs, *, kmin=1, kmax=None, device=0, slice_positions=None):
    """The shared match lengths of a window of a Parquet MEMBERSHIP index, summed over the window for every pair of genomes and over
    the k of [kmin, kmax] (kmax=None: 2^31 - 1).  The planes come from `memo lengths`' slices, from the right, each slice is
    accumulated into one device matrix where its planes lie, and 8 N^2 bytes are downloaded at the end; the matrix does not depend on
    slice_positions.  `region` is CHR:START-END as `memo query -r` takes it, and what is wrong with it raises what memo_query.main
    raises.  One device.  Returns uint64 [N, N]; an empty window gives zeros and touches no index."""
    n_docs = int(n_docs)
    if not 1 <= n_docs <= N_MAX:
        raise ValueError(f"n_docs must be in [1, {N_MAX}]")
    kmin, kmax = _span(kmin, kmax)
    record, qs, qe = parse_region(region)
    L = qe - qs
    if qs < 0:
        raise ValueError("the window starts before position 0 of the record")
    if L > L_MAX:
        raise ValueError(f"a window of at most {L_MAX} positions")
    if L == 0:
        return np.zeros((n_docs, n_docs), np.uint64)
    feed, buf = region_feed(index_path, record, device)
    with buf, DevBuffer.of(np.zeros((n_docs, n_docs), np.uint64), device) as d_sums:
        for a, b, d_cells, pitch in finished_slices(feed, qs, L, n_docs, kmax, device, slice_positions, halo=0):
            _accumulate(d_cells, b - a, pitch, n_docs, kmin, kmax, d_sums.d, device)
        return d_sums.to_host((n_docs, n_docs), np.uint64)


def mean_lengths(sums, positions):
    """S / L as float64: the mean shared match length per position of the window"""
    return np.asarray(sums).astype(np.float64) / float(positions)
