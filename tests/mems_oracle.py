"""The definitions `memo mems` is tested against, in NumPy, built on tests/maxk_oracle.py and tests/lengths_oracle.py.

With v[p] the length of `memo maxk` / `memo lengths` at position p for the chosen mode and cap, position p of [qs, qe) is REPORTED when

    v[p] >= min_len   and   ( p == 0   or   v[p - 1] < v[p]   or   v[p - 1] == v[p] < cap )

as the match [p, p + v[p]).  v[qs - 1] is the true length of the position before the window (the vector is taken on [qs - 1, qe) when
qs > 0), so a window reports exactly the matches that start in it.  The covered bases (`-u`) are the union of [p, p + min_len) over the
positions of the window with v[p] >= min_len, as maximal intervals; the cap plays no part in them."""
import numpy as np

from tests import lengths_oracle, maxk_oracle


def start_mask(v, cap, min_len, halo):
    """The rule on values alone, along the last axis of v: which cells are reported.  halo = 1: cell 0 is only a neighbour and is never
    reported; halo = 0: cell 0 is position 0 of its record."""
    v = np.asarray(v, np.int64)
    start = np.empty(v.shape, bool)
    if v.shape[-1]:
        start[..., 0] = not halo
        start[..., 1:] = (v[..., :-1] < v[..., 1:]) | ((v[..., :-1] == v[..., 1:]) & (v[..., 1:] < cap))
    return start & (v >= min_len)


def starts_of(v, cap, min_len, halo):
    """the reported cells of one plane, ascending"""
    return np.flatnonzero(start_mask(np.asarray(v, np.int64).reshape(-1), cap, min_len, halo))


def band_mask(v, min_len):
    """Along the last axis of v: the cells at which v >= min_len changes, the cell before cell 0 counting as false"""
    key = np.asarray(v, np.int64) >= min_len
    before = np.zeros(key.shape, bool)
    before[..., 1:] = key[..., :-1]
    return key != before


def band_boundaries(v, min_len):
    """one plane's boundaries, ascending: 2j opens an interval, 2j + 1 closes it"""
    return np.flatnonzero(band_mask(np.asarray(v, np.int64).reshape(-1), min_len))


def vector(s, e, a, qs, qe, cap, n_docs, *, threshold=None, genome=None, membership=False):
    """v on [qs, qe): the conservation index at threshold, genome `genome` of a membership index, or (membership and threshold) the
    threshold-th largest of the genomes' lengths"""
    if membership and genome is None:
        return lengths_oracle.kth(s, e, a, qs, qe, cap, n_docs, threshold)
    if membership:
        return maxk_oracle.maxk(s, e, a, qs, qe, cap, genome=genome)
    return maxk_oracle.maxk(s, e, a, qs, qe, cap, threshold=threshold)


def matches(s, e, a, qs, qe, cap, n_docs, *, min_len=1, **mode):
    """(starts, ends) int64, absolute, of the matches that start in [qs, qe)"""
    halo = 1 if qs > 0 else 0
    v = vector(s, e, a, qs - halo, qe, cap, n_docs, **mode).astype(np.int64)
    at = starts_of(v, cap, min_len, halo)
    p = at + (qs - halo)
    return p, p + v[at]


def all_matches(s, e, a, qs, qe, cap, n_docs, *, min_len=1):
    """`-m -a`: [(genome, starts, ends)] for the genomes 1 .. n_docs - 1 (genome 0 is the pivot: it has no rows and is left out)"""
    return [(g, *matches(s, e, a, qs, qe, cap, n_docs, min_len=min_len, membership=True, genome=g)) for g in range(1, n_docs)]


def merge(begin, end):
    """intervals sorted by begin -> the maximal intervals of their union (overlapping or abutting intervals are one)"""
    out = []
    for b, e in zip(np.asarray(begin, np.int64).tolist(), np.asarray(end, np.int64).tolist()):
        if out and b <= out[-1][1]:
            out[-1][1] = max(out[-1][1], e)
        else:
            out.append([b, e])
    arr = np.asarray(out, np.int64).reshape(-1, 2)
    return arr[:, 0].copy(), arr[:, 1].copy()


def union(s, e, a, qs, qe, n_docs, *, min_len=1, **mode):
    """`-u`: (begins, ends) of the bases covered by a stretch of at least min_len that starts in the window.  Runs at cap = min_len."""
    v = vector(s, e, a, qs, qe, min_len, n_docs, **mode)
    p = np.flatnonzero(v >= min_len) + qs
    return merge(p, p + min_len)


def expand(starts, ends, qs, qe):
    """The lengths on [qs, qe) from the list at min_len = 1: v[p] = max(0, v[p_i] - (p - p_i)) from a start to the next (lossless where
    no value is the cap and the rows have end >= start)"""
    out = np.zeros(qe - qs, np.int64)
    starts, ends = np.asarray(starts, np.int64), np.asarray(ends, np.int64)
    nxt = np.append(starts[1:], qe)
    for p, q, n in zip(starts.tolist(), ends.tolist(), nxt.tolist()):
        at = np.arange(p, n)
        out[at - qs] = np.maximum(0, q - at)
    return out


def text(record, starts, ends, genome=None):
    """REC  start  end  [genome] lines"""
    tail = "" if genome is None else f"\t{int(genome)}"
    return "".join(f"{record}\t{int(b)}\t{int(e)}{tail}\n" for b, e in zip(starts, ends)).encode()
