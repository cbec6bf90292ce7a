"""The oracle of `memo features`: NumPy on a result that holds the positions first .. first + L -- the unpacked bits B [L, N] of a
membership result, or the vector v [L] of a conservation result -- and features [start, end) in the same coordinates, clipped to it:

    membership     table[f][g] = B[start_f : end_f, g].sum()                                              int64 [F, N]
    conservation   table[f]    = (v[start_f : end_f].sum(), (v[start_f : end_f] >= T).sum())               int64 [F, 2]

in two forms: feature by feature, and through one prefix sum.  And the segment tables the two kernels are checked against."""
import numpy as np


def _clip(starts, ends, first, L):
    return (np.clip(np.asarray(starts, np.int64) - int(first), 0, L), np.clip(np.asarray(ends, np.int64) - int(first), 0, L))


def memb(B, starts, ends, first=0):
    B = np.asarray(B)
    lo, hi = _clip(starts, ends, first, len(B))
    return np.array([B[a:b].sum(axis=0, dtype=np.int64) for a, b in zip(lo, hi)], np.int64).reshape(len(lo), B.shape[1])


def memb_fast(B, starts, ends, first=0):
    B = np.asarray(B)
    lo, hi = _clip(starts, ends, first, len(B))
    cum = np.zeros((len(B) + 1, B.shape[1]), np.int64)
    np.cumsum(B, axis=0, dtype=np.int64, out=cum[1:])
    return cum[hi] - cum[lo]


def cons(v, starts, ends, threshold, first=0):
    v = np.asarray(v, np.int64)
    lo, hi = _clip(starts, ends, first, len(v))
    return np.array([[v[a:b].sum(), (v[a:b] >= threshold).sum()] for a, b in zip(lo, hi)], np.int64).reshape(len(lo), 2)


def cons_fast(v, starts, ends, threshold, first=0):
    v = np.asarray(v, np.int64)
    return memb_fast(np.stack([v, (v >= threshold).astype(np.int64)], axis=1), starts, ends, first)


def inside_ends(starts, ends, k):
    """the ends of -i: only k-mers that lie wholly inside the feature"""
    starts, ends = np.asarray(starts, np.int64), np.asarray(ends, np.int64)
    return np.maximum(starts, ends - k + 1)


def segment_table(v, edges, threshold, first=0):
    """what memo_segment_conservation_dev adds: int64 [2, segs], the edges clipped to the slice"""
    return np.ascontiguousarray(cons(v, np.asarray(edges)[:-1], np.asarray(edges)[1:], threshold, first).T)


def segment_table_fast(v, edges, threshold, first=0):
    return np.ascontiguousarray(cons_fast(v, np.asarray(edges)[:-1], np.asarray(edges)[1:], threshold, first).T)


def feature_sums(table, lo, hi):
    """what memo_feature_sums_dev writes: uint64 [F, rows], modulo 2^64, through numpy.cumsum"""
    table = np.asarray(table, np.uint64)
    cum = np.zeros((table.shape[0], table.shape[1] + 1), np.uint64)
    np.cumsum(table, axis=1, dtype=np.uint64, out=cum[:, 1:])
    return np.ascontiguousarray((cum[:, np.asarray(hi, np.int64)] - cum[:, np.asarray(lo, np.int64)]).T)
