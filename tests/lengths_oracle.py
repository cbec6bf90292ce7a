"""The definition `memo lengths` is tested against, in NumPy, built on tests/maxk_oracle.py:

    len[g][p - qs] = min( cap, max( 0, min{ e_i - p : a_i = g, p < s_i, qs < s_i < qe + cap } ) )        0 <= g < N, cap where the set is empty
    sel_T[p - qs]  = the T-th largest of { len[g][p - qs] : 0 <= g < N }                                  1 <= T <= N

and the slice-and-carry scheme the product runs a long window with, restated on the host (sliced_planes)."""
import numpy as np

from tests import maxk_oracle


def planes(s, e, a, qs, qe, cap, n_docs):
    """uint32 [N, qe - qs]: len[g] is maxk_oracle.maxk(genome=g)"""
    out = np.empty((n_docs, max(qe - qs, 0)), np.uint32)
    for g in range(n_docs):
        out[g] = maxk_oracle.maxk(s, e, a, qs, qe, cap, genome=g)
    return out


def select(values, threshold, cap=None):
    """the threshold-th largest over the rows of values [N, L] (values above cap taken as cap), by np.sort"""
    values = np.asarray(values, np.uint32)
    if cap is not None:
        values = np.minimum(values, np.uint32(cap))
    assert 1 <= threshold <= values.shape[0]
    return np.sort(values, axis=0)[values.shape[0] - threshold].astype(np.uint32)


def kth(s, e, a, qs, qe, cap, n_docs, threshold):
    return select(planes(s, e, a, qs, qe, cap, n_docs), threshold)


def sliced_planes(s, e, a, qs, qe, cap, n_docs, step):
    """The planes of [qs, qe) in slices of `step` positions from the right, every row taken once: an int64 carry per genome holds the
    smallest end among the rows right of the slice (seeded from the tail qe < s < qe + cap; INT64_MAX: none) and stands in the slice's
    last cell; the slice itself takes the rows a < s <= b.  Cells are relative to the slice and saturated to its identity."""
    s, e, a = (np.asarray(c, np.int64) for c in (s, e, a))
    L = qe - qs
    out = np.empty((n_docs, L), np.uint32)
    none = np.iinfo(np.int64).max
    carry = np.full(n_docs, none, np.int64)
    known = (a >= 0) & (a < n_docs)

    def into_carry(lo, hi):
        take = known & (s > lo) & (s < hi)
        np.minimum.at(carry, a[take], e[take])
    if L <= 0:
        return out
    into_carry(qe, qe + cap)
    for lo in range(qs + (L - 1) // step * step, qs - 1, -step):
        hi = min(lo + step, qe)
        n = hi - lo
        ident = n - 1 + cap
        cell = np.full((n_docs, n), ident, np.int64)
        have = carry != none
        cell[have, n - 1] = np.clip(carry[have] - lo, 0, ident)
        take = known & (s > lo) & (s <= hi)
        np.minimum.at(cell, (a[take], np.minimum(s[take] - 1 - lo, n - 1)), np.clip(e[take] - lo, 0, ident))
        bound = np.minimum.accumulate(cell[:, ::-1], axis=1)[:, ::-1]
        i = np.arange(n, dtype=np.int64)
        out[:, lo - qs:hi - qs] = np.where(bound > i, np.minimum(bound - i, cap), 0)
        into_carry(lo, hi + 1)
    return out


def text(vec):
    return maxk_oracle.text(vec)


def rows_text(planes):
    """line p: planes[0][p] ... planes[N - 1][p], blank-separated"""
    planes = np.asarray(planes)
    return "".join(" ".join(str(int(v)) for v in planes[:, p]) + "\n" for p in range(planes.shape[1])).encode()
