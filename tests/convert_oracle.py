"""The definition `memo convert` is tested against, in NumPy, built on tests/lengths_oracle.py and oracle/dap_oracle.py.

Per record with rows (s, e, a), N genomes and Lrec = max s (or the length given):

    ms[p][g - 1] = min( Lrec - p, len[g][p] )        0 <= p < Lrec, 1 <= g < N;  len: lengths_oracle.planes with qs = 0, qe = Lrec,
                                                                                 cap = min(Lrec, 2^31 - 1)
    rows out     = dap_oracle.dap_rows(ms, [0, Lrec], overlap=True, order=not membership), the annot is the column + 1"""
import numpy as np

from oracle import dap_oracle
from tests import lengths_oracle

L_MAX = 2 ** 31 - 1


def record_length(s, length=None):
    top = int(np.max(s)) if len(s) else 0
    return top if length is None else int(length)


def ms(s, e, a, n_docs, length=None):
    """int64 [Lrec, N - 1]: the matching statistics the membership rows say"""
    L = record_length(s, length)
    planes = lengths_oracle.planes(s, e, a, 0, L, min(L, L_MAX), n_docs).astype(np.int64)
    return np.minimum(planes[1:].T, (L - np.arange(L, dtype=np.int64))[:, None])


def rows(s, e, a, n_docs, order=True, length=None):
    """(start, end, annot) int64: the record's conservation rows (order=True) or its canonical membership rows, in file order"""
    L = record_length(s, length)
    if not L:
        return tuple(np.empty(0, np.int64) for _ in range(3))
    _rec, start, end, annot = dap_oracle.dap_rows(ms(s, e, a, n_docs, length), np.asarray([0, L], np.int64), overlap=True, order=order)
    return start.astype(np.int64), end.astype(np.int64), annot.astype(np.int64)


def carries(s, e, a, length, n_docs, step):
    """{(a, b): int64 [N]}: for every slice [a, b) of [0, length) cut at multiples of `step`, the smallest end per genome among the rows
    with b < start < length + cap, straight from the definition (INT64_MAX: none)"""
    s, e, a = (np.asarray(c, np.int64) for c in (s, e, a))
    reach = length + min(length, L_MAX)
    out = {}
    for lo in range(0, length, step):
        hi = min(lo + step, length)
        carry = np.full(n_docs, np.iinfo(np.int64).max, np.int64)
        for g in range(n_docs):
            ends = e[(a == g) & (s > hi) & (s < reach)]
            if len(ends):
                carry[g] = ends.min()
        out[(lo, hi)] = carry
    return out
