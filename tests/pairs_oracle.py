"""The definition `memo pairs` is tested against, in NumPy, built on tests/lengths_oracle.py.

The cells v are [planes, L] match lengths; with 1 <= kmin <= kmax

    w[g][p] = max(0, min(v[g][p], kmax) - (kmin - 1))          the number of k in [kmin, kmax] at which genome g holds the k-mer at p
    S[g][h] = sum over p of min(w[g][p], w[h][p])              uint64 [planes, planes], symmetric

For a window of a membership index v is lengths_oracle.planes with cap = kmax."""
import numpy as np

from tests import lengths_oracle


def weights(v, kmin, kmax):
    """int64 [planes, L]"""
    v = np.asarray(v, np.int64)
    assert v.ndim == 2
    assert 1 <= kmin <= kmax <= 2 ** 31 - 1
    return np.maximum(np.minimum(v, kmax) - (kmin - 1), 0)


def sums(v, kmin, kmax):
    """uint64 [planes, planes], by np.minimum, row by row"""
    w = weights(v, kmin, kmax)
    out = np.empty((len(w), len(w)), np.uint64)
    for g in range(len(w)):
        out[g] = np.minimum(w[g][None, :], w).sum(axis=1, dtype=np.int64).astype(np.uint64)      # (below 2^31 x 2^31: no wrap)
    return out


def window_sums(s, e, a, qs, qe, kmin, kmax, n_docs):
    """the matrix of the window [qs, qe) of a membership index's rows"""
    return sums(lengths_oracle.planes(s, e, a, qs, qe, kmax, n_docs), kmin, kmax)
