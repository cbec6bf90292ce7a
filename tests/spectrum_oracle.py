"""The definition `memo spectrum` is tested against, in NumPy, built on tests/lengths_oracle.py.  With len[g][p] the
planes of `memo lengths` at cap = KMAX (the plane is the row's annot) and sel_1 >= sel_2 >= ... >= sel_N per position

    sel_T[p]      = the T-th largest of len[0 .. N)[p]                       a membership index
    sel_T[p]      = min{ len[a][p] : 0 <= a < T }                            a conservation index
    cons(p, k)    = max({ T : sel_T[p] >= k } + {0})                         1 <= k <= KMAX
    exact[k][v]   = #{ p : cons(p, k) = v }                                  0 <= v <= N
    atleast[k][t] = #{ p : sel_t[p] >= k } = sum of exact[k][v] over v >= t  1 <= t <= N
"""
import numpy as np

from tests import lengths_oracle


def sel(planes, kmax, membership):
    """int64 [N, L]: row T - 1 is sel_T, of planes [N, L] (values above kmax taken as kmax)"""
    v = np.minimum(np.asarray(planes, np.int64), kmax)
    if membership:
        return np.sort(v, axis=0)[::-1]
    return np.minimum.accumulate(v, axis=0)


def cons(planes, kmax, membership):
    """int64 [L, kmax]: column k - 1 is cons(p, k).  sel is non-increasing in T, so the largest T with sel_T >= k is the number of
    T with sel_T >= k: the values of sel[:, p] are counted per position and summed from kmax down."""
    s = sel(planes, kmax, membership)
    n, L = s.shape
    # held[p][x] = #{ T : sel_T[p] = x }
    held = np.bincount((np.arange(L)[None, :] * (kmax + 1) + s).ravel(), minlength=L * (kmax + 1)).reshape(L, kmax + 1)
    return np.cumsum(held[:, ::-1], axis=1)[:, ::-1][:, 1:]


def count(cons, n_docs):
    """uint64 [kmax, N + 1] of cons [L, kmax]: row k - 1 is the bincount of column k - 1"""
    L, kmax = cons.shape
    flat = (np.arange(kmax)[None, :] * (n_docs + 1) + cons).ravel()
    return np.bincount(flat, minlength=kmax * (n_docs + 1)).reshape(kmax, n_docs + 1).astype(np.uint64)


def table(planes, kmax, membership):
    """uint64 [kmax, N + 1]: row k - 1 is exact[k]"""
    return count(cons(planes, kmax, membership), np.asarray(planes).shape[0])


def table_by_rank(planes, kmax, membership):
    """table() without cons [L, kmax], in O(N L + N kmax): sel_T does not increase in T, so cons(p, k) >= t exactly when sel_t[p] >= k, and
    atleast[k][t] = #{ p : sel_t[p] >= k } is the count of rank t's values from k up; atleast[k][0] = L, atleast[k][N + 1] = 0, and
    exact[k][v] = atleast[k][v] - atleast[k][v + 1]"""
    s = sel(planes, kmax, membership)
    n, L = s.shape
    least = np.zeros((kmax, n + 2), np.int64)
    least[:, 0] = L
    for t in range(1, n + 1):
        least[:, t] = np.cumsum(np.bincount(s[t - 1], minlength=kmax + 1)[::-1])[::-1][1:]
    return (least[:, :-1] - least[:, 1:]).astype(np.uint64)


def exact(s, e, a, qs, qe, n_docs, kmax, membership):
    return table(lengths_oracle.planes(s, e, a, qs, qe, kmax, n_docs), kmax, membership)


def atleast(exact):
    """uint64 [kmax, N]: column t - 1 is the sum of exact[k][v] over v >= t"""
    exact = np.asarray(exact, np.uint64)
    return np.cumsum(exact[:, ::-1], axis=1, dtype=np.uint64)[:, ::-1][:, 1:]


def text(exact, cumulative=False):
    exact = np.asarray(exact)
    n = exact.shape[1] - 1
    body = atleast(exact) if cumulative else exact
    first = 1 if cumulative else 0
    out = "\t".join(["k"] + [str(v) for v in range(first, n + 1)]) + "\n"
    for k in range(body.shape[0]):
        out += "\t".join([str(k + 1)] + [str(int(c)) for c in body[k]]) + "\n"
    return out.encode()
