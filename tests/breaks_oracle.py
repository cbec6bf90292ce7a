"""The definition `memo breaks` is tested against, in NumPy, built on tests/mems_oracle.py.

The cells v are [planes, L]; with halo = 1 cell 0 of every plane is only the left neighbour of cell 1 and is not counted, with
halo = 0 it is position 0 of its record.  Counted cell i is position first + i - halo, and with bins + 1 non-decreasing edges in the
same coordinates that hold every counted position

    table[0][g][b] = #{ counted p, edges[b] <= p < edges[b + 1] : v[p] >= min_len and p starts a match }     mems_oracle.start_mask
    table[1][g][b] = sum of v[p] over the same p                                                             (min_len plays no part)

Two forms: table() by prefix sums cut at the edges, naive() one position at a time."""
import numpy as np

from tests import mems_oracle


def table(v, edges, cap, min_len=1, halo=0, first=0):
    """uint64 [2, planes, bins]"""
    v = np.asarray(v, np.int64)
    v = v.reshape(-1, v.shape[-1])
    edges = np.asarray(edges, np.int64)
    flags = mems_oracle.start_mask(v, cap, min_len, halo)[:, halo:].astype(np.int64)
    values = v[:, halo:]
    n = values.shape[1]
    assert (np.diff(edges) >= 0).all() and edges[0] <= first and first + n <= edges[-1]
    cut = np.clip(edges - first, 0, n)
    out = np.empty((2, v.shape[0], len(edges) - 1), np.uint64)
    for which, x in enumerate((flags, values)):
        prefix = np.concatenate([np.zeros((v.shape[0], 1), np.int64), np.cumsum(x, axis=1)], axis=1)
        out[which] = (prefix[:, cut[1:]] - prefix[:, cut[:-1]]).astype(np.uint64)
    return out


def naive(v, edges, cap, min_len=1, halo=0, first=0):
    """the same, one position at a time, the rule spelled out"""
    v = np.asarray(v, np.int64)
    v = v.reshape(-1, v.shape[-1])
    edges = [int(x) for x in edges]
    bins = len(edges) - 1
    out = np.zeros((2, v.shape[0], bins), np.uint64)
    for g, row in enumerate(v.tolist()):
        for i in range(halo, len(row)):
            p = first + i - halo
            hit = [b for b in range(bins) if edges[b] <= p < edges[b + 1]]
            assert len(hit) == 1, "every counted position lies in exactly one bin"
            cur = row[i]
            if i == 0:
                starts = True                                # (halo = 0: position 0 of its record)
            else:
                starts = row[i - 1] < cur or (row[i - 1] == cur and cur < cap)
            out[0, g, hit[0]] += np.uint64(1 if starts and cur >= min_len else 0)
            out[1, g, hit[0]] += np.uint64(cur)
    return out


def window_planes(s, e, a, qs, qe, cap, n_docs, threshold=None):
    """(cells [R, L + halo], halo) of the window [qs, qe) with its left neighbour where qs > 0: every genome's plane of a membership
    index (threshold None), or the one plane of a conservation index at `threshold`"""
    from tests import lengths_oracle, maxk_oracle
    halo = 1 if qs > 0 else 0
    if threshold is None:
        return lengths_oracle.planes(s, e, a, qs - halo, qe, cap, n_docs), halo
    return maxk_oracle.maxk(s, e, a, qs - halo, qe, cap, threshold=threshold).reshape(1, -1), halo


def window_table(s, e, a, qs, qe, edges, cap, n_docs, *, min_len=1, threshold=None):
    """the table of the window [qs, qe) with absolute edges"""
    cells, halo = window_planes(s, e, a, qs, qe, cap, n_docs, threshold)
    return table(cells, edges, cap, min_len, halo, qs)
