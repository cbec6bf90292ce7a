"""The definition `memo nearest` is tested against, in NumPy.

The cells are [planes, L], plane 0 the pivot's; v = min(cells, cap); cell i is position first + i.  With a candidate set C of
1 .. planes - 1 (None: all of them), per position

    best = max of v over C        ok = best >= min_len        att[g] = g in C and ok and v[g] == best
    sole[g] = att[g] and exactly one genome attains          winner = the smallest g with att[g], 0 where not ok

and per bin of bins + 1 non-decreasing edges in the positions' coordinates that hold the slice

    wins[0][g][b] = #att[g]   wins[1][g][b] = #sole[g]   (g >= 1)      wins[0][0][b] = wins[1][0][b] = #(not ok)      sums[b] = sum of best

Two forms: table() / winners() vectorised, naive() one position at a time."""
import numpy as np


def _candidates(candidates, planes):
    c = list(range(1, planes)) if candidates is None else sorted(int(g) for g in candidates)
    assert c and c[0] >= 1 and c[-1] < planes and len(set(c)) == len(c)
    return np.asarray(c, np.int64)


def per_position(v, cap, min_len=1, candidates=None):
    """(best int64 [L], ok bool [L], att bool [planes, L], sole bool [planes, L], winner uint16 [L])"""
    v = np.minimum(np.asarray(v, np.int64), cap)
    planes, L = v.shape
    c = _candidates(candidates, planes)
    best = v[c].max(axis=0) if L else np.zeros(0, np.int64)
    ok = best >= min_len
    att = np.zeros((planes, L), bool)
    att[c] = (v[c] == best[None, :]) & ok[None, :]
    sole = att & (att.sum(axis=0) == 1)[None, :]
    winner = np.where(ok, att.argmax(axis=0), 0).astype(np.uint16)
    return best, ok, att, sole, winner


def _cut(edges, first, L):
    edges = np.asarray(edges, np.int64)
    assert (np.diff(edges) >= 0).all() and edges[0] <= first and first + L <= edges[-1]
    return np.clip(edges - first, 0, L)


def _binned(x, cut):
    prefix = np.concatenate([np.zeros(x.shape[:-1] + (1,), np.int64), np.cumsum(x.astype(np.int64), axis=-1)], axis=-1)
    return (prefix[..., cut[1:]] - prefix[..., cut[:-1]]).astype(np.uint64)


def table(v, edges, cap, min_len=1, candidates=None, first=0):
    """(wins uint64 [2, planes, bins], sums uint64 [bins])"""
    best, ok, att, sole, _ = per_position(v, cap, min_len, candidates)
    cut = _cut(edges, first, len(best))
    wins = np.stack([_binned(att, cut), _binned(sole, cut)])
    wins[:, 0] = _binned(~ok, cut)
    return wins, _binned(best, cut)


def winners(v, cap, min_len=1, candidates=None):
    """uint16 [L]"""
    return per_position(v, cap, min_len, candidates)[4]


def run_code(vec):
    """(starts int64 [R], values [R]) of the maximal runs of equal value"""
    vec = np.asarray(vec)
    if not len(vec):
        return np.zeros(0, np.int64), vec[:0]
    starts = np.concatenate([[0], np.flatnonzero(vec[1:] != vec[:-1]) + 1]).astype(np.int64)
    return starts, vec[starts]


def naive(v, edges, cap, min_len=1, candidates=None, first=0):
    """(wins, sums, winner), one position at a time, the definition spelled out"""
    rows = [[min(int(x), cap) for x in row] for row in np.asarray(v).tolist()]
    planes, L = len(rows), len(rows[0])
    c = list(range(1, planes)) if candidates is None else sorted(int(g) for g in candidates)
    edges = [int(x) for x in edges]
    bins = len(edges) - 1
    wins, sums, winner = np.zeros((2, planes, bins), np.uint64), np.zeros(bins, np.uint64), np.zeros(L, np.uint16)
    for i in range(L):
        p = first + i
        hit = [b for b in range(bins) if edges[b] <= p < edges[b + 1]]
        assert len(hit) == 1, "every position lies in exactly one bin"
        b = hit[0]
        best = max(rows[g][i] for g in c)
        sums[b] += np.uint64(best)
        if best < min_len:
            wins[0, 0, b] += np.uint64(1)
            wins[1, 0, b] += np.uint64(1)
            continue
        attain = [g for g in c if rows[g][i] == best]
        winner[i] = attain[0]
        for g in attain:
            wins[0, g, b] += np.uint64(1)
        if len(attain) == 1:
            wins[1, attain[0], b] += np.uint64(1)
    return wins, sums, winner


def window_planes(s, e, a, qs, qe, cap, n_docs):
    """every genome's plane of the window [qs, qe) of a membership index's rows"""
    from tests import lengths_oracle
    return lengths_oracle.planes(s, e, a, qs, qe, cap, n_docs)


def window_table(s, e, a, qs, qe, edges, cap, n_docs, *, min_len=1, candidates=None):
    """(wins, sums) of the window with absolute edges"""
    return table(window_planes(s, e, a, qs, qe, cap, n_docs), edges, cap, min_len, candidates, qs)


def window_winners(s, e, a, qs, qe, cap, n_docs, *, min_len=1, candidates=None):
    """(starts from qs, winners) of the window's runs"""
    return run_code(winners(window_planes(s, e, a, qs, qe, cap, n_docs), cap, min_len, candidates))
