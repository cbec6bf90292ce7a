"""The definition `memo maxk` is tested against, in NumPy:

    out[p - qs] = min( cap, max( 0, min{ e_i - p : pred(a_i), p < s_i, qs < s_i < qe + cap } ) )        cap where the set is empty

pred: 0 <= a < threshold, or a == genome."""
import numpy as np


def maxk(s, e, a, qs, qe, cap, threshold=None, genome=None):
    assert (threshold is None) != (genome is None)
    s, e, a = (np.asarray(c, np.int64) for c in (s, e, a))
    keep = ((a >= 0) & (a < threshold)) if genome is None else (a == genome)
    keep &= (s > qs) & (s < qe + cap)
    s, e = s[keep], e[keep]
    order = np.argsort(s, kind="stable")
    s, e = s[order], e[order]
    p = np.arange(qs, qe, dtype=np.int64)
    out = np.full(len(p), cap, np.int64)
    if len(s):
        ends_from = np.minimum.accumulate(e[::-1])[::-1]          # the smallest end among the rows from this one on
        first = np.searchsorted(s, p, side="right")               # the first row with s > p
        bounded = first < len(s)
        out[bounded] = np.clip(ends_from[first[bounded]] - p[bounded], 0, cap)
    return out.astype(np.uint32)


def text(vec):
    return "".join(f"{int(v)}\n" for v in vec).encode()
