"""CPU references for `memo index` (TEST INFRASTRUCTURE -- checkers of memo_amd/csrc/memo_ms.hip).

* ``ms``          matching statistics by suffix automaton over bytes (ms_oracle.c, in libmemo_oracle.so);
* ``brute_ms``    the same by its definition, substring search in Python (tools/make_golden.py's rule);
* ``check_sa``    the O(n) suffix-array checker of Burkhardt and Kaerkkaeinen, vectorised in NumPy: it checks a
                  suffix array without sorting a single suffix, so it works on homopolymers of 10^8 bytes.

MS[i] of pivot position i against a text is the length of the longest prefix of the pivot's record from i on that
occurs in the text (a NUL-separated genome text, build_index.genome_text, or any other bytes).
"""
import ctypes as C

import numpy as np

from . import memo_oracle

_i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
_i64p = np.ctypeslib.ndpointer(np.int64, flags="C_CONTIGUOUS")
_u8p = np.ctypeslib.ndpointer(np.uint8, flags="C_CONTIGUOUS")

_bound = None


def _lib():
    global _bound
    if _bound is None:
        L = memo_oracle.lib()
        L.oracle_ms.argtypes = [_u8p, C.c_int64, _u8p, _i64p, C.c_int64, _i32p]
        L.oracle_ms.restype = C.c_int
        _bound = L
    return _bound


def _u8(b):
    return np.frombuffer(bytes(b), np.uint8) if not isinstance(b, np.ndarray) else np.ascontiguousarray(b, np.uint8)


def ms(text, pivot, rec_begin):
    """int32 [positions]: MS of the pivot (bytes, records at int64 offsets rec_begin[0 .. nrec]) against text"""
    t, p = _u8(text), _u8(pivot)
    rb = np.ascontiguousarray(rec_begin, np.int64)
    if rb[0] != 0 or rb[-1] != len(p) or np.any(np.diff(rb) < 0):
        raise ValueError("rec_begin must run from 0 to the pivot's length without decreasing")
    out = np.zeros(len(p), np.int32)
    rc = _lib().oracle_ms(t if len(t) else np.zeros(1, np.uint8), len(t), p if len(p) else np.zeros(1, np.uint8),
                          rb, len(rb) - 1, out if len(out) else np.zeros(1, np.int32))
    if rc:
        raise MemoryError(f"oracle_ms: text of {len(t)} bytes refused ({rc})")
    return out


def records_layout(records):
    """(concatenated pivot bytes, int64 rec_begin) of a list of record byte strings"""
    rb = np.zeros(len(records) + 1, np.int64)
    rb[1:] = np.cumsum([len(r) for r in records])
    return b"".join(records), rb


def ms_records(records, text):
    return ms(text, *records_layout(records))


def brute_ms(records, text):
    """the definition (tools/make_golden.py's rule): longest prefix of record[i:] occurring in the text, by
    binary search on the length"""
    out = []
    for rec in records:
        for i in range(len(rec)):
            lo, hi = 0, len(rec) - i
            while lo < hi:
                mid = (lo + hi + 1) // 2
                if rec[i:i + mid] in text:
                    lo = mid
                else:
                    hi = mid - 1
            out.append(lo)
    return np.array(out, np.int32)


def check_sa(text, sa, block=1 << 24):
    """None if sa is the suffix array of text (bytes compared unsigned, a proper prefix sorts first), else a
    message naming the first offending SA slot.  Burkhardt and Kaerkkaeinen: sa is a permutation of [0, n), and
    for every adjacent pair a = sa[x - 1], b = sa[x]: T[a] < T[b], or T[a] == T[b] and rank(a + 1) < rank(b + 1),
    with rank(n), the empty suffix, below every other."""
    t = _u8(text)
    sa = np.asarray(sa)
    n = len(t)
    if sa.shape != (n,):
        return f"suffix array has shape {sa.shape}, the text {n} bytes"
    if n == 0:
        return None
    if sa.dtype.kind not in "iu":
        return f"suffix array of dtype {sa.dtype}"
    if sa.min() < 0 or sa.max() >= n:
        return f"entries outside [0, {n}): min {sa.min()}, max {sa.max()}"
    seen = np.zeros(n, bool)
    seen[sa] = True
    if not seen.all():
        return f"not a permutation: {int(n - seen.sum())} positions missing, e.g. {int(np.argmin(seen))}"
    del seen
    rank = np.empty(n + 1, np.int64 if n >= (1 << 31) - 1 else np.int32)
    rank[n] = 0
    rank[sa] = np.arange(1, n + 1, dtype=rank.dtype)
    for x0 in range(1, n, block):
        a, b = sa[x0 - 1:min(x0 - 1 + block, n - 1)], sa[x0:min(x0 + block, n)]
        ta, tb = t[a], t[b]
        bad = (ta > tb) | ((ta == tb) & (rank[a + 1] >= rank[b + 1]))
        if bad.any():
            x = x0 + int(np.argmax(bad))
            return f"SA[{x - 1}] = {sa[x - 1]} does not sort before SA[{x}] = {sa[x]}"
    return None
