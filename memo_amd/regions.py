"""`memo regions`: a query result as intervals, run-coded on the GPU.

No counterpart in the reference: its users run-length the text of `memo query` (src/memo_query.py:65-71) on the host.  Here
the sweep's result stays in HBM, memo_runs_*_dev (memo_amd/csrc/memo_runs.hip) compacts its maximal runs of equal key there,
and only the runs are downloaded.  Three keys:

  value   runs of equal conservation value       starts [R] int64, values [R] uint16          (lossless)
  band    lo <= value <= hi                      boundaries [R] int64: 2j opens an interval, 2j + 1 closes it,
                                                 an odd R leaves the last interval to end at L
  bits    runs of equal membership rows          starts [R] int64, run_bits [R, W] uint32

Starts are offsets from the window start.  The text forms (bedGraph, BED3, BED + one character per genome) are written by
memo_emit_runs / memo_emit_membership_runs (memo_amd/csrc/memo_emit.cpp); the flags are memo_amd/regions_cli.py.
"""
import collections
import ctypes as C

import numpy as np

from ._device import DevBuffer, emit_text, on_device
from ._lib import check, lib
from ._window import parse_region
from .index import words

Runs = collections.namedtuple("Runs", "record qs L starts values run_bits num_docs")
Runs.__doc__ = """region_runs' result: `starts` as runs() / membership_runs() return them; values is None for a band and for
membership, run_bits is None for conservation"""


def tile(words_per_position=0):
    """positions per tile of the three passes (0: a conservation result): the lengths a test wants to straddle"""
    return int(lib().memo_runs_tile(int(words_per_position)))


def runs(vec, mode="value", lo=None, hi=None, device=0, stream=None):
    """Runs of a conservation vector: a host uint16 array, or (device pointer, L).  mode "value": (starts, values); mode
    "band": the boundaries of lo <= value <= hi (one int64 array)."""
    if mode not in ("value", "band"):
        raise ValueError("mode must be 'value' or 'band'")
    band = mode == "band"
    if band and (lo is None or hi is None):
        raise ValueError("a band needs lo and hi")
    d_starts, d_values, n = C.c_void_p(), C.c_void_p(), C.c_uint64(0)
    with on_device(vec, np.uint16, device) as (d_vec, L):
        check(lib().memo_runs_conservation_dev(d_vec, L, 1 if band else 0, int(lo) if band else 0, int(hi) if band else 0,
                                               C.byref(d_starts), None if band else C.byref(d_values), C.byref(n), device,
                                               None if stream is None else C.c_void_p(int(stream))))
    with DevBuffer.adopt(d_starts, device) as b_starts, DevBuffer.adopt(d_values, device) as b_values:
        starts = b_starts.to_host(n.value, np.int64)
        return starts if band else (starts, b_values.to_host(n.value, np.uint16))


def membership_runs(bits, num_docs, device=0, stream=None):
    """Runs of equal rows of a membership result: a host uint32 array [L, W], or (device pointer, L).  (starts, run_bits [R, W])."""
    W = words(num_docs)
    if not isinstance(bits, tuple):
        bits = np.ascontiguousarray(bits, np.uint32).reshape(-1, W)
    d_starts, d_rows, n = C.c_void_p(), C.c_void_p(), C.c_uint64(0)
    with on_device(bits, np.uint32, device) as (d_bits, L):
        check(lib().memo_runs_membership_dev(d_bits, L, num_docs, C.byref(d_starts), C.byref(d_rows), C.byref(n), device,
                                             None if stream is None else C.c_void_p(int(stream))))
    with DevBuffer.adopt(d_starts, device) as b_starts, DevBuffer.adopt(d_rows, device) as b_rows:
        return b_starts.to_host(n.value, np.int64), b_rows.to_host((n.value, W), np.uint32)


def band_intervals(boundaries, L):
    """(begin, end) offsets of a band's intervals from its boundaries"""
    b = np.asarray(boundaries, np.int64)
    if len(b) & 1:
        b = np.append(b, np.int64(L))
    return b[0::2], b[1::2]


def expand(starts, values, L):
    """the vector (or the rows) the runs came from"""
    lengths = np.diff(np.append(np.asarray(starts, np.int64), np.int64(L)))
    return np.repeat(values, lengths, axis=0)


def region_runs(index_path, region, k, n_docs, membership=False, lo=None, hi=None, device=0):
    """The runs of a window of a Parquet index, without the vector in between: the sweep's result stays in HBM and is
    run-coded there; only the runs leave the device.  `region` is CHR:START-END as `memo query -r` takes it, and what is
    wrong with it raises what memo_query.main raises.  lo and / or hi: the band lo <= value <= hi (lo defaults to 0, hi to
    n_docs); membership: runs of equal rows.  One device.  Returns Runs."""
    from . import memo_query
    if membership and (lo is not None or hi is not None):
        raise ValueError("a band is a question about conservation values, not about membership rows")
    record, qs, qe = parse_region(region)
    band = lo is not None or hi is not None
    index = memo_query.region_index(index_path, record, qs, qe + k, device=device, k=k, num_docs=n_docs, membership=membership)
    L = qe - qs
    with index, DevBuffer(device, max(L * (4 * words(n_docs) if membership else 2), 8)) as vec:       # (an empty window has an address too)
        if membership:
            index.membership_dev(qs, qe, k, n_docs, vec.d.value)
            index.check()
            starts, rows = membership_runs((vec.d.value, L), n_docs, device)
            return Runs(record, qs, L, starts, None, rows, n_docs)
        index.conservation_dev(qs, qe, k, n_docs, vec.d.value)
        index.check()
        if band:
            starts = runs((vec.d.value, L), "band", 0 if lo is None else lo, n_docs if hi is None else hi, device)
            return Runs(record, qs, L, starts, None, None, n_docs)
        starts, values = runs((vec.d.value, L), "value", device=device)
        return Runs(record, qs, L, starts, values, None, n_docs)


def emit_runs(record, qs, L, starts, values=None):
    """bedGraph lines (values given) or BED3 lines of a band's intervals (values None), as a uint8 array"""
    s = np.ascontiguousarray(starts, np.int64)
    v = None if values is None else np.ascontiguousarray(values, np.uint16)
    return emit_text(lambda buf, cap: lib().memo_emit_runs(record.encode(), qs, L, s.ctypes.data, None if v is None else v.ctypes.data,
                                                       len(s), buf, cap))


def emit_membership_runs(record, qs, L, starts, run_bits, num_docs):
    """REC start end 0110... lines (num_docs characters, genome 0 first), as a uint8 array"""
    s = np.ascontiguousarray(starts, np.int64)
    b = np.ascontiguousarray(run_bits, np.uint32)
    return emit_text(lambda buf, cap: lib().memo_emit_membership_runs(record.encode(), qs, L, s.ctypes.data, b.ctypes.data, len(s),
                                                                  num_docs, buf, cap))


def emit(result):
    """the text of a region_runs result"""
    if result.run_bits is not None:
        return emit_membership_runs(result.record, result.qs, result.L, result.starts, result.run_bits, result.num_docs)
    return emit_runs(result.record, result.qs, result.L, result.starts, result.values)
