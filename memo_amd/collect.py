"""`memo collect`: core and covered k-mer curves over genome orders (the collector's curve), reduced on the GPU.

No counterpart in the reference: its users write the membership text of `memo query -m`, parse it again and run
np.logical_and.accumulate over the [L, N] bit matrix once per order on the host.  Here the sweep's result stays in HBM,
memo_collect_dev (memo_amd/csrc/memo_collect.hip) walks every order over the per-genome bit planes, and only orders x steps integers
leave the device.  For an order q (a row of genome ids) and its step j:

    core   [q][j] = #{ p in [0, L) : bit[p][orders[q][i]] = 1 for every i <= j }
    covered[q][j] = #{ p in [0, L) : bit[p][orders[q][i]] = 1 for some  i <= j }        uint64 [P, M]

Genome 0 is the pivot (it holds every k-mer of its own, so the orders of `orders()` leave it out: the curve starts from it).
A whole window is swept in slices into one reused result buffer and accumulated (region_curves), as matrix.region_matrix
does it.  The flags are memo_amd/collect_cli.py.
"""
import ctypes as C

import numpy as np

from ._device import DevBuffer, on_device
from ._lib import check, lib
from ._window import membership_slices, parse_region
from .index import words


def tile(words_per_position=1):
    """positions per tile of the sweep at that many genome words: the lengths a test wants to straddle"""
    return int(lib().memo_collect_tile(int(words_per_position)))


def orders(n_docs, perms=0, seed=0):
    """The orders of `memo collect`, uint16 [P, N - 1], the pivot left out: perms = 0 is the index order 1 .. N - 1 alone,
    perms = P >= 1 are P rows default_rng(seed).permutation(N - 1) + 1, drawn in sequence from one generator."""
    n_docs, perms = int(n_docs), int(perms)
    if n_docs < 1 or n_docs > 65535:
        raise ValueError("n_docs must be in [1, 65535]")
    if perms < 0:
        raise ValueError("perms must be at least 0")
    if perms == 0:
        return np.arange(1, n_docs, dtype=np.uint16)[None, :]
    rng = np.random.default_rng(seed)
    return np.array([rng.permutation(n_docs - 1) + 1 for _ in range(perms)], np.uint16).reshape(perms, n_docs - 1)


def _as_orders(order_rows):
    rows = np.asarray(order_rows)
    if rows.ndim != 2:
        raise ValueError("orders must be [P, M]")
    if rows.size and (rows.min() < 0 or rows.max() > 65535):
        raise ValueError("a genome id of an order is outside [0, 65535]")
    return np.ascontiguousarray(rows, np.uint16)


def _curve(shape, start):
    """`start` as a host array uint64 [P, M] (None: zeros)"""
    host = np.zeros(shape, np.uint64) if start is None else np.ascontiguousarray(start, np.uint64)
    if host.shape != tuple(shape):
        raise ValueError(f"a starting curve must be {list(shape)}")
    return host


def _accumulate(d_bits, L, num_docs, order_rows, d_core, d_covered, device, stream=None):
    """order_rows: uint16 [P, M], C-contiguous, on the host (the library checks and uploads them)"""
    P, M = order_rows.shape
    check(lib().memo_collect_dev(d_bits, L, num_docs, order_rows.ctypes.data, P, M, d_core, d_covered, device,
                                 None if stream is None else C.c_void_p(int(stream))))


def curves(bits, num_docs, orders, core=None, covered=None, device=0, stream=None):
    """The curves of a membership result: a host uint32 array [L, W], or (device pointer, L).  `orders` is [P, M] genome ids.
    Returns (core, covered), uint64 [P, M] each; a `core` / `covered` passed in is the starting value (several windows
    accumulate)."""
    W = words(num_docs)
    rows = _as_orders(orders)
    if not isinstance(bits, tuple):
        bits = np.ascontiguousarray(bits, np.uint32).reshape(-1, W)
    with DevBuffer.of(_curve(rows.shape, core), device) as d_core, DevBuffer.of(_curve(rows.shape, covered), device) as d_covered, \
            on_device(bits, np.uint32, device) as (d_bits, L):
        _accumulate(d_bits, L, num_docs, rows, d_core.d, d_covered.d, device, stream)
        return d_core.to_host(rows.shape, np.uint64), d_covered.to_host(rows.shape, np.uint64)


def region_curves(index_path, region, k, n_docs, orders, device=0, slice_positions=1 << 24):
    """The curves of a window of a Parquet MEMBERSHIP index over `orders` ([P, M] genome ids): the window is swept in slices of at
    most `slice_positions` into one reused device buffer, each slice is accumulated into the two device curves, and 2 x P x M x 8
    bytes are downloaded at the end.  A slice is swept as part of its window (membership_slice_dev), so the curves do not depend on
    the slices.  One device.  Returns (core, covered), uint64 [P, M] each; orders without a step (N = 1) or without a row touch no
    device."""
    from . import memo_query
    record, qs, qe = parse_region(region)
    rows = _as_orders(orders)
    if not rows.size:
        return np.zeros(rows.shape, np.uint64), np.zeros(rows.shape, np.uint64)
    index = memo_query.region_index(index_path, record, qs, qe + k, device=device, k=k, num_docs=n_docs, membership=True)
    with index, DevBuffer.of(_curve(rows.shape, None), device) as d_core, DevBuffer.of(_curve(rows.shape, None), device) as d_covered:
        for d_bits, s, e in membership_slices(index, qs, qe, k, n_docs, slice_positions, device):
            _accumulate(d_bits, e - s, n_docs, rows, d_core.d, d_covered.d, device)
        return d_core.to_host(rows.shape, np.uint64), d_covered.to_host(rows.shape, np.uint64)


def format_curves(L, core, covered, form="curve", orders=None, labels=None):
    """Tab-separated text with a header line; `genomes` counts the pivot, so every curve starts with the pivot alone: core L,
    covered 0 (nothing seen in another genome yet).
      form "curve"  genomes core covered            the first order
      form "band"   genomes core_min core_mean core_max covered_min covered_mean covered_max      over the P orders; integers as
                    they are, means as repr(float(sum / P))
      form "long"   order genomes core covered      every order in turn
    With labels (one per genome, the pivot first) and the orders, "curve" and "long" get a last column `added`: the genome a step
    adds, the pivot on the first row."""
    core, covered = np.asarray(core), np.asarray(covered)
    if core.ndim != 2 or core.shape != covered.shape:
        raise ValueError("core and covered must be [P, M] alike")
    P, M = core.shape
    L = int(L)
    core, covered = core.tolist(), covered.tolist()
    if labels is not None:
        labels = list(labels)
        if form == "band":
            raise ValueError("a band has no genome to name")
        if orders is None or np.asarray(orders).shape != (P, M):
            raise ValueError("labels need the orders the curves were taken over")
        orders = np.asarray(orders).tolist()
    added = (lambda q, j: [labels[0] if j < 0 else labels[orders[q][j]]]) if labels is not None else (lambda q, j: [])
    if form == "curve":
        if P < 1:
            raise ValueError("no order")
        lines = [["genomes", "core", "covered"] + (["added"] if labels is not None else []), ["1", str(L), "0"] + added(0, -1)]
        lines += [[str(j + 2), str(core[0][j]), str(covered[0][j])] + added(0, j) for j in range(M)]
    elif form == "long":
        lines = [["order", "genomes", "core", "covered"] + (["added"] if labels is not None else [])]
        for q in range(P):
            lines.append([str(q), "1", str(L), "0"] + added(q, -1))
            lines += [[str(q), str(j + 2), str(core[q][j]), str(covered[q][j])] + added(q, j) for j in range(M)]
    elif form == "band":
        if P < 1:
            raise ValueError("no order")
        lines = [["genomes", "core_min", "core_mean", "core_max", "covered_min", "covered_mean", "covered_max"],
                 ["1", str(L), repr(float(L)), str(L), "0", repr(0.0), "0"]]
        for j in range(M):
            a, o = [core[q][j] for q in range(P)], [covered[q][j] for q in range(P)]
            lines.append([str(j + 2), str(min(a)), repr(float(sum(a) / P)), str(max(a)), str(min(o)), repr(float(sum(o) / P)), str(max(o))])
    else:
        raise ValueError(f"unknown form {form!r}")
    return "".join("\t".join(fields) + "\n" for fields in lines)
