"""`memo matrix`: pairwise k-mer sharing between genomes, reduced on the GPU.

No counterpart in the reference: its users write the membership text of `memo query -m`, parse it again and take B.T @ B of
the [L, N] bit matrix on the host.  Here the sweep's result stays in HBM, memo_cooccurrence_dev (memo_amd/csrc/memo_cooc.hip)
counts, for every pair of genomes, the positions both hold the k-mer at, and only N x N integers leave the device:

    C[g][h] = #{ p in [0, L) : bit[p][g] = 1 and bit[p][h] = 1 }        uint64 [N, N], symmetric

Genome 0 is the pivot (dap_to_bed.py:113 numbers the others from 1); the diagonal is each genome's own count.  A whole window
is swept in slices into one reused result buffer and accumulated (region_matrix), so its membership result never exists as a
whole.  The flags are memo_amd/matrix_cli.py.
"""
import ctypes as C

import numpy as np

from ._device import DevBuffer, on_device
from ._lib import check, lib
from ._window import membership_slices, parse_region
from .index import words


def tile(words_per_position=1):
    """positions per tile of the sweep: the lengths a test wants to straddle"""
    return int(lib().memo_cooccurrence_tile(int(words_per_position)))


def _accumulate(d_bits, L, num_docs, d_counts, device, stream=None):
    check(lib().memo_cooccurrence_dev(d_bits, L, num_docs, d_counts, device, None if stream is None else C.c_void_p(int(stream))))


def _matrix(num_docs, counts):
    """`counts` as a host matrix uint64 [N, N] (None: zeros)"""
    host = np.zeros((num_docs, num_docs), np.uint64) if counts is None else np.ascontiguousarray(counts, np.uint64)
    if host.shape != (num_docs, num_docs):
        raise ValueError(f"counts must be [{num_docs}, {num_docs}]")
    return host


def cooccurrence(bits, num_docs, counts=None, device=0, stream=None):
    """The co-occurrence matrix of a membership result: a host uint32 array [L, W], or (device pointer, L).  Returns uint64
    [N, N]; a `counts` passed in is the starting value (several windows accumulate)."""
    W = words(num_docs)
    if not isinstance(bits, tuple):
        bits = np.ascontiguousarray(bits, np.uint32).reshape(-1, W)
    with DevBuffer.of(_matrix(num_docs, counts), device) as d_counts, on_device(bits, np.uint32, device) as (d_bits, L):
        _accumulate(d_bits, L, num_docs, d_counts.d, device, stream)
        return d_counts.to_host((num_docs, num_docs), np.uint64)


def region_matrix(index_path, region, k, n_docs, device=0, slice_positions=1 << 24):
    """The co-occurrence matrix of a window of a Parquet MEMBERSHIP index: the window is swept in slices of at most
    `slice_positions` into one reused device buffer of slice_positions x W x 4 bytes, each slice is accumulated into one device
    matrix, and N x N x 8 bytes are downloaded at the end.  A slice is swept as part of its window (membership_slice_dev), so the
    matrix does not depend on the slices.  `region` is CHR:START-END as `memo query -r` takes it, and what is
    wrong with it raises what memo_query.main raises.  One device.  Returns uint64 [N, N]."""
    from . import memo_query
    record, qs, qe = parse_region(region)
    index = memo_query.region_index(index_path, record, qs, qe + k, device=device, k=k, num_docs=n_docs, membership=True)
    with index, DevBuffer.of(_matrix(n_docs, None), device) as d_counts:
        for d_bits, s, e in membership_slices(index, qs, qe, k, n_docs, slice_positions, device):
            _accumulate(d_bits, e - s, n_docs, d_counts.d, device)
        return d_counts.to_host((n_docs, n_docs), np.uint64)


def jaccard(counts):
    """Jaccard distances 1 - C[g][h] / (C[g][g] + C[h][h] - C[g][h]) of a co-occurrence matrix, float64; 0.0 where the union is
    empty (two genomes that hold nothing differ in nothing)"""
    c = np.asarray(counts).astype(np.float64)
    own = np.diag(c)
    union = own[:, None] + own[None, :] - c
    out = np.zeros_like(c)
    np.divide(c, union, out=out, where=union != 0)
    return np.where(union != 0, 1.0 - out, 0.0)


def format_matrix(m, labels=None):
    """tab-separated text, one row per genome: integers as they are, floats by repr (the convention of `memo view`'s .tsv);
    with labels a header line (an empty first field) and a first column"""
    m = np.asarray(m)
    cell = (lambda v: repr(float(v))) if m.dtype.kind == "f" else (lambda v: str(int(v)))
    lines = []
    if labels is not None:
        labels = list(labels)
        if len(labels) != len(m):
            raise ValueError(f"{len(labels)} labels for {len(m)} genomes")
        lines.append("\t".join([""] + labels))
    for i, row in enumerate(m.tolist()):
        fields = [cell(v) for v in row]
        lines.append("\t".join(([labels[i]] if labels is not None else []) + fields))
    return "".join(line + "\n" for line in lines)
