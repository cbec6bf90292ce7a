"""`memo view` preprocessing on the GPU: the per-bin composition of a conservation vector.

Counterpart of /root/reference/src/plot_conservation.py:40-65 (fileReader, preprocess_data).  The two parts that touch
every position run on the device: reading the reference's text file (memo_parse_conservation_text_dev: the file goes to
HBM as it is and is parsed there) and the histogram, straight from a vector that is still in HBM -- a parsed file, or the
result of a sweep that was never written out (preprocess_region).  Normalisation and the long-format table are host-side
and follow the reference line by line:

  reading     [int(line.strip()) for line in open(path)]                        :40-49
              (a text outside the device reader's grammar is read exactly so: _read_text_reference)
  bin edges   list(map(int, np.linspace(0, positions, n_bins + 1)))            :52
  per bin     count[order] / (positions in the bin)  for order in 0..n_docs     :55-56
              (an empty bin raises ZeroDivisionError, as in the reference)
  table       melt over orders, bins innermost; rows of order == n_docs dropped :60-65
The table's writers (TSV, a matplotlib plot) are memo_amd/view_cli.py.
"""
import ctypes as C
import mmap
import os

import numpy as np

from ._device import DevBuffer, on_device
from ._lib import check, lib
from ._window import parse_region


def bin_edges(positions, n_bins):
    return np.array(list(map(int, np.linspace(0, positions, n_bins + 1))), np.int64)


def bin_counts(vec, n_docs, n_bins, device=0, stream=None):
    """uint64 [n_bins, n_docs + 1] histogram.  vec: host uint16 array, or (device pointer, length)."""
    with on_device(vec, np.uint16, device) as (d_vec, L):
        edges = bin_edges(L, n_bins)
        counts = np.zeros((n_bins, n_docs + 1), np.uint64)
        check(lib().memo_bin_conservation_dev(d_vec, L, edges.ctypes.data, n_bins, n_docs, counts.ctypes.data,
                                              device, None if stream is None else C.c_void_p(int(stream))))
    return counts, edges


def read_conservation_text(path):
    """the reference's out.txt: one integer per line, as a host array (read on the host; blank lines and '#' comments are
    skipped here, which the reference refuses -- preprocess_data reads through read_conservation_text_dev)"""
    return np.loadtxt(path, dtype=np.int64, ndmin=1).astype(np.uint16)


def _read_text_reference(path):
    """The reference's own reading (plot_conservation.py:40-49), for texts the device reader hands back: whatever int()
    takes (signs, underscores, any white space) and its ValueError for what it does not.  Values outside [0, 65534] come
    back as 65535: no column of the table counts them, the bin's width does (the reference's Counter)."""
    with open(path, "r") as fh:
        values = [int(line.strip()) for line in fh]
    return np.fromiter((v if 0 <= v < 65535 else 65535 for v in values), np.uint16, len(values))


def read_conservation_text_dev(path, device=0):
    """(device pointer, L, free): the file's L values as uint16 in HBM, free() releases them.  The file is copied to the
    device as it is (memory-mapped, in pieces through the pinned ring) and parsed there; a text outside the device
    reader's grammar (include/memo_amd_dap.h) is read as the reference reads it and uploaded."""
    with open(path, "rb") as fh:
        nbytes = os.fstat(fh.fileno()).st_size
        cap = nbytes // 2 + 1
        vec = DevBuffer(device, 2 * cap)
        lines, odd = C.c_int64(0), C.c_int64(-1)
        try:
            if nbytes:
                with DevBuffer(device, nbytes) as text:
                    with mmap.mmap(fh.fileno(), nbytes, access=mmap.ACCESS_READ) as mm:
                        host = np.frombuffer(mm, np.uint8)
                        try:
                            check(lib().memo_dev_upload_pipelined(device, text.d, host.ctypes.data, nbytes))
                        finally:
                            del host                       # (the map cannot close under an exported buffer)
                    check(lib().memo_parse_conservation_text_dev(text.d, nbytes, vec.d, cap, C.byref(lines), C.byref(odd),
                                                                 device, None))
        except BaseException:
            vec.close()
            raise
    L = lines.value
    if odd.value >= 0:
        vec.close()
        values = _read_text_reference(path)                # (or its ValueError)
        L = len(values)
        vec = DevBuffer.of(values, device)
    return int(vec.d.value), L, vec.close


def _table(counts, edges, n_docs, n_bins):
    """the reference's melted DataFrame from the histogram: dict of arrays 'bin' (int64), 'No. Genomes' (float64),
    'value' (float64), rows ordered as pd.melt leaves them"""
    width = np.diff(edges)
    if np.any(width == 0):
        raise ZeroDivisionError("division by zero")        # Counter of an empty bin (:56)
    value = counts.astype(np.float64) / width[:, None].astype(np.float64)      # [bin, order]
    orders = np.arange(n_docs)                               # order == n_docs is dropped (:65)
    return {"bin": np.tile(np.arange(n_bins, dtype=np.int64), n_docs),
            "No. Genomes": np.repeat(orders.astype(np.float64), n_bins),
            "value": value[:, :n_docs].T.reshape(-1)}


def preprocess_data(vec_or_path, n_docs, n_bins, device=0):
    """Same table as the reference's preprocess_data, from its text file (a path) or from a host vector."""
    if isinstance(vec_or_path, (str, os.PathLike)):
        d_vec, L, free = read_conservation_text_dev(os.fspath(vec_or_path), device)
        try:
            counts, edges = bin_counts((d_vec, L), n_docs, n_bins, device)
        finally:
            free()
    else:
        counts, edges = bin_counts(vec_or_path, n_docs, n_bins, device)
    return _table(counts, edges, n_docs, n_bins)


def preprocess_region(index_path, region, k, n_docs, n_bins, device=0):
    """The same table for a window of a Parquet conservation index, without the text in between: the sweep's result stays
    in HBM and is binned there; only n_bins x (n_docs + 1) counts leave the device.  `region` is CHR:START-END as `memo
    query -r` takes it, and what is wrong with it raises what memo_query.main raises.  One device."""
    from . import memo_query
    record, qs, qe = parse_region(region)
    index = memo_query.region_index(index_path, record, qs, qe + k, device=device, k=k, num_docs=n_docs, membership=False)
    L = qe - qs
    with index, DevBuffer(device, max(2 * L, 8)) as vec:                          # (an empty window has an address too)
        index.conservation_dev(qs, qe, k, n_docs, vec.d.value)
        index.check()
        counts, edges = bin_counts((vec.d.value, L), n_docs, n_bins, device)
    return _table(counts, edges, n_docs, n_bins)
