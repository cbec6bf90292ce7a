"""`memo spectrum`: how many positions of a window are held by exactly v genomes, at EVERY k-mer size from 1 to a cap, in one pass
over the index rows, on the GPU.

No counterpart in the reference.  With N genomes, a window [qs, qe), 1 <= kmax <= 1024 and the planes of `memo lengths` at cap = kmax
(memo_amd/lengths.py; the plane is the row's annot), per position p (memo_amd/csrc/memo_spectrum.hip)

    sel_T[p]    = the T-th largest of len[0 .. N)[p]                  a membership index: `memo lengths -t T`
    sel_T[p]    = min{ len[a][p] : 0 <= a < T }                       a conservation index: `memo maxk -t T`
    cons(p, k)  = max({ T : sel_T[p] >= k } + {0})                    1 <= k <= kmax
    exact[k][v] = #{ p : cons(p, k) = v }                             0 <= v <= N

For rows with end >= start exact[k] is numpy.bincount of what `memo query -k k` writes for the window on a conservation index, and of
the one-bit counts of what `memo query -m -k k` writes on a membership index.  Nothing in an index tells the two kinds apart: the
caller says which it is.  The planes stay on the device, slice by slice (lengths.finished_slices); every slice is added into one table
there, and kmax (N + 1) integers leave it.  The result depends neither on the slicing nor on the cut of the rows into chunks.  The
flags are memo_amd/spectrum_cli.py.
"""
import numpy as np

from ._device import DevBuffer
from ._lib import check, lib
from .lengths import N_MAX, docs, finished_slices, host_feed, pitch_of, region_feed, region_window
from .maxk import window

KMAX_MAX = 1024


def tile(n_docs, kmax, membership):
    """positions per tile of the kernel at that shape: the lengths a test wants to straddle"""
    return int(lib().memo_spectrum_tile(int(n_docs), int(kmax), 1 if membership else 0))


def _kmax(kmax):
    kmax = int(kmax)
    if not 1 <= kmax <= KMAX_MAX:
        raise ValueError(f"kmax must be in [1, {KMAX_MAX}]")
    return kmax


class _Table:
    """the difference table of one window on the device, between memo_spectrum_begin_dev and memo_spectrum_finish_dev"""

    def __init__(self, n_docs, kmax, membership, device):
        self.n, self.kmax, self.mode, self.device = n_docs, kmax, 1 if membership else 0, device
        self.scratch = DevBuffer(device, int(lib().memo_spectrum_scratch_bytes(n_docs, kmax)))
        try:
            check(lib().memo_spectrum_begin_dev(self.scratch.d, n_docs, kmax, device, None))
        except BaseException:
            self.scratch.close()
            raise

    def add(self, d_cells, L, pitch):
        check(lib().memo_spectrum_add_dev(d_cells, L, pitch, self.n, self.kmax, self.mode, self.scratch.d, self.device, None))

    def finish(self):
        shape = (self.kmax, self.n + 1)
        with DevBuffer(self.device, 8 * shape[0] * shape[1]) as d_exact:
            check(lib().memo_spectrum_finish_dev(self.scratch.d, self.n, self.kmax, d_exact.d, self.device, None))
            return d_exact.to_host(shape, np.uint64)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.scratch.close()


def table(planes, kmax, membership, device=0):
    """The kernel alone on host values: the table of `planes` (uint32 [N, L]; values above kmax are taken as kmax).  Returns uint64
    [kmax, N + 1]: row k - 1 is exact[k]."""
    planes = np.asarray(planes, np.uint32)
    if planes.ndim != 2:
        raise ValueError("planes must be [n_docs, positions]")
    n_docs, kmax = docs(planes.shape[0]), _kmax(kmax)
    L = planes.shape[1]
    pitch = pitch_of(L)
    padded = np.zeros((n_docs, pitch), np.uint32)
    padded[:, :L] = planes
    with DevBuffer(device, padded.nbytes) as cells, _Table(n_docs, kmax, membership, device) as tab:
        if L:
            check(lib().memo_dev_upload(device, cells.d, padded.ctypes.data, padded.nbytes, None))
        tab.add(cells.d, L, pitch)
        return tab.finish()


def _exact(feed, buf, qs, L, n_docs, kmax, membership, device, slice_positions):
    with buf, _Table(n_docs, kmax, membership, device) as tab:
        for a, b, d_cells, pitch in finished_slices(feed, qs, L, n_docs, kmax, device, slice_positions):
            tab.add(d_cells, b - a, pitch)
        return tab.finish()


def exact(start, end, annot, qs, qe, n_docs, *, kmax, membership, device=0, chunk_rows=None, slice_positions=None):
    """exact[k][v] of the window [qs, qe) from host columns (any order; rows outside qs < start < qe + kmax and annots outside
    [0, n_docs) are ignored).  chunk_rows: feed the rows in calls of that many; slice_positions: take the window in slices of that many
    positions (the result depends on neither).  Returns uint64 [kmax, n_docs + 1]: row k - 1 is exact[k]."""
    n_docs, kmax = docs(n_docs), _kmax(kmax)
    qs, L, _ = window(qs, qe, kmax)
    feed, buf = host_feed(start, end, annot, chunk_rows, device, (qs, min(qs + L + kmax, 2 ** 62)))
    return _exact(feed, buf, qs, L, n_docs, kmax, membership, device, slice_positions)


def region_exact(index_path, region, n_docs, kmax=128, membership=False, device=0, slice_positions=None):
    """exact[k][v] of a window of a Parquet index.  `region` is CHR:START-END as `memo query -r` takes it, and what is wrong with it
    raises what memo_query.main raises.  One device.  Returns uint64 [kmax, n_docs + 1]."""
    n_docs, kmax = docs(n_docs), _kmax(kmax)
    record, qs, L, _ = region_window(region, kmax)
    feed, buf = region_feed(index_path, record, device)
    return _exact(feed, buf, qs, L, n_docs, kmax, membership, device, slice_positions)


def atleast(exact):
    """atleast[k][t] = #{ p : sel_t[p] >= k } = the sum of exact[k][v] over v >= t, for t = 1 ... N: uint64 [kmax, N]"""
    exact = np.asarray(exact, np.uint64)
    return np.cumsum(exact[:, ::-1], axis=1, dtype=np.uint64)[:, ::-1][:, 1:]


def emit(exact, cumulative=False):
    """the text of `memo spectrum`: a header `k`, 0 ... N (cumulative: 1 ... N), then one line per k, tab-separated"""
    exact = np.asarray(exact, np.uint64)
    n = exact.shape[1] - 1
    body = atleast(exact) if cumulative else exact
    lines = ["\t".join(["k"] + [str(v) for v in range(1 if cumulative else 0, n + 1)])]
    lines += ["\t".join([str(k + 1)] + [str(int(c)) for c in row]) for k, row in enumerate(body)]
    return ("\n".join(lines) + "\n").encode()


__all__ = ["N_MAX", "KMAX_MAX", "tile", "table", "exact", "region_exact", "atleast", "emit"]
