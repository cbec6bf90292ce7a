#!/usr/bin/env python3
"""What `memo spectrum` costs, and what it replaces (GPU box; profiles/spectrum_timing.txt).
  python tools/spectrum_timing.py                # a synthetic membership index: 100 genomes, a window of 10^7 positions, KMAX 128 and 1024
In one process, on the index's own int64 columns (memo_index_columns):
  - the planes once per KMAX (memo_lengths_begin_dev / _rows_dev / _finish_dev at cap = KMAX), then memo_spectrum_add_dev and
    memo_spectrum_finish_dev on them: the device time of each launch from event pairs (memo_debug_spectrum_times of the A/B library),
    medians of --repeats warm calls after --warm; the add against the 4 N L bytes it reads over 8 TB/s; the global atomics one add
    issued, counted in a run of their own (the count costs an atomic beside each);
  - the two routes this replaces, reported and not gated, launch to wait on the host clock, alternating round by round with the whole
    new pass (begin, rows, finish of the planes, the spectrum's begin, add, finish, the download of the table) timed the same way:
      A  N x `memo lengths -t T` (begin, rows, finish, select and the download of 4 L bytes, per T) and a histogram of each on the host;
      B  KMAX x the membership sweep (`memo query -m -k k`, the result downloaded), the one-bit counts and their histogram on the host,
         at KMAX = 128 only;
    --yard-repeats rounds of each, for A after one that is not counted (B takes minutes a round and has none);
  - the tables of the three routes are compared."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch  # (before the library, as tools/ab.py: both then share one HIP runtime) -- only for what the runtime says the device is

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from memo_amd import _lib, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--positions", type=int, default=10_000_000)
ap.add_argument("--num-docs", type=int, default=100)
ap.add_argument("--kmax", type=int, nargs="+", default=[128, 1024])
ap.add_argument("--sweeps-at", type=int, default=128, help="the KMAX at which route B runs")
ap.add_argument("--warm", type=int, default=5)
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--yard-repeats", type=int, default=2)
a = ap.parse_args()
M, n = a.positions, a.num_docs
pitch = (M + 3) & ~3
_lib.use_ab(True)
lib, check = _lib.lib, _lib.check
POP16 = np.array([bin(i).count("1") for i in range(1 << 16)], np.uint8)


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def stats(v):
    return f"median {med(v):.3f} ms, min {min(v):.3f}, max {max(v):.3f}"


def planes_pass(cols, rows, d_cells, kmax):
    check(lib().memo_lengths_begin_dev(d_cells, M, pitch, n, kmax, 0, None, 0, None))
    check(lib().memo_lengths_rows_dev(*cols, rows, 0, M, pitch, n, kmax, d_cells, 0, None))
    check(lib().memo_lengths_finish_dev(d_cells, M, pitch, n, kmax, 0, None))


def spectrum_pass(d_cells, d_scratch, d_exact, kmax, mode=1):
    check(lib().memo_spectrum_begin_dev(d_scratch, n, kmax, 0, None))
    check(lib().memo_spectrum_add_dev(d_cells, M, pitch, n, kmax, mode, d_scratch, 0, None))
    check(lib().memo_spectrum_finish_dev(d_scratch, n, kmax, d_exact, 0, None))
    out = np.empty((kmax, n + 1), np.uint64)
    check(lib().memo_dev_download(0, out.ctypes.data, d_exact, out.nbytes, None))
    return out


def route_a(cols, rows, d_cells, d_out, kmax):
    """N x `memo lengths -t T`, each with its histogram on the host: atleast[k][T] = #{p : sel_T[p] >= k}"""
    least = np.empty((kmax, n), np.int64)
    sel = np.empty(M, np.uint32)
    for t in range(1, n + 1):
        planes_pass(cols, rows, d_cells, kmax)
        check(lib().memo_lengths_select_dev(d_cells, M, pitch, n, kmax, t, d_out, 0, None))
        check(lib().memo_dev_download(0, sel.ctypes.data, d_out, sel.nbytes, None))
        held = np.bincount(sel, minlength=kmax + 1)                     # positions per value of sel_T
        least[:, t - 1] = np.cumsum(held[::-1])[::-1][1:]
    return least


def route_b(ix, kmax):
    """KMAX x `memo query -m -k k`, the one-bit counts and their histogram on the host"""
    out = np.empty((kmax, n + 1), np.int64)
    for k in range(1, kmax + 1):
        bits = ix.membership(0, M, k, n)
        held = POP16[bits.view(np.uint16)].reshape(M, -1).sum(axis=1, dtype=np.int64)
        out[k - 1] = np.bincount(held, minlength=n + 1)
        if k % 32 == 0:
            print(f"      (route B: k = {k})", flush=True)
    return out


def main():
    props = torch.cuda.get_device_properties(0)
    print(f"device 0: {props.name} ({getattr(props, 'gcnArchName', '?')}), {props.multi_processor_count} CUs, {props.total_memory / 2 ** 30:.0f} GiB; {lib().memo_version().decode()}", flush=True)
    print(f"== {n} genomes, a window of {M} positions: a synthetic index (memo_amd/synth.py) read as a membership index", flush=True)
    ix, (r0, r1) = synth.device_index(0, M, max(a.kmax) + 1, n, M)
    rows = r1 - r0
    bufs = [C.c_void_p() for _ in range(4)]
    d_cells, d_out, d_scratch, d_exact = bufs
    for d, size in zip(bufs, (4 * n * pitch, 4 * M, 8 * (n + 1) * (max(a.kmax) + 1), 8 * (n + 1) * max(a.kmax))):
        check(lib().memo_dev_malloc(0, size, C.byref(d)))
    plane_bytes = 4 * n * M
    floor = plane_bytes / 8e12 * 1e3
    try:
        with ix:
            cols = ix.columns()
            ix.finalize(0, False)            # (handing out the columns made the index a draft again; nothing here writes through them)
            print(f"{rows} rows; planes {plane_bytes / 1e9:.2f} GB, {floor:.3f} ms at 8 TB/s", flush=True)
            for kmax in a.kmax:
                planes_pass(cols, rows, d_cells, kmax)
                tile = lib().memo_spectrum_tile(n, kmax, 1)
                ms, path, atomics = (C.c_float * 2)(), C.c_int32(-1), C.c_uint64(0)
                times = []
                check(lib().memo_debug_spectrum_times(1, None, None, None))
                for i in range(a.warm + a.repeats):
                    exact = spectrum_pass(d_cells, d_scratch, d_exact, kmax)
                    check(lib().memo_debug_spectrum_times(1, ms, C.byref(path), None))
                    if i >= a.warm:
                        times.append(list(ms))
                check(lib().memo_debug_spectrum_times(2, None, None, None))                 # the atomics, in a run of their own
                spectrum_pass(d_cells, d_scratch, d_exact, kmax)
                check(lib().memo_debug_spectrum_times(0, None, None, C.byref(atomics)))
                t = np.asarray(times)
                steps = int((exact[1:] != exact[:-1]).any(axis=1).sum())
                print(f"-- KMAX = {kmax} (-m): tiles of {tile} positions, {'the private table in LDS' if path.value else 'wave-merged global atomics'}; "
                      f"exact[k] changes at {steps} of {kmax - 1} k; held by all at k = 1: {int(exact[0][n])}, at k = KMAX: {int(exact[-1][n])}", flush=True)
                print(f"   add: {stats(t[:, 0])} = {med(t[:, 0]) / floor:.2f} x the 8 TB/s time of its 4 N L bytes ({plane_bytes / med(t[:, 0]) / 1e9:.2f} TB/s)", flush=True)
                print(f"   finish: {stats(t[:, 1])}", flush=True)
                print(f"   global atomics of one add: {atomics.value} ({atomics.value / M:.4f} a position)", flush=True)
                # the same planes read as a conservation index: the running-minimum kernel's time (the numbers mean nothing)
                times = []
                check(lib().memo_debug_spectrum_times(1, None, None, None))
                for i in range(a.warm + a.repeats):
                    spectrum_pass(d_cells, d_scratch, d_exact, kmax, mode=0)
                    check(lib().memo_debug_spectrum_times(1, ms, C.byref(path), None))
                    if i >= a.warm:
                        times.append(ms[0])
                check(lib().memo_debug_spectrum_times(0, None, None, None))
                print(f"   add without -m on the same planes ({'private table' if path.value else 'wave-merged atomics'}): {stats(times)} = "
                      f"{med(times) / floor:.2f} x ({plane_bytes / med(times) / 1e9:.2f} TB/s)", flush=True)
                # the routes, alternating, host clock
                new_ms, a_ms, b_ms = [], [], []
                least = sweeps = None
                for i in range(1 + a.yard_repeats):
                    t0 = time.perf_counter()
                    planes_pass(cols, rows, d_cells, kmax)
                    exact = spectrum_pass(d_cells, d_scratch, d_exact, kmax)
                    t1 = time.perf_counter()
                    least = route_a(cols, rows, d_cells, d_out, kmax)
                    t2 = time.perf_counter()
                    if kmax == a.sweeps_at and i >= 1:                                      # (minutes a round: no uncounted one)
                        sweeps = route_b(ix, kmax)
                    t3 = time.perf_counter()
                    print(f"      (round {i}: new {1e3 * (t1 - t0):.1f} ms, A {1e3 * (t2 - t1):.0f} ms, B {1e3 * (t3 - t2):.0f} ms)", flush=True)
                    if i >= 1:
                        new_ms.append((t1 - t0) * 1e3), a_ms.append((t2 - t1) * 1e3), b_ms.append((t3 - t2) * 1e3)
                print(f"   memo spectrum (planes, add, finish, download): {stats(new_ms)}", flush=True)
                print(f"   A  {n} x memo lengths -t T + host histograms: {stats(a_ms)}; ratio {med(a_ms) / med(new_ms):.1f}", flush=True)
                mine = np.cumsum(exact[:, ::-1].astype(np.int64), axis=1)[:, ::-1][:, 1:]
                same = np.array_equal(mine, least)
                if sweeps is not None:
                    print(f"   B  {kmax} x memo query -m -k k + host one-bit counts and histograms: {stats(b_ms)}; ratio {med(b_ms) / med(new_ms):.1f}", flush=True)
                    same = same and np.array_equal(exact.astype(np.int64), sweeps)
                print("   the tables of the routes are equal" if same else "   THE TABLES OF THE ROUTES DIFFER", flush=True)
    finally:
        for d in bufs:
            lib().memo_dev_free(0, d)


main()
