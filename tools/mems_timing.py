#!/usr/bin/env python3
"""What `memo mems` costs, pass by pass, and what it spares (GPU box; profiles/mems_timing.txt).
  python tools/mems_timing.py                          # BASELINE config 3's rows (100 genomes, 10^8 positions, 5e8 rows, int64 columns)
In one process, on the index's own int64 columns (memo_index_columns):
  - memo_mems_dev on the finished cells of memo_maxk_*_dev at T = N and T = N / 2: the device time of the count pass, of the scan with
    the gather of the plane bases, and of the scatter pass from event pairs (memo_debug_mems_times of the A/B library), medians of
    --repeats warm calls after --warm, and the whole call on the host clock; the number of matches found;
  - the yardstick, in the same process, alternating call by call: the route this replaces -- memo_maxk_finish_dev's result downloaded
    (4 L bytes) and the starts found with NumPy on the host; its list is compared with the device's;
  - the floor: the bytes the three passes move (the cells are read twice, 8 bytes written per match, the tile counts and bases) over
    8 TB/s;
  - for comparison, memo_runs_conservation_dev (the same count and scatter kernels on its value key) on a uint16 result of the same length, whole
    call on the host clock, against its own bytes;
  - `-a`: the planes 1 .. N - 1 of one slice of the same rows read as a membership index (config 4), memo_lengths_*_dev's cells."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from memo_amd import _lib, lengths, mems, synth  # noqa: E402
from memo_amd._device import DevBuffer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--positions", type=int, default=100_000_000)
ap.add_argument("--num-docs", type=int, default=100)
ap.add_argument("--cap", type=int, default=2 ** 31 - 1)
ap.add_argument("--warm", type=int, default=5)
ap.add_argument("--repeats", type=int, default=20)
a = ap.parse_args()
M, n, cap = a.positions, a.num_docs, a.cap
_lib.use_ab(True)
lib, check = _lib.lib, _lib.check


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def stats(v):
    return f"median {med(v):.3f} ms, min {min(v):.3f}, max {max(v):.3f}"


def device_call(d_cells, L, pitch, planes, halo, keep=False):
    """(the three device times, the whole call on the host clock in ms, matches, the lists when asked for)"""
    ms = (C.c_float * 3)()
    counts = np.zeros(planes, np.uint64)
    d_s, d_l = C.c_void_p(), C.c_void_p()
    check(lib().memo_debug_mems_times(1, None))
    t = time.perf_counter()
    check(lib().memo_mems_dev(d_cells, L, pitch, planes, cap, 1, 1, halo, C.byref(d_s), C.byref(d_l), counts.ctypes.data, 0, None))
    wall = (time.perf_counter() - t) * 1e3
    check(lib().memo_debug_mems_times(0, ms))
    total, lists = int(counts.sum()), None
    try:
        if keep:
            lists = [np.empty(total, np.uint32) for _ in range(2)]
            for host, d in zip(lists, (d_s, d_l)):
                if total:
                    check(lib().memo_dev_download(0, host.ctypes.data, d, host.nbytes, None))
    finally:
        for d in (d_s, d_l):
            if d:
                lib().memo_dev_free(0, d)
    return list(ms), wall, total, lists


def host_route(d_cells, L, out):
    """the route this replaces: the lengths downloaded, the starts found with NumPy; (ms, starts, lengths)"""
    t = time.perf_counter()
    check(lib().memo_dev_download(0, out.ctypes.data, d_cells, out.nbytes, None))
    start = np.empty(L, bool)
    start[0] = True
    np.less(out[:-1], out[1:], out=start[1:])
    start[1:] |= (out[:-1] == out[1:]) & (out[1:] < cap)
    start &= out >= 1
    at = np.flatnonzero(start)
    vals = out[at]
    return (time.perf_counter() - t) * 1e3, at, vals


def report(name, d_cells, L, pitch, planes, halo, yardstick):
    ntiles = planes * -(-L // mems.tile())
    times, walls, host = [], [], []
    out = np.empty(L, np.uint32) if yardstick else None
    total = 0
    for i in range(a.warm + a.repeats):
        ms, wall, total, lists = device_call(d_cells, L, pitch, planes, halo, keep=(i == 0 and yardstick))
        if yardstick:
            h, at, vals = host_route(d_cells, L, out)
            if i == 0:
                assert np.array_equal(lists[0], at) and np.array_equal(lists[1], vals), "the device's list and the host's differ"
        if i >= a.warm:
            times.append(ms)
            walls.append(wall)
            if yardstick:
                host.append(h)
    t = np.asarray(times)
    whole = t.sum(axis=1)
    moved = 8 * planes * L + 8 * total + 4 * ntiles * 2 + 8 * ntiles * 2
    floor = moved / 8e12 * 1e3
    print(f"-- {name}: {planes} plane(s) of {L} cells, {ntiles} tiles, {total} matches ({total / (planes * L):.4f} per position; the list is "
          f"{8 * total / 1e6:.1f} MB against {4 * planes * L / 1e6:.0f} MB of lengths)", flush=True)
    print(f"   count {stats(t[:, 0])}; scan + plane bases {stats(t[:, 1])}; scatter {stats(t[:, 2])}", flush=True)
    print(f"   the three passes: {stats(whole)} = {med(whole) / floor:.2f} x the 8 TB/s time of the {moved / 1e6:.0f} MB they move ({floor:.3f} ms; "
          f"{moved / med(whole) / 1e9:.2f} TB/s); the whole call on the host clock: {stats(walls)}", flush=True)
    if yardstick:
        print(f"   yardstick, download 4 L bytes + NumPy starts on the host: {stats(host)} = {med(host) / med(walls):.0f} x the call, "
              f"{med(host) / med(whole):.0f} x the passes; same list", flush=True)
    return med(whole), floor


def runs_comparison(ix):
    """memo_runs_conservation_dev on a uint16 result of the same length: value runs, whole call on the host clock"""
    d_vec = C.c_void_p()
    check(lib().memo_dev_malloc(0, 2 * M, C.byref(d_vec)))
    try:
        ix.conservation_dev(0, M, 31, n, d_vec.value)
        ix.check()
        walls, runs = [], 0
        for i in range(a.warm + a.repeats):
            d_s, d_v, r = C.c_void_p(), C.c_void_p(), C.c_uint64(0)
            t = time.perf_counter()
            check(lib().memo_runs_conservation_dev(d_vec, M, 0, 0, 0, C.byref(d_s), C.byref(d_v), C.byref(r), 0, None))
            if i >= a.warm:
                walls.append((time.perf_counter() - t) * 1e3)
            runs = r.value
            for d in (d_s, d_v):
                if d:
                    lib().memo_dev_free(0, d)
        moved = 4 * M + 10 * runs
        print(f"-- for comparison, memo_runs_conservation_dev (value runs) on the uint16 result at k = 31 of the same {M} positions: {runs} runs, "
              f"whole call on the host clock {stats(walls)} = {med(walls) / (moved / 8e12 * 1e3):.2f} x the 8 TB/s time of its {moved / 1e6:.0f} MB", flush=True)
    finally:
        lib().memo_dev_free(0, d_vec)


def main():
    print(f"one session on one MI355X; {lib().memo_version().decode()}", flush=True)
    print(f"== {n} genomes, a window of {M} positions, cap {cap}", flush=True)
    ix, (r0, r1) = synth.device_index(0, M, 257, n, M)
    rows = r1 - r0
    d_cells = C.c_void_p()
    check(lib().memo_dev_malloc(0, 4 * M, C.byref(d_cells)))
    try:
        with ix:
            runs_comparison(ix)
            cols = ix.columns()          # (after the sweep: the index is not finalized any more once its columns are handed out)
            for arg, what in ((n, f"maxk's cells at T = N = {n}"), (n // 2, f"maxk's cells at T = N / 2 = {n // 2}")):
                check(lib().memo_maxk_begin_dev(d_cells, M, cap, 0, None))
                check(lib().memo_maxk_rows_dev(*cols, rows, 0, M, cap, 0, arg, d_cells, 0, None))
                check(lib().memo_maxk_finish_dev(d_cells, M, cap, 0, None))
                report(what, d_cells, M, (M + 3) & ~3, 1, 0, yardstick=True)
            # -a: one slice of the planes of the same rows read as a membership index
            Ls = min(lengths.default_slice_positions(n), M)
            pitch = (Ls + 3) & ~3
            with DevBuffer(0, 4 * n * pitch) as planes:
                check(lib().memo_lengths_begin_dev(planes.d, Ls, pitch, n, cap, 0, None, 0, None))
                check(lib().memo_lengths_rows_dev(*cols, rows, 0, Ls, pitch, n, cap, planes.d, 0, None))
                check(lib().memo_lengths_finish_dev(planes.d, Ls, pitch, n, cap, 0, None))
                report(f"-a: the planes 1 .. {n - 1} of a slice of the membership reading", planes.at(4 * pitch), Ls, pitch, n - 1, 0, yardstick=False)
    finally:
        lib().memo_dev_free(0, d_cells)


main()
