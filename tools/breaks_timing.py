#!/usr/bin/env python3
"""What `memo breaks` costs and what it spares (GPU box; profiles/breaks_timing.txt).
  python tools/breaks_timing.py                       # planes of 100 genomes x 5.4e6 positions
In one process:
  1. memo_breaks_dev alone on resident planes (uint32 [N][pitch], the layout memo_lengths_finish_dev leaves: falling ramps between
     random breaks, a mean match of --mean-match positions, every plane its own) with 500 bins: the device time of its kernel from an
     event pair (memo_debug_breaks_times of the A/B library), the median of --repeats calls after --warm calls that also ramp the
     clocks, the host clock around the whole blocking call (with the upload of the edges), and the bytes read over the kernel time;
  2. memo_mems_dev (the starts key) on the same cells, alternating with 1 (memo_debug_mems_times: count + scan + scatter): what the
     parent commit does to those cells before the host can histogram anything -- it reads them in the count and in the scatter and
     writes every match;
  3. memo_breaks_dev with 2^20 bins of 16 cells on 2^24 cells a plane (the same buffer, cut into fewer and longer planes): the
     narrow-bin walk, every lane with its own atomics;
  4. end to end on a synthetic Parquet membership index (memo_amd/synth.py) written to a temporary directory, a window of --positions
     positions: breaks.region_breaks against mems.region_mems(all_genomes=True) + np.histogram per genome, and against
     lengths.region_planes + np.add.reduceat.  The tables are compared.
The tables of 1 and 3 are compared with NumPy on some planes."""
import argparse
import ctypes as C
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from memo_amd import _lib, breaks, lengths, mems, synth, view  # noqa: E402
from memo_amd._device import DevBuffer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--resident", type=int, default=5_400_000)
ap.add_argument("--num-docs", type=int, default=100)
ap.add_argument("--mean-match", type=int, default=100)
ap.add_argument("--bins", type=int, default=500)
ap.add_argument("--positions", type=int, default=10_000_000)
ap.add_argument("--e2e-docs", type=int, default=20)
ap.add_argument("--warm", type=int, default=5)
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--no-end-to-end", action="store_true")
a = ap.parse_args()
CAP = 2 ** 31 - 1
_lib.use_ab(True)
lib, check = _lib.lib, _lib.check


def timed(fn):
    t = time.perf_counter()
    r = fn()
    return r, time.perf_counter() - t


def stats(ms):
    ms = sorted(ms)
    return f"median {ms[len(ms) // 2]:.3f} ms, min {ms[0]:.3f}, max {ms[-1]:.3f} ({len(ms)} calls)"


def median(ms):
    return sorted(ms)[len(ms) // 2]


def ramps(rng, L, mean):
    """match lengths as an index leaves them: from every break a length that falls by one a position until the next break"""
    at = np.flatnonzero(rng.random(L) < 1.0 / mean)
    at = np.concatenate([[0], at[at > 0], [L]])
    reach = at[1:] + rng.integers(0, mean, len(at) - 1)             # where the match that starts at a break ends
    return (np.repeat(reach, np.diff(at)) - np.arange(L)).astype(np.uint32)


def host_table(v, edges, halo):
    """NumPy on one plane: the starts and the sums of every bin (min_len = 1, no value at the cap)"""
    w = v.astype(np.int64)
    start = np.zeros(len(w), np.int64)
    start[0] = 0 if halo else int(w[0] >= 1)
    start[1:] = (w[1:] >= 1) & (w[:-1] <= w[1:])
    cut = np.asarray(edges, np.int64)[:-1]
    return np.stack([np.add.reduceat(x[halo:], cut) for x in (start, w)]).astype(np.uint64)       # (no bin is empty)


def breaks_call(d_cells, L, pitch, planes, edges, d_table, halo=1):
    """(device ms of the kernel, host ms of the blocking call) of one call"""
    ms = (C.c_float * 1)()
    check(lib().memo_debug_breaks_times(1, None))
    _, wall = timed(lambda: check(lib().memo_breaks_dev(d_cells, L, pitch, planes, CAP, 1, halo, 0, edges.ctypes.data, len(edges) - 1, d_table, 0, None)))
    check(lib().memo_debug_breaks_times(0, ms))
    return ms[0], wall * 1e3


def mems_call(d_cells, L, pitch, planes):
    """(device ms of the three passes, host ms of the blocking call, matches) of one call; the lists are freed, not downloaded"""
    ms = (C.c_float * 3)()
    d_starts, d_lengths = C.c_void_p(), C.c_void_p()
    counts = np.zeros(planes, np.uint64)
    check(lib().memo_debug_mems_times(1, None))
    _, wall = timed(lambda: check(lib().memo_mems_dev(d_cells, L, pitch, planes, CAP, 1, 1, 1, C.byref(d_starts), C.byref(d_lengths),
                                                      counts.ctypes.data, 0, None)))
    check(lib().memo_debug_mems_times(0, ms))
    with DevBuffer.adopt(d_starts, 0), DevBuffer.adopt(d_lengths, 0):
        return list(ms), wall * 1e3, int(counts.sum())


def table_of(d_cells, L, pitch, planes, edges, table, halo=1):
    zero = np.zeros((2, planes, len(edges) - 1), np.uint64)
    check(lib().memo_dev_upload(0, table.d, zero.ctypes.data, zero.nbytes, None))
    breaks_call(d_cells, L, pitch, planes, edges, table.d, halo)
    return table.to_host(zero.shape, np.uint64)


def resident():
    n, L = a.num_docs, a.resident + 1                                # one neighbour cell and a.resident counted cells a plane
    pitch = lengths.pitch_of(L)
    nbytes = 4 * n * pitch
    print(f"== {n} planes of {L} cells (a neighbour cell and {a.resident} positions), a mean match of {a.mean_match}: {nbytes / 1e6:.0f} MB "
          "of finished lengths, resident", flush=True)
    rng = np.random.default_rng(1)
    base = ramps(rng, pitch + 4096 * n, a.mean_match)
    host = np.empty((n, pitch), np.uint32)
    for g in range(n):
        host[g] = base[4096 * g:4096 * g + pitch]                    # (every plane its own cut of one long ramp train)
    long_L = 1 << 24
    long_planes = min(host.size // long_L, n)
    with DevBuffer.of(host, 0) as cells, DevBuffer(0, 16 * max(n * a.bins, long_planes << 20)) as table:
        floor_ms = 4 * n * L / 8e12 * 1e3
        print(f"the cells over 8 TB/s: {floor_ms:.3f} ms", flush=True)
        wide = view.bin_edges(a.resident, a.bins)
        got = table_of(cells.d, L, pitch, n, wide, table)
        for g in sorted({0, n // 2, n - 1}):
            assert np.array_equal(got[:, g], host_table(host[g, :L], wide, 1)), f"plane {g} of the table of {a.bins} bins differs from NumPy's"
        t_breaks, t_mems = [], []
        for i in range(a.warm + a.repeats):                          # alternating: the same clocks, the same neighbours
            t, m = breaks_call(cells.d, L, pitch, n, wide, table.d), mems_call(cells.d, L, pitch, n)
            if i >= a.warm:
                t_breaks.append(t)
                t_mems.append(m)
        dev = median([d for d, _ in t_breaks])
        print(f"1. memo_breaks_dev, {a.bins} bins: kernel {stats([d for d, _ in t_breaks])}; blocking call on the host clock "
              f"{stats([w for _, w in t_breaks])}", flush=True)
        print(f"   {4 * n * L / 1e6:.0f} MB read over the kernel's median: {4 * n * L / dev / 1e9:.2f} TB/s, {dev / floor_ms:.1f} x the 8 TB/s time", flush=True)
        whole = median([sum(m) for m, _, _ in t_mems])
        print(f"2. memo_mems_dev (starts) on the same cells, alternating with 1: count + scan + scatter {stats([sum(m) for m, _, _ in t_mems])} "
              f"(count {median([m[0] for m, _, _ in t_mems]):.3f}, scan {median([m[1] for m, _, _ in t_mems]):.3f}, scatter "
              f"{median([m[2] for m, _, _ in t_mems]):.3f}); blocking call {stats([w for _, w, _ in t_mems])}; {t_mems[0][2]} matches, "
              f"{8 * t_mems[0][2] / 1e6:.0f} MB of lists that the host would still have to download and histogram", flush=True)
        print(f"   breaks over mems: {dev / whole:.2f} x", flush=True)
        assert t_mems[0][2] == int(got[0].sum()), "memo_mems_dev reports another number of starts"
        narrow = np.arange(0, long_L + 1, 16, dtype=np.int64)
        flat = host.reshape(-1)
        got = table_of(cells.d, long_L, long_L, long_planes, narrow, table, halo=0)
        for g in sorted({0, long_planes - 1}):
            assert np.array_equal(got[:, g], host_table(flat[g * long_L:(g + 1) * long_L], narrow, 0)), f"plane {g} of the table of 2^20 bins differs"
        t_narrow = [breaks_call(cells.d, long_L, long_L, long_planes, narrow, table.d, halo=0) for _ in range(a.warm + a.repeats)][a.warm:]
        nar = median([d for d, _ in t_narrow])
        nb = 4 * long_planes * long_L
        print(f"3. memo_breaks_dev, 2^20 bins of 16 cells, {long_planes} planes of 2^24 cells ({nb / 1e6:.0f} MB): kernel {stats([d for d, _ in t_narrow])}; "
              f"blocking call {stats([w for _, w in t_narrow])} (8 MiB of edges uploaded per call)", flush=True)
        print(f"   {nb / nar / 1e9:.3f} TB/s, {nar / (nb / 8e12 * 1e3):.1f} x the 8 TB/s time; cells of the table that are not zero, one atomic "
              f"or more each: {int((got != 0).sum())} of {got.size}", flush=True)
        print("   the tables equal NumPy's on the planes compared", flush=True)


def end_to_end():
    n, L, k = a.e2e_docs, a.positions, 31
    tmp = tempfile.mkdtemp(prefix="memo_breaks_timing_")
    try:
        path = os.path.join(tmp, "synth_memb.parquet")
        rows, t = timed(lambda: synth.write_parquet(path, n, L + k + 1))
        print(f"== end to end: a synthetic index of {n} genomes, {rows} rows, {os.path.getsize(path) / 1e6:.0f} MB of Parquet (written in {t:.1f} s); "
              f"window chr1:0-{L}, {a.bins} bins", flush=True)
        region = f"chr1:0-{L}"
        for turn in ("first", "second"):
            (table, edges, qs), t_new = timed(lambda: breaks.region_breaks(path, region, n, a.bins, membership=True))

            def by_mems():
                m = mems.region_mems(path, region, n, membership=True, all_genomes=True)
                return np.stack([np.histogram(m.starts[m.genome == g], edges)[0] for g in range(1, n)]), len(m.starts)
            (starts, matches), t_mems = timed(by_mems)
            sums, t_planes = timed(lambda: np.add.reduceat(lengths.region_planes(path, region, n).astype(np.uint64), edges[:-1], axis=1))
            assert np.array_equal(table[0, 1:].astype(np.int64), starts), "region_breaks and the histogram of region_mems differ"
            assert np.array_equal(table[1], sums), "region_breaks and the reduced region_planes differ"
            print(f"4. {turn} turn: breaks.region_breaks {t_new * 1e3:.0f} ms; mems.region_mems(all_genomes) + np.histogram of {matches} matches "
                  f"{t_mems * 1e3:.0f} ms (ratio {t_mems / t_new:.1f}); lengths.region_planes + np.add.reduceat of {4 * n * L / 1e6:.0f} MB "
                  f"{t_planes * 1e3:.0f} ms (ratio {t_planes / t_new:.1f}); the tables are equal", flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


print(f"one session on one MI355X; {lib().memo_version().decode()}", flush=True)
resident()
if not a.no_end_to_end:
    end_to_end()
