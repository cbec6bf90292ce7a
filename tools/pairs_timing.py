#!/usr/bin/env python3
"""What `memo pairs` costs and what it spares (GPU box; profiles/pairs_timing.txt).
  python tools/pairs_timing.py > profiles/pairs_timing.txt          # planes of 100 genomes x 2e6 positions
In one process:
  1. memo_pairs_dev alone on resident planes (uint32 [N][pitch], the layout memo_lengths_finish_dev leaves: falling ramps between
     random breaks, a mean match of --mean-match positions, every plane its own) in its narrow form (-K --narrow-kmax: 32-bit sums)
     and in its wide form (the default cap: 64-bit sums), the two alternating: the device times of the sweep and of the reduce launch
     from event pairs (memo_debug_pairs_times of the A/B library), the medians of --repeats calls after --warm calls that also ramp
     the clocks, the host clock around the whole blocking call, and beside them the two floors: two vector instructions per pair
     and position over the device's vector issue (256 CUs x 128 lanes a clock at 2.4 GHz), and the cells over 8 TB/s;
  2. the same call on --small-docs genomes: what a launch costs when one workgroup along grid.y holds every unit;
  3. end to end on a synthetic Parquet membership index (memo_amd/synth.py) written to a temporary directory, a window of --positions
     positions and k = --kmin .. --kmax: pairs.region_pairs (the rows read once, one kernel call a slice) against the route of the
     parent commit, matrix.region_matrix -- `memo matrix -k k` in process: the rows read, one membership sweep, memo_cooccurrence_dev
     -- once per k, the matrices summed on the host.  The two matrices are compared for equality.
The matrices of 1 and 2 are compared with NumPy on some pairs."""
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
from memo_amd import _lib, lengths, matrix, pairs, synth  # noqa: E402
from memo_amd._device import DevBuffer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--resident", type=int, default=2_000_000)
ap.add_argument("--num-docs", type=int, default=100)
ap.add_argument("--small-docs", type=int, default=20)
ap.add_argument("--mean-match", type=int, default=100)
ap.add_argument("--narrow-kmax", type=int, default=1000)
ap.add_argument("--positions", type=int, default=1_000_000)
ap.add_argument("--e2e-docs", type=int, default=20)
ap.add_argument("--kmin", type=int, default=1)
ap.add_argument("--kmax", type=int, default=128)
ap.add_argument("--warm", type=int, default=5)
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--turns", type=int, default=2)
ap.add_argument("--no-end-to-end", action="store_true")
a = ap.parse_args()
CAP = 2 ** 31 - 1
LANES_PER_SECOND = 256 * 128 * 2.4e9                                # the device's vector issue: CUs x lanes a clock x clock
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


def host_pair(host, L, g, h, kmin, kmax):
    w = np.maximum(np.minimum(host[[g, h], :L].astype(np.int64), kmax) - (kmin - 1), 0)
    return int(np.minimum(w[0], w[1]).sum())


def pairs_call(d_cells, L, pitch, planes, kmin, kmax, d_sums):
    """(device ms of the sweeps, of the reduce launches, host ms of the blocking call) of one call"""
    ms = (C.c_float * 2)()
    check(lib().memo_debug_pairs_times(1, None))
    _, wall = timed(lambda: check(lib().memo_pairs_dev(d_cells, L, pitch, planes, kmin, kmax, d_sums, 0, None)))
    check(lib().memo_debug_pairs_times(0, ms))
    return ms[0], ms[1], wall * 1e3


def sums_of(d_cells, L, pitch, planes, kmin, kmax, d_sums):
    zero = np.zeros((planes, planes), np.uint64)
    check(lib().memo_dev_upload(0, d_sums.d, zero.ctypes.data, zero.nbytes, None))
    pairs_call(d_cells, L, pitch, planes, kmin, kmax, d_sums.d)
    return d_sums.to_host(zero.shape, np.uint64)


def resident():
    n, L = a.num_docs, a.resident
    pitch = lengths.pitch_of(L)
    print(f"== {n} planes of {L} positions, a mean match of {a.mean_match}: {4 * n * pitch / 1e6:.0f} MB of finished lengths, resident; "
          f"tile {pairs.tile()}, chunk {pairs.chunk()}, narrow up to a span of {pairs.narrow_span()}", flush=True)
    rng = np.random.default_rng(1)
    base = ramps(rng, pitch + 4096 * n, a.mean_match)
    host = np.empty((n, pitch), np.uint32)
    for g in range(n):
        host[g] = base[4096 * g:4096 * g + pitch]                    # (every plane its own cut of one long ramp train)
    forms = (("narrow", 1, a.narrow_kmax), ("wide", 1, CAP))
    with DevBuffer.of(host, 0) as cells, DevBuffer(0, 8 * n * n) as d_sums:
        for planes in (n, min(a.small_docs, n)):
            pair_positions = planes * (planes + 1) // 2 * L
            issue_ms, hbm_ms = 2 * pair_positions / LANES_PER_SECOND * 1e3, 4 * planes * L / 8e12 * 1e3
            print(f"-- {planes} genomes: {pair_positions:.3g} pair-positions; two vector instructions each over the device's vector issue: "
                  f"{issue_ms:.3f} ms; the cells over 8 TB/s: {hbm_ms:.3f} ms", flush=True)
            for name, kmin, kmax in forms:
                got = sums_of(cells.d, L, pitch, planes, kmin, kmax, d_sums)
                for g, h in sorted({(0, 0), (0, planes - 1), (planes // 2, planes - 1), (planes - 1, planes - 1), (1 % planes, planes // 3)}):
                    want = host_pair(host, L, g, h, kmin, kmax)
                    assert got[g, h] == want == got[h, g], f"{name}: pair ({g}, {h}) is {got[g, h]}, NumPy says {want}"
            times = {name: [] for name, _, _ in forms}
            for i in range(a.warm + a.repeats):                      # alternating: the same clocks, the same neighbours
                for name, kmin, kmax in forms:
                    t = pairs_call(cells.d, L, pitch, planes, kmin, kmax, d_sums.d)
                    if i >= a.warm:
                        times[name].append(t)
            for name, kmin, kmax in forms:
                sweep = median([t[0] for t in times[name]])
                print(f"   memo_pairs_dev, {name} (k = {kmin} .. {kmax}): sweep {stats([t[0] for t in times[name]])}; reduce "
                      f"{stats([t[1] for t in times[name]])}; blocking call on the host clock {stats([t[2] for t in times[name]])}", flush=True)
                print(f"     the sweep is {sweep / issue_ms:.1f} x the vector-issue floor and {sweep / hbm_ms:.1f} x the 8 TB/s time; "
                      f"{pair_positions / sweep / 1e6:.0f} G pair-positions a second", flush=True)
        print("   the matrices equal NumPy's on the pairs compared", flush=True)


def end_to_end():
    n, L = a.e2e_docs, a.positions
    tmp = tempfile.mkdtemp(prefix="memo_pairs_timing_")
    try:
        path = os.path.join(tmp, "synth_memb.parquet")
        rows, t = timed(lambda: synth.write_parquet(path, n, L + a.kmax + 1))
        print(f"== end to end: a synthetic index of {n} genomes, {rows} rows, {os.path.getsize(path) / 1e6:.0f} MB of Parquet (written in {t:.1f} s); "
              f"window chr1:0-{L}, k = {a.kmin} .. {a.kmax}", flush=True)
        region = f"chr1:0-{L}"
        for turn in range(a.turns):
            got, t_new = timed(lambda: pairs.region_pairs(path, region, n, kmin=a.kmin, kmax=a.kmax))
            want, t_old = timed(lambda: sum(matrix.region_matrix(path, region, k, n) for k in range(a.kmin, a.kmax + 1)))
            assert np.array_equal(got, want), "region_pairs and the sum of region_matrix over k differ"
            print(f"3. turn {turn + 1}: pairs.region_pairs {t_new * 1e3:.0f} ms; matrix.region_matrix once per k, {a.kmax - a.kmin + 1} calls, "
                  f"{t_old * 1e3:.0f} ms (ratio {t_old / t_new:.1f}); the matrices are equal", flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


print(f"one session on one MI355X; {lib().memo_version().decode()}", flush=True)
resident()
if not a.no_end_to_end:
    end_to_end()
