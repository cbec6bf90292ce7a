#!/usr/bin/env python3
"""What `memo mosaic` costs, lap by lap, and the two choices its parse leaves to a measurement (GPU box; profiles/mosaic_timing.txt).
  python tools/mosaic_timing.py > profiles/mosaic_timing.txt
In one process, device times from event pairs (memo_debug_mosaic_times of the A/B library), medians of --repeats calls after --warm:
  1. memo_mosaic_fold_dev alone on resident planes (uint32 [N][pitch], the layout memo_lengths_finish_dev leaves: falling ramps
     between random breaks, a mean match of --mean-match positions, every plane its own -- tools/nearest_timing.py's buffer),
     alternating with memo_nearest_dev with only the winner asked for on the same buffer, beside the 8 TB/s time of the bytes; step
     and winner are compared with NumPy on the first --check positions;
  2. memo_mosaic_parse_dev on --parse positions (10^7 and 10^8), per lap (exits, walk, mark, lines), for three inputs -- the ramps
     (mean 100), geometric steps of mean 8, all steps 1 -- at every tile T of 4096, 8192, 16384, 32768 and with both marks (the
     serial lane, the doubling rounds; memo_debug_mosaic_shape); the walk lap beside tiles x one HBM miss (900 cycles at 2.4 GHz);
     the lines are compared across the shapes, and with a host walk on the first --check positions;
  3. end to end on a synthetic Parquet membership index (memo_amd/synth.py) written to a temporary directory, a window of
     --positions positions: mosaic.region_mosaic against the only host route there is -- lengths.region_planes, a NumPy max / argmax,
     a Python walk of the steps.  The lines are compared."""
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
from memo_amd import _lib, lengths, mosaic, synth  # noqa: E402
from memo_amd._device import DevBuffer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--resident", type=int, default=5_400_000)
ap.add_argument("--num-docs", type=int, default=100)
ap.add_argument("--mean-match", type=int, default=100)
ap.add_argument("--check", type=int, default=300_000)
ap.add_argument("--parse", type=int, nargs="*", default=[10_000_000, 100_000_000])
ap.add_argument("--positions", type=int, default=10_000_000)
ap.add_argument("--e2e-docs", type=int, default=20)
ap.add_argument("--warm", type=int, default=5)
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--no-fold", action="store_true")
ap.add_argument("--no-end-to-end", action="store_true")
a = ap.parse_args()
CAP = 2 ** 31 - 1
MISS_MS = 900 / 2.4e9 * 1e3                                      # one dependent HBM miss, idle chip
TILES = (4096, 8192, 16384, 32768)
MARKS = {1: "serial", 2: "doubling"}
_lib.use_ab(True)
lib, check = _lib.lib, _lib.check


def timed(fn):
    t = time.perf_counter()
    r = fn()
    return r, time.perf_counter() - t


def median(ms):
    return sorted(ms)[len(ms) // 2]


def spread(ms):
    ms = sorted(ms)
    return f"median {ms[len(ms) // 2]:.3f} ms, min {ms[0]:.3f}, max {ms[-1]:.3f} ({len(ms)} calls)"


def ramps(rng, L, mean):
    """match lengths as an index leaves them: from every break a length that falls by one a position until the next break"""
    at = np.flatnonzero(rng.random(L) < 1.0 / mean)
    at = np.concatenate([[0], at[at > 0], [L]])
    reach = at[1:] + rng.integers(0, mean, len(at) - 1)
    return (np.repeat(reach, np.diff(at)) - np.arange(L)).astype(np.uint32)


def host_walk(step, winner, upto):
    """the lines that start before `upto`, one phrase at a time"""
    starts, genomes, p, previous = [], [], 0, None
    while p < upto:
        g = int(winner[p])
        if not (g == 0 and previous == 0):
            starts.append(p), genomes.append(g)
        previous = g
        p += max(int(step[p]), 1)
    return np.asarray(starts, np.int64), np.asarray(genomes, np.uint16)


def laps():
    ms = (C.c_float * 5)()
    check(lib().memo_debug_mosaic_times(0, ms))
    return list(ms)


def fold():
    n, L = a.num_docs, a.resident
    pitch = lengths.pitch_of(L)
    read = 4 * (n - 1) * L
    print(f"== {n} planes of {L} positions, a mean match of {a.mean_match}: {4 * n * pitch / 1e6:.0f} MB of finished lengths, resident; the fold reads the "
          f"{n - 1} candidate planes, {read / 1e6:.0f} MB, and writes {6 * L / 1e6:.0f} MB", flush=True)
    rng = np.random.default_rng(1)
    base = ramps(rng, pitch + 4096 * n, a.mean_match)
    host = np.empty((n, pitch), np.uint32)
    for g in range(n):
        host[g] = base[4096 * g:4096 * g + pitch]
    m = min(a.check, L)
    floor_ms = read / 8e12 * 1e3
    with DevBuffer.of(host, 0) as cells, DevBuffer(0, 4 * pitch) as d_step, DevBuffer(0, 2 * pitch) as d_winner:
        def fold_call():
            check(lib().memo_debug_mosaic_times(1, None))
            check(lib().memo_mosaic_fold_dev(cells.d, L, pitch, n, CAP, 1, None, d_step.d, d_winner.d, 0, None))
            return laps()[0]

        def nearest_call():
            ms = (C.c_float * 1)()
            check(lib().memo_debug_nearest_times(1, None))
            check(lib().memo_nearest_dev(cells.d, L, pitch, n, CAP, 1, None, 0, None, 0, None, None, d_winner.d, 0, None))
            check(lib().memo_debug_nearest_times(0, ms))
            return ms[0]
        fold_call()
        c = host[1:, :m].astype(np.int64)
        best = c.max(axis=0)
        assert np.array_equal(d_step.to_host(m, np.uint32), np.where(best >= 1, best, 1).astype(np.uint32)), "the fold's step differs from NumPy's"
        assert np.array_equal(d_winner.to_host(m, np.uint16), np.where(best >= 1, c.argmax(axis=0) + 1, 0).astype(np.uint16)), "the fold's winner differs"
        print(f"   step and winner equal NumPy's on the first {m} positions", flush=True)
        t = {"fold": [], "nearest": []}
        for i in range(a.warm + a.repeats):                          # alternating: the same clocks, the same neighbours
            got = {"fold": fold_call(), "nearest": nearest_call()}
            if i >= a.warm:
                for k in t:
                    t[k].append(got[k])
        f, w = median(t["fold"]), median(t["nearest"])
        print(f"1. memo_mosaic_fold_dev: kernel {spread(t['fold'])}; {read / f / 1e9:.2f} TB/s of the cells read, {f / floor_ms:.1f} x their 8 TB/s time of {floor_ms:.3f} ms",
              flush=True)
        print(f"   alternating with it on the same buffer, memo_nearest_dev with only the winner asked for: kernel {spread(t['nearest'])}; "
              f"fold over nearest: {f / w:.2f} x", flush=True)
        # the parse of what the fold left: the lines of the resident window
        check(lib().memo_debug_mosaic_times(1, None))
        lines = mosaic._parse(d_step.d, d_winner.d, L, 0)
        ms = laps()
        print(f"   the parse of these {L} positions: {len(lines[0])} lines; exits {ms[1]:.3f} ms, walk {ms[2]:.3f}, mark {ms[3]:.3f}, lines {ms[4]:.3f}", flush=True)


def parse(L):
    rng = np.random.default_rng(2)
    winner = rng.integers(1, 100, L).astype(np.uint16)
    inputs = (("ramps, mean 100", ramps(rng, L, 100)), ("geometric, mean 8", np.maximum(rng.geometric(1.0 / 8, L), 1).astype(np.uint32)),
              ("all steps 1", np.ones(L, np.uint32)))
    print(f"== the parse alone on {L} positions (step 4 bytes and winner 2 bytes a position, resident); kernel medians of {a.repeats} calls after {a.warm}, ms", flush=True)
    with DevBuffer(0, 4 * L) as d_step, DevBuffer.of(winner, 0) as d_winner:
        for name, step in inputs:
            check(lib().memo_dev_upload(0, d_step.d, step.ctypes.data, step.nbytes, None))
            m = min(a.check, L)
            want, first = host_walk(step, winner, m), None
            print(f"2. {name}", flush=True)
            for T in TILES:
                for mark in MARKS:
                    check(lib().memo_debug_mosaic_shape(T, mark))
                    t = []
                    for i in range(a.warm + a.repeats):
                        check(lib().memo_debug_mosaic_times(1, None))
                        (lines, wall) = timed(lambda: mosaic._parse(d_step.d, d_winner.d, L, 0))
                        if i >= a.warm:
                            t.append(laps()[1:] + [wall * 1e3])
                    k = int(np.searchsorted(lines[0], m))
                    assert np.array_equal(lines[0][:k], want[0]) and np.array_equal(lines[1][:k], want[1]), f"T {T}, {MARKS[mark]}: the lines differ from the host walk"
                    if first is None:
                        first = lines
                    assert np.array_equal(lines[0], first[0]) and np.array_equal(lines[1], first[1]), f"T {T}, {MARKS[mark]}: the lines differ from the first shape's"
                    ex, wk, mk, ln, wall = (median([x[j] for x in t]) for j in range(5))
                    tiles = -(-L // T)
                    print(f"   T {T:5d}, {MARKS[mark]:8s} mark: exits {ex:7.3f}  walk {wk:7.3f} ({tiles} tiles x one miss = {tiles * MISS_MS:.3f})  mark {mk:7.3f}  "
                          f"lines {ln:7.3f}  sum {ex + wk + mk + ln:7.3f}; the blocking call with its two downloads {wall:8.3f}; {len(lines[0])} lines", flush=True)
            check(lib().memo_debug_mosaic_shape(0, 0))
            print(f"   the lines are the same at every shape, and the host walk's on the first {m} positions", flush=True)


def end_to_end():
    n, L, k = a.e2e_docs, a.positions, 31
    tmp = tempfile.mkdtemp(prefix="memo_mosaic_timing_")
    try:
        path = os.path.join(tmp, "synth_memb.parquet")
        rows, t = timed(lambda: synth.write_parquet(path, n, L + k + 1))
        print(f"== end to end: a synthetic index of {n} genomes, {rows} rows, {os.path.getsize(path) / 1e6:.0f} MB of Parquet (written in {t:.1f} s); window chr1:0-{L}",
              flush=True)
        region = f"chr1:0-{L}"
        for turn in ("first", "second"):
            (starts, genomes, _, _), t_new = timed(lambda: mosaic.region_mosaic(path, region, n))

            def by_planes():
                planes = lengths.region_planes(path, region, n)
                best, winner = np.zeros(L, np.uint32), np.zeros(L, np.uint16)
                for lo in range(0, L, 1 << 20):                      # a slice at a time: the argmax of the whole window would not fit a cache
                    c = planes[1:, lo:lo + (1 << 20)]
                    best[lo:lo + (1 << 20)], winner[lo:lo + (1 << 20)] = c.max(axis=0), c.argmax(axis=0) + 1
                winner[best < 1] = 0
                return host_walk(np.maximum(best, 1), winner, L)
            (h_starts, h_genomes), t_host = timed(by_planes)
            assert np.array_equal(starts, h_starts) and np.array_equal(genomes, h_genomes), "region_mosaic and the host route differ"
            print(f"3. {turn} turn: mosaic.region_mosaic {t_new * 1e3:.0f} ms ({len(starts)} lines); lengths.region_planes + NumPy argmax of {4 * n * L / 1e6:.0f} MB "
                  f"+ a Python walk {t_host * 1e3:.0f} ms (ratio {t_host / t_new:.1f}); the lines are equal", flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


print(f"one session on one MI355X; {lib().memo_version().decode()}; the product's tile {mosaic.tile()}", flush=True)
if not a.no_fold:
    fold()
for L in a.parse:
    parse(L)
if not a.no_end_to_end:
    end_to_end()
