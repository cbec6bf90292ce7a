#!/usr/bin/env python3
"""What `memo cover` costs and what it spares (GPU box; profiles/cover_timing.txt).
  python tools/cover_timing.py                        # 100 genomes x 10^7 positions in both cell widths, then whole runs of 20 and 100 genomes
In one process:
  - the four entries of memo_amd/csrc/memo_cover.hip on resident planes of --num-docs genomes x --positions positions, in cells of 2
    bytes (-K 64) and of 4 (the default cap): the device time of their launches from event pairs (memo_debug_cover_times of the A/B
    library), warm, and the host clock around the blocking calls.  The lengths are random, a slice of --positions / 10 positions
    written ten times end to end (the kernels' time does not depend on the values), so the weights are timed as ten calls of
    memo_cover_weights_dev; begin has no event pair and is timed on the host clock alone;
  - the score pass of every candidate against the time its bytes take at 8 TB/s: the planes of the list and, once per block of 8
    candidates, the two vectors;
  - the whole region_cover (Parquet rows, lengths, weights, steps; host clock) on a synthetic index of --e2e-positions positions, for
    each of --panels genome counts, at -K 64 and at the default cap, lazy and eager, against the only route there was before:
    lengths.region_planes to the host and a NumPy greedy there that rescores every candidate at every step.  All tables are asserted
    equal."""
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
from memo_amd import _lib, cover, lengths, synth  # noqa: E402
from memo_amd._device import DevBuffer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--positions", type=int, default=10_000_000)
ap.add_argument("--e2e-positions", type=int, default=10_000_000)
ap.add_argument("--num-docs", type=int, default=100)
ap.add_argument("--panels", default="20,100")
ap.add_argument("--warm", type=int, default=3)
ap.add_argument("--repeats", type=int, default=10)
a = ap.parse_args()
assert a.positions % 80 == 0, "--positions must be a multiple of 80: ten slices laid end to end on 16-byte boundaries"
_lib.use_ab(True)
lib, check = _lib.lib, _lib.check
CAP_MAX = 2 ** 31 - 1


def timed(fn):
    t = time.perf_counter()
    r = fn()
    return r, (time.perf_counter() - t) * 1e3


def stats(ms):
    ms = sorted(ms)
    return f"median {ms[len(ms) // 2]:.3f} ms, min {ms[0]:.3f}, max {ms[-1]:.3f} ({len(ms)} calls)"


def median(ms):
    return sorted(ms)[len(ms) // 2]


def device_times(fn, slots):
    """fn() a.warm + a.repeats times under the event pairs: [(device ms summed over `slots`, host ms)] of the repeats"""
    out, ms = [], (C.c_float * 4)()
    for i in range(a.warm + a.repeats):
        check(lib().memo_debug_cover_times(1, None))
        _, wall = timed(fn)
        check(lib().memo_debug_cover_times(0, ms))
        if i >= a.warm:
            out.append((sum(ms[s] for s in slots), wall))
    return out


def entries(n, d_lengths, Ls, pitch_src, copies, kmax):
    L = Ls * copies
    named = list(range(1, n))
    with cover.Weights(L, named, 1, kmax) as w:
        cb = w.cell_bytes
        print(f"-- resident planes of {len(named)} genomes x {L} positions at -K {kmax}: cells of {cb} bytes, {w.plane_bytes * len(named) / 1e6:.0f} MB, "
              f"core and covered {w.plane_bytes / 1e6:.0f} MB each", flush=True)
        ms, wall = [], []
        for i in range(a.warm + a.repeats):
            dev = 0.0
            t = time.perf_counter()
            for c in range(copies):
                check(lib().memo_debug_cover_times(1, None))
                w.pack(d_lengths, Ls, pitch_src, n, c * Ls)
                out = (C.c_float * 4)()
                check(lib().memo_debug_cover_times(0, out))
                dev += out[0]
            if i >= a.warm:
                ms.append(dev)
                wall.append((time.perf_counter() - t) * 1e3)
        moved = (4 + cb) * L * len(named)
        print(f"memo_cover_weights_dev ({copies} call(s) of {Ls} positions): device {stats(ms)}; on the host clock {stats(wall)}; lengths read and weights "
              f"written {moved / 1e6:.0f} MB: {moved / median(ms) / 1e9:.2f} TB/s", flush=True)
        wall = [timed(w.begin)[1] for _ in range(a.warm + a.repeats)][a.warm:]
        print(f"memo_cover_begin_dev: blocking call on the host clock {stats(wall)}; core and covered written {2 * w.plane_bytes / 1e6:.0f} MB", flush=True)
        everyone = list(range(len(named)))
        t = device_times(lambda: w.score(everyone), (1, 2))
        blocks = -(-len(everyone) // 8)
        read = w.plane_bytes * (len(everyone) + 2 * blocks)
        floor = read / 8e12 * 1e3
        print(f"memo_cover_score_dev, {len(everyone)} candidates: device {stats([d for d, _ in t])}; blocking call on the host clock {stats([x for _, x in t])}",
              flush=True)
        print(f"   bytes read {read / 1e6:.0f} MB ({len(everyone)} planes and {blocks} x 2 vectors): {floor:.3f} ms at 8 TB/s; device median over it: "
              f"{median([d for d, _ in t]) / floor:.2f} x = {read / median([d for d, _ in t]) / 1e9:.2f} TB/s", flush=True)
        for few in (1, 8):
            t = device_times(lambda: w.score(everyone[:few]), (1, 2))
            read = w.plane_bytes * (few + 2)
            print(f"memo_cover_score_dev, {few} candidate(s) (a lazy step's batch): device {stats([d for d, _ in t])}; on the host clock {stats([x for _, x in t])}; "
                  f"{read / median([d for d, _ in t]) / 1e9:.2f} TB/s", flush=True)
        t = device_times(lambda: w.take(1), (3,))
        print(f"memo_cover_take_dev: device {stats([d for d, _ in t])}; blocking call on the host clock {stats([x for _, x in t])}; plane and vectors read, vectors "
              f"written {5 * w.plane_bytes / 1e6:.0f} MB: {5 * w.plane_bytes / median([d for d, _ in t]) / 1e9:.2f} TB/s", flush=True)


def host_route(path, region, n, kmax):
    """the only route there was before `memo cover`: the lengths to the host, the greedy in NumPy, every candidate rescored at every step"""
    planes = lengths.region_planes(path, region, n, cap=kmax)
    W = np.minimum(planes, np.uint32(kmax))                       # kmin = 1: the weights are the capped lengths
    L = W.shape[1]
    core, covered = np.full(L, kmax, np.uint32), np.zeros(L, np.uint32)
    remaining, rows = list(range(1, n)), []
    while remaining:
        seen = int(covered.sum(dtype=np.uint64))
        keys = [(int(np.maximum(W[g], covered).sum(dtype=np.uint64)) - seen, int(np.minimum(W[g], core).sum(dtype=np.uint64)), -g) for g in remaining]
        best = remaining.pop(max(range(len(keys)), key=keys.__getitem__))
        core, covered = np.minimum(core, W[best]), np.maximum(covered, W[best])
        rows.append((best, int(core.sum(dtype=np.uint64)), int(covered.sum(dtype=np.uint64))))
    return rows


def whole(path, n, L, kmax):
    region = f"chr1:0-{L}"
    print(f"-- the whole cover: {n} genomes, window {region}, -K {kmax}, objective covered", flush=True)
    results = {}
    for lazy, what in ((True, "lazy"), (False, "eager")):
        wall = []
        for i in range(1 + 2):
            got, t = timed(lambda: cover.region_cover(path, region, n, kmax=kmax, lazy=lazy))
            if i >= 1:
                wall.append(t)
        results[lazy] = list(zip(got[0].tolist(), got[1].tolist(), got[2].tolist()))
        print(f"region_cover, {what}: {stats(wall)} on the host clock (rows, lengths, weights, {len(results[lazy])} steps); planes scored {cover.planes_scored()}",
              flush=True)
        if lazy:
            lazy_ms = median(wall)
    assert results[True] == results[False], "lazy and eager differ"
    rows, t = timed(lambda: host_route(path, region, n, kmax))
    assert rows == results[True], "the two routes differ"
    print(f"lengths.region_planes + a NumPy greedy over {4 * n * L / 1e6:.0f} MB of lengths: {t:.0f} ms on the host clock (1 call), the same table; over lazy "
          f"region_cover: {t / lazy_ms:.1f} x", flush=True)
    print(f"   the order begins {[r[0] for r in rows[:8]]}; covered after 1, 2, 4, 8 genomes {[rows[i][2] for i in (0, 1, 3, 7) if i < len(rows)]} of {L * kmax}",
          flush=True)


print(f"one session on one MI355X; {lib().memo_version().decode()}", flush=True)
n, copies = a.num_docs, 10
Ls = a.positions // copies
pitch_src = lengths.pitch_of(Ls)
rng = np.random.default_rng(20261021)
host = rng.integers(0, 200, (n, pitch_src), dtype=np.uint32)       # match lengths around the caps people pass
host[rng.random((n, pitch_src)) < 0.01] = 100_000                  # ... and a few long ones
print(f"== {n} genomes, random lengths of {Ls} positions laid {copies} times end to end", flush=True)
with DevBuffer.of(host, 0) as d_lengths:
    for kmax in (64, CAP_MAX):
        entries(n, d_lengths.d, Ls, pitch_src, copies, kmax)
del host
tmp = tempfile.mkdtemp(prefix="memo_cover_timing_")
try:
    for n in map(int, a.panels.split(",")):
        path = os.path.join(tmp, f"synth_memb_{n}.parquet")
        rows, t = timed(lambda: synth.write_parquet(path, n, a.e2e_positions + 64))
        print(f"== end to end: a synthetic index of {n} genomes, {rows} rows, {os.path.getsize(path) / 1e6:.0f} MB of Parquet (written in {t / 1e3:.1f} s)", flush=True)
        for kmax in (64, CAP_MAX):
            whole(path, n, a.e2e_positions, kmax)
finally:
    shutil.rmtree(tmp, ignore_errors=True)
