#!/usr/bin/env python3
"""What `memo panel` costs and what it spares (GPU box; profiles/panel_timing.txt).
  python tools/panel_timing.py                        # 100 genomes x 10^7 and 10^8 positions, then whole runs of 20 and 100 genomes
In one process:
  - the three entries of memo_amd/csrc/memo_panel.hip on resident planes of --num-docs genomes x --positions positions and ten times
    as many: the device time of their launches from event pairs (memo_debug_panel_times of the A/B library), warm, and the host clock
    around the blocking calls.  The rows are a synthetic pangenome's membership sweep of --positions positions; the longer planes are
    that slice packed ten times end to end (the bits repeat: the kernels' time does not depend on them), so packing them is timed as
    ten calls of memo_panel_planes_dev;
  - the score pass of every candidate against the time its bytes take at 8 TB/s: the planes of the list and, once per block of 8
    candidates, the two masks;
  - the whole index_panel (sweep, planes, steps; host clock) on a synthetic index of --positions positions, for each of --panels
    genome counts, lazy (as the driver sizes a step's first call, and with first calls of 8 planes) and eager, with the planes each
    scored, against the route there was before: the same sweep, then one memo_collect_dev call per step over the orders prefix + g
    of every remaining candidate g and the same choice on the host.  All tables are asserted equal."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from memo_amd import _lib, collect, panel, synth  # noqa: E402
from memo_amd._device import DevBuffer  # noqa: E402
from memo_amd.index import words  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--positions", type=int, default=10_000_000)
ap.add_argument("--pivot", type=int, default=100_000_000)
ap.add_argument("--num-docs", type=int, default=100)
ap.add_argument("--panels", default="20,100")
ap.add_argument("--warm", type=int, default=3)
ap.add_argument("--repeats", type=int, default=10)
a = ap.parse_args()
assert a.positions % 128 == 0, "--positions must be a multiple of 128: the slices are laid end to end on 16-byte boundaries"
k = 31
_lib.use_ab(True)
lib, check = _lib.lib, _lib.check


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
        check(lib().memo_debug_panel_times(1, None))
        _, wall = timed(fn)
        check(lib().memo_debug_panel_times(0, ms))
        if i >= a.warm:
            out.append((sum(ms[s] for s in slots), wall))
    return out


def entries(n, d_rows, Ls, copies):
    L = Ls * copies
    with panel.Planes(L, n) as planes:
        print(f"-- resident planes of {n} genomes x {L} positions: {4 * planes.words * n / 1e6:.0f} MB, the masks {4 * planes.words / 1e6:.2f} MB each", flush=True)
        ms, wall = [], []
        for i in range(a.warm + a.repeats):
            dev = 0.0
            t = time.perf_counter()
            for c in range(copies):
                check(lib().memo_debug_panel_times(1, None))
                planes.pack(d_rows, Ls, c * Ls)
                out = (C.c_float * 4)()
                check(lib().memo_debug_panel_times(0, out))
                dev += out[0]
            if i >= a.warm:
                ms.append(dev)
                wall.append((time.perf_counter() - t) * 1e3)
        moved = 4 * words(n) * L + 4 * (L // 32) * n
        print(f"memo_panel_planes_dev ({copies} call(s) of {Ls} positions): device {stats(ms)}; on the host clock {stats(wall)}; rows read and planes "
              f"written {moved / 1e6:.0f} MB: {moved / median(ms) / 1e9:.2f} TB/s", flush=True)
        planes.begin()
        everyone = list(range(1, n))
        t = device_times(lambda: planes.score(everyone), (1, 2))
        blocks = -(-len(everyone) // 8)
        read = 4 * planes.words * (len(everyone) + 2 * blocks)
        floor = read / 8e12 * 1e3
        print(f"memo_panel_score_dev, {len(everyone)} candidates: device {stats([d for d, _ in t])}; blocking call on the host clock {stats([w for _, w in t])}",
              flush=True)
        print(f"   bytes read {read / 1e6:.0f} MB ({len(everyone)} planes and {blocks} x 2 masks): {floor:.3f} ms at 8 TB/s; device median over it: "
              f"{median([d for d, _ in t]) / floor:.2f} x = {read / median([d for d, _ in t]) / 1e9:.2f} TB/s", flush=True)
        for few in (1, 8):
            t = device_times(lambda: planes.score(everyone[:few]), (1, 2))
            print(f"memo_panel_score_dev, {few} candidate(s) (a lazy step's batch): device {stats([d for d, _ in t])}; on the host clock {stats([w for _, w in t])}",
                  flush=True)
        t = device_times(lambda: planes.take(1), (3,))
        print(f"memo_panel_take_dev: device {stats([d for d, _ in t])}; blocking call on the host clock {stats([w for _, w in t])}; plane and masks read, masks "
              f"written {5 * 4 * planes.words / 1e6:.2f} MB", flush=True)


def collect_route(ix, n, L, d_bits):
    """the route before `memo panel`: one memo_collect_dev call per step over the orders prefix + g; returns (rows, order-steps walked)"""
    ix.membership_dev(0, L, k, n, d_bits.value)
    ix.check()
    prefix, remaining, rows, walked = [], list(range(1, n)), [], 0
    seen = 0
    while remaining:
        order_rows = np.array([prefix + [g] for g in remaining], np.uint16)
        core, covered = collect.curves((d_bits.value, L), n, order_rows)
        walked += order_rows.size
        best = max(range(len(remaining)), key=lambda i: (int(covered[i, -1]) - seen, int(core[i, -1]), -remaining[i]))
        rows.append((remaining[best], int(core[best, -1]), int(covered[best, -1])))
        seen = int(covered[best, -1])
        prefix.append(remaining.pop(best))
    return rows, walked


def whole(n, L):
    print(f"-- the whole panel: {n} genomes, {L} positions of a {a.pivot}-position synthetic pivot, k = {k}, objective covered", flush=True)
    ix, _ = synth.device_index(0, L, k, n, a.pivot, pack="keep")
    with ix, DevBuffer(0, 4 * words(n) * L) as d_bits:
        results = {}
        lazy_bytes = panel.LAZY_BYTES
        for lazy, what in ((True, "lazy"), (8, "lazy, a step's first call 8 planes"), (False, "eager")):
            panel.LAZY_BYTES = 0 if lazy == 8 else lazy_bytes
            wall = []
            for i in range(1 + 3):
                got, t = timed(lambda: panel.index_panel(ix, 0, L, k, n, lazy=bool(lazy)))
                if i >= 1:
                    wall.append(t)
            results[lazy] = list(zip(got[0].tolist(), got[1].tolist(), got[2].tolist()))
            print(f"index_panel, {what}: {stats(wall)} on the host clock (sweep, planes, {len(results[lazy])} steps); planes scored "
                  f"{panel.planes_scored()}", flush=True)
            if lazy is True:
                lazy_ms = median(wall)
        panel.LAZY_BYTES = lazy_bytes
        assert results[True] == results[False] == results[8], "lazy and eager differ"
        wall = []
        for i in range(1 + 2):
            (rows, walked), t = timed(lambda: collect_route(ix, n, L, d_bits.d))
            if i >= 1:
                wall.append(t)
        assert rows == results[True], "the two routes differ"
        print(f"one memo_collect_dev call per step over prefix + g orders: {stats(wall)} on the host clock (sweep, {walked} order-steps walked), the same "
              f"table; over lazy index_panel: {median(wall) / lazy_ms:.1f} x", flush=True)
        print(f"   the order begins {[r[0] for r in rows[:8]]}; covered after 1, 2, 4, 8 genomes {[rows[i][2] for i in (0, 1, 3, 7) if i < len(rows)]} of {L}",
              flush=True)


print(f"one session on one MI355X; {lib().memo_version().decode()}", flush=True)
n = a.num_docs
print(f"== {n} genomes (W = {words(n)}), rows of {a.positions} positions of a {a.pivot}-position synthetic pivot, k = {k}", flush=True)
ix, _ = synth.device_index(0, a.positions, k, n, a.pivot, pack="keep")
with ix, DevBuffer(0, 4 * words(n) * a.positions) as d_rows:
    ix.membership_dev(0, a.positions, k, n, d_rows.d.value)
    ix.check()
    for copies in (1, 10):
        entries(n, d_rows.d, a.positions, copies)
for n in map(int, a.panels.split(",")):
    whole(n, a.positions)
