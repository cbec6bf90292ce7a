#!/usr/bin/env python3
"""What `memo collect` costs and what it spares (GPU box; profiles/collect_timing.txt).
  python tools/collect_timing.py                      # 10^7 positions of the 100-genome pangenome (W = 4) and of a 500-genome
                                                      # one (W = 16), the index order alone (P = 1) and 100 random orders
Per pangenome, in one process:
  - the membership sweep that produces the input, launch to wait (host clock around work that ends in a device wait), and the
    input's bytes over 8 TB/s: yardsticks only;
  - memo_collect_dev on that result, per number of orders: the device time of its launches from event pairs
    (memo_debug_collect_times of the A/B library: the sweep launches, the reduce launches), warm, after --warm calls that also
    ramp the clocks, and the host clock around the whole blocking call (with its scratch allocation and the upload of the orders);
    the lane-steps P x M x L / 32 it takes and what one costs;
  - the host route it replaces: the download of the same buffer into pageable host memory (the box's measured device-to-host
    rate) and np.logical_and.accumulate / np.logical_or.accumulate over the unpacked bits, one order per task on the threads the
    box grants, timed on --host-positions positions and --host-orders orders and scaled to the window and the orders, which is
    said in the line.
The curves of the device are compared with the host's on the timed positions."""
import argparse
import ctypes as C
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from memo_amd import _lib, collect, synth  # noqa: E402
from memo_amd._device import DevBuffer  # noqa: E402
from memo_amd.index import words  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--positions", type=int, default=10_000_000)
ap.add_argument("--pivot", type=int, default=100_000_000)
ap.add_argument("--num-docs", default="100,500")
ap.add_argument("--orders", default="1,100")
ap.add_argument("--warm", type=int, default=5)
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--host-positions", type=int, default=1_000_000)
ap.add_argument("--host-orders", type=int, default=16)
a = ap.parse_args()
Lw, k = a.positions, 31
THREADS = int(os.environ.get("OMP_NUM_THREADS", "16") or "16")
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


def collect_times(d_bits, L, n, rows, d_core, d_covered):
    """(device ms of the sweeps, of the reduce launches, host ms of the blocking call) per call"""
    out, ms = [], (C.c_float * 2)()
    for i in range(a.warm + a.repeats):
        check(lib().memo_debug_collect_times(1, None))
        _, wall = timed(lambda: collect._accumulate(d_bits, L, n, rows, d_core, d_covered, 0))
        check(lib().memo_debug_collect_times(0, ms))
        if i >= a.warm:
            out.append((ms[0], ms[1], wall * 1e3))
    return out


def host_curves(B, rows):
    """the host route on unpacked bits B bool [L, N]: one order per task"""
    def one(order):
        cols = B[:, order]
        return np.logical_and.accumulate(cols, axis=1).sum(0), np.logical_or.accumulate(cols, axis=1).sum(0)
    with ThreadPoolExecutor(THREADS) as pool:
        got = list(pool.map(one, rows.astype(np.int64)))
    return np.array([g[0] for g in got], np.int64), np.array([g[1] for g in got], np.int64)


def one(n):
    W = words(n)
    nbytes = 4 * W * Lw
    print(f"== {n} genomes (W = {W}), {Lw} positions of a {a.pivot}-position pivot, k = {k}: {nbytes / 1e6:.0f} MB of membership rows", flush=True)
    ix, _ = synth.device_index(0, Lw, k, n, a.pivot, pack="keep")
    d_bits = C.c_void_p()
    check(lib().memo_dev_malloc(0, nbytes, C.byref(d_bits)))
    try:
        with ix:
            sweep = []
            for i in range(3 + 5):
                _, t = timed(lambda: (ix.membership_dev(0, Lw, k, n, d_bits.value), ix.check()))
                if i >= 3:
                    sweep.append(t * 1e3)
        print(f"membership sweep, launch to wait: {stats(sweep)}", flush=True)
        floor_ms = nbytes / 8e12 * 1e3
        print(f"the rows over 8 TB/s: {floor_ms:.3f} ms", flush=True)
        host = np.empty((Lw, W), np.uint32)
        check(lib().memo_dev_download(0, host.ctypes.data, d_bits, nbytes, None))          # (first touch of the pages)
        _, t_down = timed(lambda: check(lib().memo_dev_download(0, host.ctypes.data, d_bits, nbytes, None)))
        print(f"download of the rows into pageable host memory: {t_down * 1e3:.1f} ms ({nbytes / t_down / 1e9:.1f} GB/s)", flush=True)
        Lh = min(a.host_positions, Lw)
        B = np.unpackbits(host[:Lh].view(np.uint8), axis=1, bitorder="little")[:, :n].astype(bool)
        for P in map(int, a.orders.split(",")):
            rows = collect.orders(n, 0) if P == 1 else collect.orders(n, P, 1)
            M = rows.shape[1]
            zeros = np.zeros(rows.shape, np.uint64)
            with DevBuffer.of(zeros, 0) as d_core, DevBuffer.of(zeros, 0) as d_covered:
                t = collect_times(d_bits, Lw, n, rows, d_core.d, d_covered.d)
                core = d_core.to_host(rows.shape, np.uint64)
                assert not (core % np.uint64(a.warm + a.repeats)).any()
                core = core // np.uint64(a.warm + a.repeats)
            dev = [s + f for s, f, _ in t]
            steps = P * M * (Lw / 32)
            print(f"memo_collect_dev, P = {P} orders of M = {M} steps: device {stats(dev)} = sweep {stats([s for s, _, _ in t])} + reduce "
                  f"{stats([f for _, f, _ in t])}; blocking call on the host clock {stats([w for _, _, w in t])}", flush=True)
            print(f"   {steps:.3g} lane-steps, {median(dev) * 1e6 / steps * 64:.3f} ns per wave of 64 of them on the whole device; device median over "
                  f"the 8 TB/s floor: {median(dev) / floor_ms:.1f} x; over the sweep before it: {median(dev) / median(sweep):.2f} x; "
                  f"core of the first order after its last step {int(core[0, -1])}", flush=True)
            Ph = min(P, a.host_orders)
            want, t_host = timed(lambda: host_curves(B, rows[:Ph]))
            got = collect.curves((d_bits.value, Lh), n, rows[:Ph])
            assert np.array_equal(got[0].astype(np.int64), want[0]) and np.array_equal(got[1].astype(np.int64), want[1]), "device and host differ"
            scaled = t_host * (Lw / Lh) * (P / Ph)
            print(f"   host route: accumulate in NumPy ({THREADS} threads, one order a task) {t_host * 1e3:.0f} ms for {Ph} orders over {Lh} "
                  f"positions, equal to the device's curves of them; scaled to {P} orders over {Lw} positions {scaled * 1e3:.0f} ms; with the "
                  f"download {(t_down + scaled) * 1e3:.0f} ms against {median(dev):.3f} ms on the device: {(t_down + scaled) * 1e3 / median(dev):.0f} x",
                  flush=True)
    finally:
        lib().memo_dev_free(0, d_bits)


print(f"one session on one MI355X; {lib().memo_version().decode()}", flush=True)
for n in map(int, a.num_docs.split(",")):
    one(n)
