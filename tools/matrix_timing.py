#!/usr/bin/env python3
"""What `memo matrix` costs and what it spares (GPU box; profiles/matrix_timing.txt).
  python tools/matrix_timing.py                       # BASELINE config 4's result (10^7 positions of the 100-genome pangenome, W = 4)
                                                      # and the same window of a 500-genome pangenome (W = 16)
Per pangenome, in one process:
  - the membership sweep that produces the input, launch to wait (host clock around work that ends in a device wait);
  - memo_cooccurrence_dev on that result: the device time of its launches from event pairs (memo_debug_cooc_times of the A/B
    library: the sweep launches, the reduce launches), warm, after --warm calls that also ramp the clocks, and the host clock
    around the whole blocking call (with its scratch allocation); partials and atomics alternate, the matrices are compared;
  - the input's bytes over 8 TB/s: the least the sweep's read of its rows could take;
  - the host route it replaces: the download of the same buffer into pageable host memory (the box's measured device-to-host
    rate) and B.T @ B in NumPy on the threads the box grants -- float32 BLAS over chunks of --chunk positions, each chunk's counts
    exact (below 2^24), summed in float64; timed on --host-positions positions and scaled to the window, which is said in the line.
The matrix of the device is compared with the host's on the timed positions."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from memo_amd import _lib, matrix, synth  # noqa: E402
from memo_amd.index import words  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--positions", type=int, default=10_000_000)
ap.add_argument("--pivot", type=int, default=100_000_000)
ap.add_argument("--num-docs", default="100,500")
ap.add_argument("--warm", type=int, default=5)
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--host-positions", type=int, default=2_000_000)
ap.add_argument("--chunk", type=int, default=250_000)
a = ap.parse_args()
M, k = a.positions, 31
_lib.use_ab(True)
lib, check = _lib.lib, _lib.check


def timed(fn):
    t = time.perf_counter()
    r = fn()
    return r, time.perf_counter() - t


def stats(ms):
    ms = sorted(ms)
    return f"median {ms[len(ms) // 2]:.3f} ms, min {ms[0]:.3f}, max {ms[-1]:.3f} ({len(ms)} calls)"


def cooc_times(d_bits, L, n, d_counts, way):
    """(device ms of the sweeps, of the reduce launches, host ms of the blocking call) per call"""
    check(lib().memo_debug_cooc_flush(way))
    out, ms = [], (C.c_float * 2)()
    for i in range(a.warm + a.repeats):
        check(lib().memo_debug_cooc_times(1, None))
        _, wall = timed(lambda: check(lib().memo_cooccurrence_dev(d_bits, L, n, d_counts, 0, None)))
        check(lib().memo_debug_cooc_times(0, ms))
        if i >= a.warm:
            out.append((ms[0], ms[1], wall * 1e3))
    check(lib().memo_debug_cooc_flush(0))
    return out


def host_matrix(bits, n):
    """B.T @ B of host rows uint32 [L, W], in chunks"""
    total = np.zeros((n, n), np.float64)
    for at in range(0, len(bits), a.chunk):
        rows = bits[at:at + a.chunk]
        B = np.unpackbits(rows.view(np.uint8), axis=1, bitorder="little")[:, :n].astype(np.float32)
        total += B.T @ B
    return total


def one(n):
    W = words(n)
    nbytes = 4 * W * M
    print(f"== {n} genomes (W = {W}), {M} positions of a {a.pivot}-position pivot, k = {k}: {nbytes / 1e6:.0f} MB of membership rows", flush=True)
    ix, _ = synth.device_index(0, M, k, n, a.pivot, pack="keep")
    d_bits, d_counts = C.c_void_p(), C.c_void_p()
    check(lib().memo_dev_malloc(0, nbytes, C.byref(d_bits)))
    check(lib().memo_dev_malloc(0, 8 * n * n, C.byref(d_counts)))
    try:
        with ix:
            sweep = []
            for i in range(3 + 5):
                _, t = timed(lambda: (ix.membership_dev(0, M, k, n, d_bits.value), ix.check()))
                if i >= 3:
                    sweep.append(t * 1e3)
        print(f"membership sweep, launch to wait: {stats(sweep)}", flush=True)
        floor_ms = nbytes / 8e12 * 1e3
        print(f"the rows over 8 TB/s: {floor_ms:.3f} ms", flush=True)
        results = {}
        for way, name in ((0, "partials + reduce"), (1, "atomics"), (0, "partials + reduce (again)"), (1, "atomics (again)")):
            zero = np.zeros((n, n), np.uint64)
            check(lib().memo_dev_upload(0, d_counts, zero.ctypes.data, zero.nbytes, None))
            t = cooc_times(d_bits, M, n, d_counts, way)
            got = np.empty((n, n), np.uint64)
            check(lib().memo_dev_download(0, got.ctypes.data, d_counts, got.nbytes, None))
            assert not (got % np.uint64(a.warm + a.repeats)).any()
            results[name] = got // np.uint64(a.warm + a.repeats)
            dev = [s + f for s, f, _ in t]
            print(f"memo_cooccurrence_dev, {name}: device {stats(dev)} = sweep {stats([s for s, _, _ in t])} + flush "
                  f"{stats([f for _, f, _ in t])}; blocking call on the host clock {stats([w for _, _, w in t])}", flush=True)
            print(f"   device median over the 8 TB/s floor: {sorted(dev)[len(dev) // 2] / floor_ms:.1f} x; over the sweep before it: "
                  f"{sorted(dev)[len(dev) // 2] / sorted(sweep)[len(sweep) // 2]:.2f} x", flush=True)
        first = results["partials + reduce"]
        assert all(np.array_equal(first, r) for r in results.values()), "partials and atomics differ"
        print(f"the four matrices are equal; C[0][0] = {int(first[0, 0])} (the pivot: every position), "
              f"present bits {np.diag(first).sum() / (M * n):.3f} of all", flush=True)
        # the host route: download, unpack, B.T @ B
        host = np.empty((M, W), np.uint32)
        check(lib().memo_dev_download(0, host.ctypes.data, d_bits, nbytes, None))          # (first touch of the pages)
        _, t_down = timed(lambda: check(lib().memo_dev_download(0, host.ctypes.data, d_bits, nbytes, None)))
        print(f"download of the rows into pageable host memory: {t_down * 1e3:.1f} ms ({nbytes / t_down / 1e9:.1f} GB/s)", flush=True)
        P = min(a.host_positions, M)
        host_matrix(host[:a.chunk], n)                                                      # (BLAS threads up)
        want, t_host = timed(lambda: host_matrix(host[:P], n))
        got = matrix.cooccurrence((d_bits.value, P), n)
        assert np.array_equal(got.astype(np.float64), want), "device and host matrices differ"
        scaled = t_host * M / P
        print(f"B.T @ B in NumPy (float32 BLAS, chunks of {a.chunk}, {os.environ.get('OMP_NUM_THREADS', '?')} threads): {t_host * 1e3:.0f} ms for "
              f"{P} positions, equal to the device's matrix of them; scaled to {M} positions: {scaled * 1e3:.0f} ms", flush=True)
        dev_med = sorted(s + f for s, f, _ in cooc_times(d_bits, M, n, d_counts, 0))[a.repeats // 2]
        print(f"host route (download + product, scaled) {(t_down + scaled) * 1e3:.0f} ms against {dev_med:.3f} ms on the device: "
              f"{(t_down + scaled) * 1e3 / dev_med:.0f} x", flush=True)
    finally:
        lib().memo_dev_free(0, d_bits)
        lib().memo_dev_free(0, d_counts)


print(f"one session on one MI355X; {lib().memo_version().decode()}", flush=True)
for n in map(int, a.num_docs.split(",")):
    one(n)
