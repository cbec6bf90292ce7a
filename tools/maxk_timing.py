#!/usr/bin/env python3
"""What `memo maxk` costs, launch by launch, and what it spares (GPU box; profiles/maxk_timing.txt).
  python tools/maxk_timing.py                          # BASELINE config 3's rows (100 genomes, 10^8 positions, 5e8 rows, int64 columns)
  python tools/maxk_timing.py --cli 100000000 --out DIR  # + the wall clock of `memo maxk` and `memo query -k 31` on that pivot's Parquet file
In one process, on the index's own int64 columns (memo_index_columns), for T = N, T = N / 2 (conservation) and a genome (membership:
config 4 is config 3's rows read that way):
  - memo_maxk_begin_dev / _rows_dev / _finish_dev: the device time of each launch from event pairs (memo_debug_maxk_times of the A/B
    library: fill, row pass, tile minima, their scan, apply), medians of --repeats warm calls after --warm; the two row-pass
    variants (memo_debug_maxk_rows: wave-aggregated atomics, one atomic per row) alternate call by call, and their results are compared;
  - the row pass against 24 B per row over 8 TB/s, the three scan launches against 8 L bytes over 8 TB/s (one read, one write; they
    move 12 L: the tile minima read the cells once more);
  - the yardstick, reported and not gated: one conservation sweep of the int64 columns at k = 257 (memo_query_conservation_dev,
    launch to wait on the host clock), times ceil(log2(cap)) -- the binary search over k this replaces."""
import argparse
import ctypes as C
import math
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from memo_amd import _lib, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--positions", type=int, default=100_000_000)
ap.add_argument("--num-docs", type=int, default=100)
ap.add_argument("--cap", type=int, default=100_000)
ap.add_argument("--warm", type=int, default=5)
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--cli", type=int, default=0, help="also time bin/memo maxk and bin/memo query on a synthetic Parquet index of this many positions")
ap.add_argument("--cli-only", action="store_true", help="skip the device part")
ap.add_argument("--out", default="/tmp/maxk_timing")
a = ap.parse_args()
M, n, cap = a.positions, a.num_docs, a.cap
_lib.use_ab(True)
lib, check = _lib.lib, _lib.check


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def stats(v):
    return f"median {med(v):.3f} ms, min {min(v):.3f}, max {max(v):.3f}"


def one_call(cols, rows, d_cells, mode, arg, way):
    """the five device times of one begin / rows / finish"""
    ms = (C.c_float * 5)()
    check(lib().memo_debug_maxk_rows(way))
    check(lib().memo_debug_maxk_times(1, None))
    check(lib().memo_maxk_begin_dev(d_cells, M, cap, 0, None))
    check(lib().memo_maxk_rows_dev(*cols, rows, 0, M, cap, mode, arg, d_cells, 0, None))
    check(lib().memo_maxk_finish_dev(d_cells, M, cap, 0, None))
    check(lib().memo_debug_maxk_times(0, ms))
    check(lib().memo_debug_maxk_rows(0))
    return list(ms)


def device_part():
    print(f"== {n} genomes, a window of {M} positions, cap {cap}", flush=True)
    ix, (r0, r1) = synth.device_index(0, M, 257, n, M)
    rows = r1 - r0
    d_cells, d_sweep = C.c_void_p(), C.c_void_p()
    check(lib().memo_dev_malloc(0, 4 * M, C.byref(d_cells)))
    check(lib().memo_dev_malloc(0, 2 * M, C.byref(d_sweep)))
    try:
        with ix:
            row_floor, scan_floor = 24 * rows / 8e12 * 1e3, 8 * M / 8e12 * 1e3
            print(f"{rows} rows as int64 columns: {24 * rows / 1e9:.1f} GB, {row_floor:.3f} ms at 8 TB/s; cells {4 * M / 1e6:.0f} MB, "
                  f"8 L bytes at 8 TB/s {scan_floor:.3f} ms", flush=True)
            sweep = []
            for i in range(a.warm + a.repeats):
                t = time.perf_counter()
                ix.conservation_dev(0, M, 257, n, d_sweep.value)
                ix.check()
                if i >= a.warm:
                    sweep.append((time.perf_counter() - t) * 1e3)
            steps = math.ceil(math.log2(cap))
            print(f"yardstick: one conservation sweep of the int64 columns at k = 257, launch to wait: {stats(sweep)}; "
                  f"x ceil(log2({cap})) = {steps} sweeps: {steps * med(sweep):.1f} ms (and {steps} result vectors compared on the host)", flush=True)
            cols = ix.columns()          # (after the sweeps: the index is not finalized any more once its columns are handed out)
            for mode, arg, what in ((0, n, f"T = N = {n} (every row is selected)"), (0, n // 2, f"T = N / 2 = {n // 2}"),
                                    (1, 1, "genome 1 of the membership reading (config 4)")):
                print(f"-- {what}", flush=True)
                times = {0: [], 1: []}
                results = {}
                for i in range(a.warm + a.repeats):
                    for way in (0, 1):
                        ms = one_call(cols, rows, d_cells, mode, arg, way)
                        if i >= a.warm:
                            times[way].append(ms)
                        if i == 0:
                            out = np.empty(M, np.uint32)
                            check(lib().memo_dev_download(0, out.ctypes.data, d_cells, out.nbytes, None))
                            results[way] = out
                assert np.array_equal(results[0], results[1]), "the two row passes differ"
                r = results[0]
                print(f"   both row passes give the same {M} lengths: min {r.min()}, median {int(np.median(r))}, max {r.max()}, "
                      f"{(r == cap).mean():.4f} of them at the cap", flush=True)
                for way, name in ((0, "wave-aggregated atomics"), (1, "one atomic per row")):
                    t = np.asarray(times[way])
                    print(f"   row pass, {name}: {stats(t[:, 1])} = {med(t[:, 1]) / row_floor:.2f} x the 8 TB/s time of its 24 B / row "
                          f"({24 * rows / med(t[:, 1]) / 1e9:.2f} TB/s); {med(t[:, 1]) / med(sweep):.2f} sweeps", flush=True)
                t = np.asarray(times[0] + times[1])
                scan = t[:, 2] + t[:, 3] + t[:, 4]
                print(f"   fill: {stats(t[:, 0])}; scan = tile minima {med(t[:, 2]):.3f} + their scan {med(t[:, 3]):.3f} + apply {med(t[:, 4]):.3f}: "
                      f"{stats(scan)} = {med(scan) / scan_floor:.2f} x the 8 TB/s time of 8 L bytes", flush=True)
                whole = t[: len(times[0]), 0] + t[: len(times[0]), 1] + scan[: len(times[0])]
                print(f"   the whole pass (wave-aggregated atomics): median {med(whole):.3f} ms = {med(whole) / med(sweep):.2f} sweeps at k = 257, against "
                      f"{steps} for the search", flush=True)
    finally:
        lib().memo_dev_free(0, d_cells)
        lib().memo_dev_free(0, d_sweep)


def cli_part():
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, f"synth_n{n}_{a.cli}.parquet")
    t = time.time()
    rows = synth.write_parquet(path, n, a.cli)
    print(f"== the command line: wrote {rows} rows, {os.path.getsize(path) / 1e6:.0f} MB of Parquet in {time.time() - t:.0f} s", flush=True)
    exe, out = os.path.join(ROOT, "bin", "memo"), os.path.join(a.out, "out.txt")
    common = ["-b", path, "-n", str(n), "-r", f"chr1:0-{a.cli}", "-o", out]
    for name, argv in (("memo maxk (T = N)", ["maxk", *common]), ("memo maxk -K 100000", ["maxk", *common, "-K", "100000"]),
                       ("memo query -k 31", ["query", *common, "-k", "31"]), ("memo maxk (T = N), again", ["maxk", *common])):
        t = time.time()
        r = subprocess.run([sys.executable, exe, *argv], capture_output=True, env=dict(os.environ, MEMO_CACHE="0"))
        wall = time.time() - t
        size = os.path.getsize(out) if os.path.exists(out) else -1
        print(f"{name}: wall {wall:.2f} s, rc {r.returncode}, output {size / 1e6:.0f} MB" + (f" {r.stderr.decode()[-300:]}" if r.returncode else ""),
              flush=True)
        if os.path.exists(out):
            os.unlink(out)
    os.unlink(path)


print(f"one session on one MI355X; {lib().memo_version().decode()}", flush=True)
if not a.cli_only:
    device_part()
if a.cli:
    cli_part()
