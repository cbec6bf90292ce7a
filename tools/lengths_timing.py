#!/usr/bin/env python3
"""What `memo lengths` costs, launch by launch, and what it replaces (GPU box; profiles/lengths_timing.txt).
  python tools/lengths_timing.py                 # a synthetic membership index: 100 genomes, a window of 10^7 positions, cap 10^5
In one process, on the index's own int64 columns (memo_index_columns):
  - memo_lengths_begin_dev / _rows_dev / _carry_dev / _finish_dev / _select_dev: the device time of each launch from event pairs
    (memo_debug_lengths_times of the A/B library), medians of --repeats warm calls after --warm;
  - the row pass and the carry pass against 24 B per row over 8 TB/s; finish against 8 N L bytes (one read, one write; it moves 12 N L);
    select against its 4 N L bytes read, and against its rounds (the bit width of the largest length under the cap, + 1);
  - the yardstick, reported and not gated: N - 1 passes of the shipped `memo maxk` genome mode (begin, rows, finish per genome) over the
    same device rows, launch to wait on the host clock, alternating call by call with the whole new pass timed the same way;
  - planes of the two routes are compared."""
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
ap.add_argument("--cap", type=int, default=100_000)
ap.add_argument("--warm", type=int, default=5)
ap.add_argument("--repeats", type=int, default=20)
a = ap.parse_args()
M, n, cap = a.positions, a.num_docs, a.cap
pitch = (M + 3) & ~3
_lib.use_ab(True)
lib, check = _lib.lib, _lib.check
NAMES = ("begin (fill)", "rows", "carry", "finish: tile minima", "finish: their scan", "finish: apply", "select")


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def stats(v):
    return f"median {med(v):.3f} ms, min {min(v):.3f}, max {max(v):.3f}"


def new_pass(cols, rows, d_cells, d_carry, d_out, threshold, timed):
    """begin, rows, carry, finish, select; the seven device times when timed"""
    ms = (C.c_float * 7)()
    if timed:
        check(lib().memo_debug_lengths_times(1, None))
    check(lib().memo_lengths_begin_dev(d_cells, M, pitch, n, cap, 0, None, 0, None))
    check(lib().memo_lengths_rows_dev(*cols, rows, 0, M, pitch, n, cap, d_cells, 0, None))
    if timed:                                        # (a whole window needs no carry: timed because a sliced one runs it once per row, too)
        check(lib().memo_lengths_carry_dev(*cols, rows, 0, M + 1, n, d_carry, 0, None))
    check(lib().memo_lengths_finish_dev(d_cells, M, pitch, n, cap, 0, None))
    check(lib().memo_lengths_select_dev(d_cells, M, pitch, n, cap, threshold, d_out, 0, None))
    if timed:
        check(lib().memo_debug_lengths_times(0, ms))
    return list(ms)


def old_route(cols, rows, d_one, genomes):
    """the route this replaces: one `memo maxk` genome pass per genome (the selection over their results would still be to do)"""
    for g in genomes:
        check(lib().memo_maxk_begin_dev(d_one, M, cap, 0, None))
        check(lib().memo_maxk_rows_dev(*cols, rows, 0, M, cap, 1, g, d_one, 0, None))
        check(lib().memo_maxk_finish_dev(d_one, M, cap, 0, None))


def main():
    props = torch.cuda.get_device_properties(0)
    print(f"device 0: {props.name} ({getattr(props, 'gcnArchName', '?')}), {props.multi_processor_count} CUs, {props.total_memory / 2 ** 30:.0f} GiB; {lib().memo_version().decode()}", flush=True)
    print(f"== {n} genomes, a window of {M} positions, cap {cap}: a synthetic index (memo_amd/synth.py) read as a membership index", flush=True)
    ix, (r0, r1) = synth.device_index(0, M, 257, n, M)
    rows = r1 - r0
    bufs = [C.c_void_p() for _ in range(4)]
    d_cells, d_carry, d_out, d_one = bufs
    for d, size in zip(bufs, (4 * n * pitch, 8 * n, 4 * M, 4 * M)):
        check(lib().memo_dev_malloc(0, size, C.byref(d)))
    none = np.full(n, np.iinfo(np.int64).max, np.int64)
    check(lib().memo_dev_upload(0, d_carry, none.ctypes.data, none.nbytes, None))
    try:
        with ix:
            cols = ix.columns()
            row_floor, plane_bytes = 24 * rows / 8e12 * 1e3, 4 * n * M
            print(f"{rows} rows as int64 columns: {24 * rows / 1e9:.2f} GB, {row_floor:.3f} ms at 8 TB/s; planes {plane_bytes / 1e9:.2f} GB, "
                  f"{plane_bytes / 8e12 * 1e3:.3f} ms at 8 TB/s", flush=True)
            for threshold in (n, n // 2, 1):
                times = []
                for i in range(a.warm + a.repeats):
                    ms = new_pass(cols, rows, d_cells, d_carry, d_out, threshold, True)
                    if i >= a.warm:
                        times.append(ms)
                t = np.asarray(times)
                sel = np.empty(M, np.uint32)
                check(lib().memo_dev_download(0, sel.ctypes.data, d_out, sel.nbytes, None))
                under = sel[sel < cap]
                rounds = (int(under.max()).bit_length() if len(under) else 0) + 1
                print(f"-- T = {threshold}: sel min {sel.min()}, median {int(np.median(sel))}, max {sel.max()}, {(sel == cap).mean():.4f} at the cap", flush=True)
                if threshold == n:
                    for i, name in enumerate(NAMES[:6]):
                        print(f"   {name}: {stats(t[:, i])}", flush=True)
                    print(f"   rows = {med(t[:, 1]) / row_floor:.2f} x the 8 TB/s time of its 24 B / row ({24 * rows / med(t[:, 1]) / 1e9:.2f} TB/s); "
                          f"carry = {med(t[:, 2]) / row_floor:.2f} x ({24 * rows / med(t[:, 2]) / 1e9:.2f} TB/s)", flush=True)
                    fin = t[:, 3] + t[:, 4] + t[:, 5]
                    print(f"   finish: {stats(fin)} = {med(fin) / (2 * plane_bytes / 8e12 * 1e3):.2f} x the 8 TB/s time of 8 N L bytes", flush=True)
                print(f"   select: {stats(t[:, 6])} = {med(t[:, 6]) / (plane_bytes / 8e12 * 1e3):.2f} x the 8 TB/s time of its 4 N L bytes "
                      f"({plane_bytes / med(t[:, 6]) / 1e9:.2f} TB/s); at most {rounds} passes over a tile's values in LDS "
                      f"(largest length under the cap: {int(under.max()) if len(under) else 0})", flush=True)
            # the two routes, alternating, launch to wait on the host clock
            new_ms, old_ms = [], []
            for i in range(a.warm + a.repeats):
                t0 = time.perf_counter()
                new_pass(cols, rows, d_cells, d_carry, d_out, n, False)
                t1 = time.perf_counter()
                old_route(cols, rows, d_one, range(1, n))
                t2 = time.perf_counter()
                if i >= a.warm:
                    new_ms.append((t1 - t0) * 1e3)
                    old_ms.append((t2 - t1) * 1e3)
            print(f"-- the two routes on the same device rows, alternating, host clock (the new one: begin, rows, finish, select at T = N; the old one: "
                  f"{n - 1} x begin, rows, finish of `memo maxk` in genome mode, no selection)", flush=True)
            print(f"   memo lengths: {stats(new_ms)}", flush=True)
            print(f"   {n - 1} x memo maxk -m -d G: {stats(old_ms)} ({med(old_ms) / (n - 1):.3f} ms a genome)", flush=True)
            print(f"   ratio: {med(old_ms) / med(new_ms):.2f}", flush=True)
            # the planes of the two routes (the old route's last genome, and genome 1)
            for g in (n - 1, 1):
                old_route(cols, rows, d_one, (g,))
                one, plane = np.empty(M, np.uint32), np.empty(M, np.uint32)
                check(lib().memo_dev_download(0, one.ctypes.data, d_one, one.nbytes, None))
                check(lib().memo_dev_download(0, plane.ctypes.data, C.c_void_p(d_cells.value + 4 * g * pitch), plane.nbytes, None))
                assert np.array_equal(one, plane), f"plane {g} differs from memo maxk's genome mode"
            print("   planes 1 and N - 1 equal the genome passes'", flush=True)
    finally:
        for d in bufs:
            lib().memo_dev_free(0, d)


main()
