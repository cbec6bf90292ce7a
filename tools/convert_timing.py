#!/usr/bin/env python3
"""What `memo convert` costs on the device, launch by launch (GPU box; profiles/convert_timing.txt).
  python tools/convert_timing.py                 # the workload of tools/lengths_timing.py: 100 genomes, 10^7 positions, 5 * 10^7 rows
In one process, on the index's own int64 columns (memo_index_columns), medians of --repeats warm calls after --warm:
  - pass A (memo_lengths_carry_dev over the rows right of the first slice: its carry), begin, rows (the slice's own), finish of that
    slice: the device time of each launch from the library's own event pairs (memo_debug_lengths_times of the A/B library);
  - convert_dap_kernel and the memo_dap_push_dev it feeds, batch by batch as the product runs them (the default batch: a matrix of about
    128 MiB), each between a pair of events on the stream the library launches on.  Both calls block, so a pair holds the launches and the
    waits between them and nothing else.  The kernel against the time its 8 (N - 1) positions bytes take at 8 TB/s, and against the push;
  - the whole device pipeline (memo_amd.convert._converted_rows on the device columns: both passes, every batch's rows fetched to the host),
    launch to last row on the host clock.  No Parquet file is read or written here."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch  # (before the library, as tools/ab.py: both then share one HIP runtime) -- the event pairs, and what the runtime says the device is

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from memo_amd import _lib, convert, lengths, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--positions", type=int, default=10_000_000)
ap.add_argument("--num-docs", type=int, default=100)
ap.add_argument("--warm", type=int, default=5)
ap.add_argument("--repeats", type=int, default=20)
a = ap.parse_args()
M, n = a.positions, a.num_docs
cap = min(M, 2 ** 31 - 1)
_lib.use_ab(True)
lib, check = _lib.lib, _lib.check


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def stats(v):
    return f"median {med(v):.3f} ms, min {min(v):.3f}, max {max(v):.3f}"


def timed(call):
    """device milliseconds between two events around a blocking library call"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    props = torch.cuda.get_device_properties(0)
    print(f"device 0: {props.name} ({getattr(props, 'gcnArchName', '?')}), {props.multi_processor_count} CUs, {props.total_memory / 2 ** 30:.0f} GiB; {lib().memo_version().decode()}", flush=True)
    print(f"== {n} genomes, a record of {M} positions: a synthetic index (memo_amd/synth.py) read as a membership index", flush=True)
    ix, (r0, r1) = synth.device_index(0, M, 257, n, M)
    rows = r1 - r0
    step = min(lengths.default_slice_positions(n), M)              # one slice of the product
    pitch = (step + 3) & ~3
    batch = min(convert.default_batch_positions(n), step)
    bufs = [C.c_void_p() for _ in range(3)]
    d_cells, d_carry, d_dap = bufs
    for d, size in zip(bufs, (4 * n * pitch, 8 * n, 4 * (n - 1) * batch)):
        check(lib().memo_dev_malloc(0, size, C.byref(d)))
    none = np.full(n, np.iinfo(np.int64).max, np.int64)
    check(lib().memo_dev_upload(0, d_carry, none.ctypes.data, none.nbytes, None))
    try:
        with ix:
            cols = ix.columns()
            num, den = synth.rows_per_position(n)

            def between(lo, hi):
                """(d_start, d_end, d_annot, rows) of the rows with lo < start < hi: the synthetic rows are sorted by start"""
                i0, i1 = (min(max(synth.first_row_at_or_after(x, num, den) - r0, 0), rows) for x in (lo + 1, hi))
                return (*(c + 8 * i0 for c in cols), max(i1 - i0, 0))
            own, right = between(0, step + 1), between(step, M + cap)
            print(f"{rows} rows as int64 columns: {24 * rows / 1e9:.2f} GB; a slice is {step} positions "
                  f"({4 * n * pitch / 1e9:.2f} GB of planes), a batch {batch} positions ({4 * (n - 1) * batch / 2 ** 20:.0f} MiB)", flush=True)
            # ---- the lengths' launches on the first slice [0, step), each pass on the rows the product hands it
            times = []
            for i in range(a.warm + a.repeats):
                ms = (C.c_float * 7)()
                check(lib().memo_dev_upload(0, d_carry, none.ctypes.data, none.nbytes, None))
                check(lib().memo_debug_lengths_times(1, None))
                check(lib().memo_lengths_carry_dev(*right, step, M + cap, n, d_carry, 0, None))   # the slice's own carry: the rows right of it
                check(lib().memo_lengths_begin_dev(d_cells, step, pitch, n, cap, 0, d_carry, 0, None))
                check(lib().memo_lengths_rows_dev(*own, 0, step, pitch, n, cap, d_cells, 0, None))
                check(lib().memo_lengths_finish_dev(d_cells, step, pitch, n, cap, 0, None))
                check(lib().memo_debug_lengths_times(0, ms))
                if i >= a.warm:
                    times.append(list(ms))
            t = np.asarray(times)
            print(f"-- the first slice, {step} positions: its own {own[3]} rows through the row pass, the {right[3]} rows right of it through the carry pass", flush=True)
            print(f"   pass A (carry): {stats(t[:, 2])} = {med(t[:, 2]) / (24 * right[3] / 8e12 * 1e3):.2f} x the 8 TB/s time of 24 B / row", flush=True)
            print(f"   begin: {stats(t[:, 0])}", flush=True)
            print(f"   rows: {stats(t[:, 1])} = {med(t[:, 1]) / (24 * own[3] / 8e12 * 1e3):.2f} x the 8 TB/s time of 24 B / row", flush=True)
            fin = t[:, 3] + t[:, 4] + t[:, 5]
            print(f"   finish: {stats(fin)} = {med(fin) / (8 * n * step / 8e12 * 1e3):.2f} x the 8 TB/s time of 8 N L bytes", flush=True)
            # ---- the new kernel and the push it feeds, batch after batch of the finished slice
            from memo_amd.dap_to_bed import DapConverter
            kernel, push, out_rows = [], [], []
            with DapConverter(n - 1, [0, M], True, True, 0) as conv:
                for i in range(min(a.warm + a.repeats, M // batch)):   # (the builder takes M positions and no more)
                    first = i % (step // batch) * batch              # the slice's batches, round and round
                    got = C.c_uint64()
                    k_ms = timed(lambda: check(lib().memo_convert_dap_dev(d_cells, pitch, n, first, batch, M - first, d_dap, 0, None)))
                    p_ms = timed(lambda: check(lib().memo_dap_push_dev(conv._h, d_dap, batch, C.byref(got))))
                    if i >= a.warm:
                        kernel.append(k_ms), push.append(p_ms), out_rows.append(got.value)
            floor = 8 * (n - 1) * batch / 8e12 * 1e3
            print(f"-- {len(kernel)} batches of {batch} positions x {n - 1} columns (conservation order)", flush=True)
            print(f"   convert_dap_kernel: {stats(kernel)} = {med(kernel) / floor:.2f} x the 8 TB/s time of its 8 (N - 1) positions bytes "
                  f"({8 * (n - 1) * batch / med(kernel) / 1e9:.2f} TB/s)", flush=True)
            print(f"   memo_dap_push_dev: {stats(push)}; {int(np.median(out_rows))} rows a batch", flush=True)
            print(f"   the transposition is {med(kernel) / med(push):.3f} of the push it feeds; over the record's {-(-M // batch)} batches: "
                  f"{med(kernel) * -(-M // batch):.1f} ms against {med(push) * -(-M // batch):.1f} ms", flush=True)
            # ---- the whole device pipeline, as the product runs it on these columns

            def feed(lo, hi):
                yield between(lo, hi)
            for order in (True, False):
                t0 = time.perf_counter()
                total = 0
                with convert._RowBuilder(n - 1, [0, M], order, 0) as builder:
                    for part in convert._converted_rows(feed, M, n, builder, 0, None, None):
                        total += len(part[0])
                print(f"-- the device pipeline, {'conservation' if order else 'membership'} order: {time.perf_counter() - t0:.2f} s on the host clock for "
                      f"{M} positions in {-(-M // step)} slices, {total} rows out (every slice's rows where they lie in device memory; no Parquet)", flush=True)
            print("not taken: the wall clock of `bin/memo convert` on a Parquet file of this index beside `memo index`'s", flush=True)
    finally:
        for d in bufs:
            lib().memo_dev_free(0, d)


main()
