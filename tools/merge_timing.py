#!/usr/bin/env python3
"""What `memo merge` costs beside `memo index` from FASTA, and its kernel beside `memo convert`'s (GPU box; profiles/merge_timing.txt).
  python tools/merge_timing.py [--length 20000000] [--genomes 16] [--out build/merge_timing]
The workload of tools/index_timing.py (profiles/index_timing_20M_x16.json): a random pivot and --genomes - 1 copies mutated as
tools/realistic_index.py does.  `memo index -m` makes the membership index of all of them, and of two groups of them (7 + 8).  Then
  - merge_dap_kernel with the identity map and with a seeded permutation against convert_dap_kernel on the same planes (the full index's,
    read back as `memo merge` reads them), one 128 MiB batch, each call between a pair of events on the stream the library launches on
    (the calls block, so a pair holds one launch and its wait): --warmup calls, then --calls timed ones, the three kernels alternating
    --repeats times.  The ratio, and the bandwidth of the 8 W positions bytes a call moves;
  - the wall clock of `bin/memo merge -c` picking 8 of the 15 genomes against `bin/memo index` on those 8 from FASTA, and of
    `bin/memo merge -o -c` of the two group indexes against `bin/memo index` and `bin/memo index -m` on all 15; a process each, the two
    sides alternating --repeats times; the files of both sides must hold the same rows (every pivot character occurs in every genome);
  - in one process, as memo_amd.merge.merge_index runs the two groups: every batch's memo_merge_dap_dev and the memo_dap_push_dev it
    feeds between event pairs, and the host clock of the whole pipeline without the Parquet writer.
Nothing is gated.  Development tool."""
import argparse
import ctypes as C
import importlib.util
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EXE = os.path.join(ROOT, "bin", "memo")

ap = argparse.ArgumentParser()
ap.add_argument("--length", type=int, default=20_000_000)
ap.add_argument("--genomes", type=int, default=16, help="genomes in the pangenome, pivot included")
ap.add_argument("--snp-lo", type=float, default=0.001)
ap.add_argument("--snp-hi", type=float, default=0.01)
ap.add_argument("--seed", type=int, default=20260)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--calls", type=int, default=30)
ap.add_argument("--out", default="build/merge_timing", help="working directory for the generated genomes (git-ignored)")
a = ap.parse_args()


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def stats(v, unit="ms"):
    return f"median {med(v):.3f} {unit}, min {min(v):.3f}, max {max(v):.3f}"


def generate():
    """the FASTA files of tools/index_timing.py's pangenome: [pivot, g1 ...]"""
    spec = importlib.util.spec_from_file_location("realistic_index", os.path.join(ROOT, "tools", "realistic_index.py"))
    ri = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ri)
    rng = np.random.default_rng(a.seed)
    letters = np.frombuffer(b"ACGT", np.uint8)
    pivot = rng.integers(0, 4, a.length).astype(np.uint8)
    fasta = []

    def write_fasta(path, seq):
        with open(path, "wb") as fh:
            fh.write(b">chr1\n")
            body = letters[seq].tobytes()
            fh.write(b"\n".join(body[i:i + 80] for i in range(0, len(body), 80)) + b"\n")
        fasta.append(path)
    write_fasta(os.path.join(a.out, "pivot.fa"), pivot)
    for g in range(1, a.genomes):
        snp = float(np.exp(rng.uniform(np.log(a.snp_lo), np.log(a.snp_hi))))
        write_fasta(os.path.join(a.out, f"g{g}.fa"), ri.mutate(rng, pivot, snp, g))
    return fasta


def listed(name, paths):
    path = os.path.join(a.out, name)
    with open(path, "w") as fh:
        fh.write("".join(p + "\n" for p in paths))
    return path


def wall(*argv):
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, EXE, *argv], capture_output=True)
    if r.returncode:
        sys.exit(f"memo {' '.join(argv)}: status {r.returncode}\n{r.stderr.decode()[-2000:]}")
    return time.perf_counter() - t0


def same(one, other):
    import pyarrow.parquet as pq
    got, want = pq.read_table(os.path.join(a.out, one)), pq.read_table(os.path.join(a.out, other))
    return f"{one}: {got.num_rows} rows, {other}: {want.num_rows}: {'the same rows' if got.equals(want) else 'THE ROWS DIFFER'}"


def main():
    os.makedirs(a.out, exist_ok=True)
    t0 = time.perf_counter()
    fasta = generate()
    others = a.genomes - 1
    half = others // 2                                                 # 7 of 15
    print(f"== a pivot of {a.length} positions and {others} mutated genomes (tools/index_timing.py's), generated in {time.perf_counter() - t0:.1f} s", flush=True)
    lists = {"full": listed("full.txt", fasta), "a": listed("a.txt", fasta[:1 + half]), "b": listed("b.txt", [fasta[0]] + fasta[1 + half:]),
             "eight": listed("eight.txt", fasta[:9])}
    for name in ("full", "a", "b"):
        print(f"-- `memo index -m` on {name}.txt ({len(open(lists[name]).read().split()) } files): {wall('index', '-g', lists[name], '-o', a.out, '-p', name, '-m'):.2f} s", flush=True)
    full, part_a, part_b = (os.path.join(a.out, name + ".parquet") for name in ("full", "a", "b"))

    # ---- the kernel beside convert_dap_kernel
    import torch  # (before the library: both then share one HIP runtime) -- the event pairs, and what the runtime says the device is
    from memo_amd import _lib, convert, lengths, merge
    from memo_amd._device import DevBuffer
    lib, check = _lib.lib, _lib.check

    def timed(call):
        """device milliseconds between two events around a blocking library call"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)
    props = torch.cuda.get_device_properties(0)
    print(f"device 0: {props.name} ({getattr(props, 'gcnArchName', '?')}), {props.multi_processor_count} CUs, {props.total_memory / 2 ** 30:.0f} GiB; {lib().memo_version().decode()}", flush=True)
    n, W, L = a.genomes, others, a.length
    batch = min(convert.default_batch_positions(n), L)
    maps = {"identity": np.arange(1, n, dtype=np.int32), "permutation": np.random.default_rng(a.seed).permutation(np.arange(1, n)).astype(np.int32)}
    feed, buf = lengths.region_feed(full, "chr1", 0)
    times = {"convert": [], "identity": [], "permutation": []}
    with buf, DevBuffer(0, 4 * W * batch) as d_dap, DevBuffer(0, 4 * W) as d_identity, DevBuffer(0, 4 * W) as d_permutation:
        d_maps = {"identity": d_identity, "permutation": d_permutation}
        for name, host in maps.items():
            check(lib().memo_dev_upload(0, d_maps[name].d, host.ctypes.data, host.nbytes, None))
        for lo, hi, d_cells, pitch in lengths.finished_slices(feed, 0, L, n, L, 0, None):
            assert (lo, hi) == (0, L), "one slice is expected at this size"
            calls = {"convert": lambda: check(lib().memo_convert_dap_dev(d_cells, pitch, n, 0, batch, L, d_dap.d, 0, None)),
                     "identity": lambda: check(lib().memo_merge_dap_dev(d_cells, pitch, n, d_maps["identity"].d, W, 0, batch, L, d_dap.d, 0, None)),
                     "permutation": lambda: check(lib().memo_merge_dap_dev(d_cells, pitch, n, d_maps["permutation"].d, W, 0, batch, L, d_dap.d, 0, None))}
            for _ in range(a.repeats):
                for name, call in calls.items():
                    for _ in range(a.warmup):
                        call()
                    times[name] += [timed(call) for _ in range(a.calls)]
    moved = 8 * W * batch
    print(f"-- one batch of {batch} positions x {W} columns ({4 * W * batch / 2 ** 20:.0f} MiB), {a.repeats} x {a.calls} timed calls each after {a.warmup} warm-up calls, "
          f"the three alternating; a call reads and writes {moved / 2 ** 20:.0f} MiB", flush=True)
    for name, v in times.items():
        what = "memo_convert_dap_dev" if name == "convert" else f"memo_merge_dap_dev, {name} map"
        print(f"   {what}: {stats(v)} = {moved / med(v) / 1e9:.2f} TB/s; {med(v) / med(times['convert']):.3f} x memo_convert_dap_dev", flush=True)

    # ---- wall clocks
    out = {name: os.path.join(a.out, name + ".parquet") for name in ("picked_cons", "merged_memb", "merged_cons")}
    pick_s, eight_s, merge_s, index_s = [], [], [], []
    for _ in range(a.repeats):
        pick_s.append(wall("merge", "-b", full, "-n", str(n), "-s", "1-8", "-c", out["picked_cons"]))
        eight_s.append(wall("index", "-g", lists["eight"], "-o", a.out, "-p", "eight_cons"))
        merge_s.append(wall("merge", "-b", part_a, "-n", str(1 + half), "-b", part_b, "-n", str(n - half), "-o", out["merged_memb"], "-c", out["merged_cons"]))
        index_s.append(wall("index", "-g", lists["full"], "-o", a.out, "-p", "full_cons") + wall("index", "-g", lists["full"], "-o", a.out, "-p", "full_memb", "-m"))
    print(f"-- wall clock, a process each, the sides alternating {a.repeats} times, host clock\n"
          f"   `memo merge -c -s 1-8` from the index of {others}: {stats(pick_s, 's')}\n"
          f"   `memo index` on those 8 from FASTA:          {stats(eight_s, 's')}            merge / index = {med(pick_s) / med(eight_s):.2f}\n"
          f"   {same('picked_cons.parquet', 'eight_cons.parquet')}\n"
          f"   `memo merge -o -c` of the indexes of {half} and {others - half}: {stats(merge_s, 's')}\n"
          f"   `memo index` and `memo index -m` on all {others}: {stats(index_s, 's')}            merge / index = {med(merge_s) / med(index_s):.2f}\n"
          f"   {same('merged_memb.parquet', 'full_memb.parquet')}\n   {same('merged_cons.parquet', 'full_cons.parquet')}\n"
          f"   files: {os.path.getsize(part_a) / 1e6:.0f} + {os.path.getsize(part_b) / 1e6:.0f} MB read, {os.path.getsize(out['merged_memb']) / 1e6:.0f} + "
          f"{os.path.getsize(out['merged_cons']) / 1e6:.0f} MB written", flush=True)

    # ---- inside one run, as merge_index makes it of the two groups
    kernel, push, sizes = [], [], []

    class Push:
        """the row builders' pushes alone between the events; the rows are fetched outside them"""

        def __init__(self, builders):
            self.builders = builders

        def push_dev(self, d_matrix, positions):
            parts = []
            for b in self.builders._each:
                got = C.c_uint64()
                push.append(timed(lambda: check(lib().memo_dap_push_dev(b._conv._h, d_matrix, positions, C.byref(got)))))
                part = b._conv._bufs(got.value)
                if got.value:
                    check(lib().memo_dap_fetch(b._conv._h, *[c.ctypes.data for c in part]))
                parts.append(part)
            return parts
    real = lib().memo_merge_dap_dev

    def timed_kernel(*args):
        rc = []
        kernel.append(timed(lambda: rc.append(real(*args))))
        sizes.append(args[6])
        return rc[0]
    sizes_in, chosen, plane_of = merge._plan([1 + half, n - half], [None, None])
    feeds, bufs = zip(*(lengths.region_feed(path, "chr1", 0) for path in (part_a, part_b)))
    rows = [0, 0]
    t1 = time.perf_counter()
    lib().memo_merge_dap_dev = timed_kernel
    try:
        with bufs[0], bufs[1], convert.Builders(W, [0, L], [False, True], 0) as builders, merge._mapped(sizes_in, plane_of, 0) as mapped:
            for parts in convert.record_rows(list(zip(feeds, sizes_in)), L, Push(builders), 0, None, None, *mapped):
                for i, part in enumerate(parts):
                    rows[i] += len(part[0])
    finally:
        lib().memo_merge_dap_dev = real
    pipe_s = time.perf_counter() - t1
    whole = [i for i, p in enumerate(sizes) if p == max(sizes)]       # the batches of full length
    k, batch = [kernel[i] for i in whole], max(sizes)
    p = [push[2 * i + j] for i in whole for j in (0, 1)]
    print(f"-- two inputs ({1 + half} + {n - half} planes stacked), {len(sizes)} batches, {len(whole)} of them of {batch} positions x {W} columns\n"
          f"   memo_merge_dap_dev: {stats(k)} ({8 * W * batch / med(k) / 1e9:.2f} TB/s)\n"
          f"   memo_dap_push_dev (two builders a batch: membership, conservation): {stats(p)}\n"
          f"   the kernel is {med(k) / med(p):.3f} of one push it feeds; over the record: {sum(kernel):.1f} ms against {sum(push):.1f} ms\n"
          f"-- the device pipeline (both indexes' rows out of their Parquet files, the lengths of both, every batch's rows of both outputs fetched; no file "
          f"written): {pipe_s:.2f} s on the host clock, {rows[0]} + {rows[1]} rows out", flush=True)


main()
