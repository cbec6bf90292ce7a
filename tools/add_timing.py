#!/usr/bin/env python3
"""What `memo add` costs beside `memo index` on the full list (GPU box; profiles/add_timing.txt).
  python tools/add_timing.py [--length 20000000] [--genomes 16] [--out build/add_timing]
The workload of tools/index_timing.py (profiles/index_timing_20M_x16.json): a random pivot and --genomes - 1 copies mutated as
tools/realistic_index.py does.  `memo index -m` on all but the last genome makes the membership index that is grown.  Then
  - the wall clock of `bin/memo add` of the last genome to that index (-o; and once with -o and -c) and of `bin/memo index -m` on the
    full list, --repeats times each, the two alternating, each a process of its own; the two membership files must hold the same rows
    (every pivot character occurs in every genome here);
  - in one process, as memo_amd.add.add_index runs it: the new genome's matching statistics (the library's event pairs and the host
    clock), and batch by batch memo_ms_rows_dev + memo_add_dap_dev and the memo_dap_push_dev it feeds, each between a pair of events on
    the stream the library launches on.  Both calls block, so a pair holds the launches and the waits between them and nothing else.
    The kernel against the time its 8 W positions bytes take at 8 TB/s, and against the push.
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
ap.add_argument("--genomes", type=int, default=16, help="genomes in the grown pangenome, pivot included")
ap.add_argument("--snp-lo", type=float, default=0.001)
ap.add_argument("--snp-hi", type=float, default=0.01)
ap.add_argument("--seed", type=int, default=20260)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--out", default="build/add_timing", help="working directory for the generated genomes (git-ignored)")
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


def main():
    os.makedirs(a.out, exist_ok=True)
    t0 = time.perf_counter()
    fasta = generate()
    n = a.genomes - 1                                                  # genomes in the index that is grown
    old_list, full_list, plus_list = listed("old.txt", fasta[:-1]), listed("full.txt", fasta), listed("plus.txt", [fasta[0], fasta[-1]])
    print(f"== a pivot of {a.length} positions and {a.genomes - 1} mutated genomes (tools/index_timing.py's), generated in {time.perf_counter() - t0:.1f} s", flush=True)
    old = os.path.join(a.out, "old.parquet")
    print(f"-- `memo index -m` on the first {n} genomes, the index that is grown: {wall('index', '-g', old_list, '-o', a.out, '-p', 'old', '-m'):.2f} s", flush=True)
    grown, cons, full = (os.path.join(a.out, name) for name in ("grown.parquet", "grown_cons.parquet", "full.parquet"))
    add_s, index_s = [], []
    for _ in range(a.repeats):
        add_s.append(wall("add", "-b", old, "-n", str(n), "-g", plus_list, "-o", grown))
        index_s.append(wall("index", "-g", full_list, "-o", a.out, "-p", "full", "-m"))
    both_s = wall("add", "-b", old, "-n", str(n), "-g", plus_list, "-o", grown, "-c", cons)
    import pyarrow.parquet as pq
    got, want = pq.read_table(grown), pq.read_table(full)
    print(f"-- wall clock, a process each, the two alternating {a.repeats} times, host clock\n"
          f"   `memo add -o` of genome {a.genomes} to the index of {n}: {stats(add_s, 's')}\n"
          f"   `memo index -m` on all {a.genomes}:             {stats(index_s, 's')}\n"
          f"   add / index = {med(add_s) / med(index_s):.2f}; `memo add -o -c` (both indexes in one run): {both_s:.2f} s\n"
          f"   files: {os.path.getsize(old) / 1e6:.0f} MB read, {os.path.getsize(grown) / 1e6:.0f} MB written; the grown index holds {got.num_rows} rows, "
          f"`memo index -m`'s {want.num_rows}: {'the same rows' if got.equals(want) else 'THE ROWS DIFFER'}", flush=True)
    del got, want

    # ---- inside one run, as add_index makes it
    import torch  # (before the library: both then share one HIP runtime) -- the event pairs, and what the runtime says the device is
    from memo_amd import _lib, add, build_index, convert, lengths
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
    names, pivot, rec_begin = add._match_pivot(old, n, fasta[0])
    W = n - 1 + 1
    kernel, push, sizes = [], [], []

    class Push:
        """the row builder's push alone between the events; the rows are fetched outside them"""

        def __init__(self, builder):
            self.builder = builder

        def push_dev(self, d_dap, positions):
            got = C.c_uint64()
            push.append(timed(lambda: check(lib().memo_dap_push_dev(self.builder._conv._h, d_dap, positions, C.byref(got)))))
            out = self.builder._conv._bufs(got.value)
            if got.value:
                check(lib().memo_dap_fetch(self.builder._conv._h, *[c.ctypes.data for c in out]))
            return out
    with build_index.MatchingStatistics(pivot, rec_begin, 1, 0) as ms:
        records = build_index.read_fasta(fasta[-1])
        t1 = time.perf_counter()
        ms.add_records([s for _, s in records], 0)
        ms_s = time.perf_counter() - t1
        t = ms.timings()
        print(f"-- the new genome's matching statistics ({ms.layout_info()['layout']} layout): {ms_s:.3f} s on the host clock; device: suffix array {t['sa_ms']:.1f} ms, "
              f"LCP + hierarchy {t['lcp_ms']:.1f} ms, walk {t['walk_ms']:.1f} ms", flush=True)

        def matrix(d_cells, pitch, at, first, positions, remaining, d_dap):
            def call():
                d_new = C.c_void_p()
                check(lib().memo_ms_rows_dev(ms._h, at, positions, C.byref(d_new)))
                check(lib().memo_add_dap_dev(d_cells, pitch, n, first, positions, remaining, d_new, 1, d_dap, 0, None))
            kernel.append(timed(call))
            sizes.append(positions)
        feed, buf = lengths.region_feed(old, names[0], 0)
        t1 = time.perf_counter()
        rows = 0
        with buf, convert._RowBuilder(W, rec_begin, False, 0) as builder:
            for part in convert.record_rows([(feed, n)], a.length, Push(builder), 0, None, None, W, matrix):
                rows += len(part[0])
        pipe_s = time.perf_counter() - t1
    whole = [i for i, p in enumerate(sizes) if p == max(sizes)]       # the batches of full length
    k, p, batch = [kernel[i] for i in whole], [push[i] for i in whole], max(sizes)
    floor = 8 * W * batch / 8e12 * 1e3
    print(f"-- {len(sizes)} batches, {len(whole)} of them of {batch} positions x {W} columns ({4 * W * batch / 2 ** 20:.0f} MiB; membership order)\n"
          f"   memo_ms_rows_dev + memo_add_dap_dev: {stats(k)} = {med(k) / floor:.2f} x the 8 TB/s time of its 8 W positions bytes "
          f"({8 * W * batch / med(k) / 1e9:.2f} TB/s)\n"
          f"   memo_dap_push_dev: {stats(p)}\n"
          f"   the kernel is {med(k) / med(p):.3f} of the push it feeds; over the record: {sum(kernel):.1f} ms against {sum(push):.1f} ms\n"
          f"-- the device pipeline (the index's rows out of the Parquet file, both passes of the lengths, every batch's rows fetched; no file written): "
          f"{pipe_s:.2f} s on the host clock, {rows} rows out", flush=True)


main()
