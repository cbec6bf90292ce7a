#!/usr/bin/env python3
"""What `memo regions` costs and what it spares (GPU box; profiles/regions_timing.txt).
  python tools/regions_timing.py --positions 100000000                  # the runs calls on BASELINE config 3's result, and on a
                                                                        # membership result of --memb-window positions
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/regions_timing.py --positions 100000000 --kernels-only
                                                                        # the same calls, once each, for the kernels' own times
  python tools/regions_timing.py --positions 100000000 --cli            # + bin/memo regions against bin/memo query, alternating, on a
                                                                        # synthetic Parquet index with a warm sidecar cache
  python tools/regions_timing.py --real DIR                             # the same two commands on tools/realistic_index.py's index in DIR
The calls are blocking (count, scan, a wait for the total, two allocations, scatter, a wait), so the host clock around them is the
cost a caller sees; the kernels alone are rocprofv3's."""
import argparse
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from memo_amd import regions, synth  # noqa: E402
from memo_amd._lib import check, lib  # noqa: E402
from memo_amd.index import words  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--positions", type=int, default=100_000_000)
ap.add_argument("--memb-window", type=int, default=10_000_000)
ap.add_argument("--num-docs", type=int, default=100)
ap.add_argument("--kernels-only", action="store_true")
ap.add_argument("--cli", action="store_true")
ap.add_argument("--real", default=None, help="directory tools/realistic_index.py wrote (cons.parquet, memb.npz)")
ap.add_argument("--repeats", type=int, default=3)
a = ap.parse_args()
N, M, n, k = a.positions, a.memb_window, a.num_docs, 31
EXE = os.path.join(ROOT, "bin", "memo")


def timed(fn):
    t = time.perf_counter()
    r = fn()
    return r, time.perf_counter() - t


def dev_buffer(nbytes):
    p = C.c_void_p()
    check(lib().memo_dev_malloc(0, nbytes, C.byref(p)))
    return p


def device_legs():
    reps = 1 if a.kernels_only else a.repeats
    ix, _ = synth.device_index(0, N, k, n, N, pack="dense")
    d_vec = dev_buffer(2 * N)
    with ix:
        for _ in range(reps):
            _, t = timed(lambda: (ix.conservation_dev(0, N, k, n, d_vec.value), ix.check()))
            print(f"conservation sweep of {N} positions ({n} genomes, k = {k}), launch to wait: {t * 1e3:.2f} ms", flush=True)
    for what, call in (("value", lambda: regions.runs((d_vec.value, N))), (f"band [{n}, {n}]", lambda: regions.runs((d_vec.value, N), "band", n, n)),
                       ("band [1, 3]", lambda: regions.runs((d_vec.value, N), "band", 1, 3))):
        for _ in range(reps):
            r, t = timed(call)
            runs = len(r[0]) if isinstance(r, tuple) else len(r)
            out = runs * (10 if isinstance(r, tuple) else 8)
            print(f"runs, {what}: {runs} runs ({N / max(runs, 1):.1f} positions a run), {t * 1e3:.2f} ms with the download of {out / 1e6:.1f} MB; "
                  f"kernel bytes 2 x {2 * N / 1e6:.0f} MB read + {out / 1e6:.1f} MB written", flush=True)
    lib().memo_dev_free(0, d_vec)
    W = words(n)
    ix, _ = synth.device_index(0, M, k, n, N, pack="keep")
    d_bits = dev_buffer(4 * W * M)
    with ix:
        for _ in range(reps):
            _, t = timed(lambda: (ix.membership_dev(0, M, k, n, d_bits.value), ix.check()))
            print(f"membership sweep of {M} positions (W = {W}), launch to wait: {t * 1e3:.2f} ms", flush=True)
    for _ in range(reps):
        (starts, rows), t = timed(lambda: regions.membership_runs((d_bits.value, M), n))
        out = len(starts) * (8 + 4 * W)
        print(f"runs, bits: {len(starts)} runs ({M / max(len(starts), 1):.1f} positions a run), {t * 1e3:.2f} ms with the download of {out / 1e6:.1f} MB; "
              f"kernel bytes 2 x {4 * W * M / 1e6:.0f} MB read + {out / 1e6:.1f} MB written", flush=True)
    lib().memo_dev_free(0, d_bits)


def run(env, *argv):
    r, wall = timed(lambda: subprocess.run([sys.executable, EXE, *argv], capture_output=True, env=env))
    assert r.returncode == 0, r.stderr.decode()[-600:]
    return wall


def count_lines(path):
    with open(path, "rb") as fh:
        return sum(buf.count(b"\n") for buf in iter(lambda: fh.read(1 << 24), b""))


def cli_legs(cons, memb, record, length, memb_length, docs, work):
    """each pair alternates on the same index and window; the first round builds the sidecar caches (MEMO_CACHE=sync), the others read them"""
    out = os.path.join(work, "out")
    common = ("-k", str(k), "-n", str(docs))
    legs = [("conservation", cons, f"{record}:0-{length}", [("query", ()), ("regions", ()), (f"regions -t {docs}", ("-t", str(docs)))])]
    if memb:
        legs.append(("membership", memb, f"{record}:0-{memb_length}", [("query -m", ("-m",)), ("regions -m", ("-m",))]))
    for title, index, region, commands in legs:
        print(f"-- {title}, {region} of {os.path.basename(index)} ({os.path.getsize(index) / 1e6:.0f} MB)", flush=True)
        for rnd, mode in enumerate(["sync"] + ["read"] * a.repeats):
            env = dict(os.environ, MEMO_CACHE=mode)
            line = []
            for name, extra in commands:
                wall = run(env, name.split()[0], "-b", index, "-r", region, *common, "-o", out, *extra)
                size = os.path.getsize(out)
                lines = count_lines(out) if rnd == 0 and name.startswith("regions") else None
                line.append(f"memo {name}: {wall:.2f} s, {size / 1e6:.1f} MB" + (f", {lines} lines" if lines is not None else ""))
                os.unlink(out)
            print(f"   MEMO_CACHE={mode}: " + ";  ".join(line), flush=True)


if a.real:
    with tempfile.TemporaryDirectory(prefix="memo_regions_timing_") as work:
        import pyarrow as pa
        import pyarrow.parquet as pq
        z = np.load(os.path.join(a.real, "memb.npz"))
        docs, length = int(z["num_docs"]), int(z["length"])
        memb = os.path.join(work, "memb.parquet")
        pq.write_table(pa.table({"f0": pa.array(["chr1"] * len(z["start"]), pa.utf8()), "f1": z["start"], "f2": z["end"], "f3": z["annot"]}),
                       memb, compression="ZSTD", row_group_size=1 << 20)
        cons = os.path.join(work, "cons.parquet")
        os.symlink(os.path.abspath(os.path.join(a.real, "cons.parquet")), cons)
        print(f"== an index built from sequences: {docs} genomes, {length} positions", flush=True)
        cli_legs(cons, memb, "chr1", length, length, docs, work)
    sys.exit(0)

print(f"== synthetic pangenome: {n} genomes, {N} positions, k = {k}", flush=True)
device_legs()
if a.cli and not a.kernels_only:
    with tempfile.TemporaryDirectory(prefix="memo_regions_timing_") as work:
        pq_path = os.path.join(work, "synth.parquet")
        rows, t_pq = timed(lambda: synth.write_parquet(pq_path, n, N))
        print(f"-- bin/memo on a Parquet index of the same pangenome ({rows} rows, written in {t_pq:.0f} s)", flush=True)
        cli_legs(pq_path, pq_path, "chr1", N, M, n, work)
