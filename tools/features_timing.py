#!/usr/bin/env python3
"""What `memo features` costs and what it spares (GPU box; profiles/features_timing.txt).
  python tools/features_timing.py                     # a synthetic membership index of 100 genomes
In one process:
  1. memo_segment_conservation_dev alone on a resident conservation vector of 2^24 positions: the device time of its kernel from an
     event pair (memo_debug_features_times of the A/B library), the median of --repeats calls after --warm calls, with one segment,
     with segments of 10^4 and of 32 positions, and with segments of one position on 2^20 positions; the bytes read (2 L) over the
     kernel time;
  2. memo_feature_sums_dev alone: the three scan launches and the gather, on the table 10^4 features of 100 genomes give (100 rows,
     about 2 x 10^4 segments) and on the largest batch of a conservation index (2 rows, 2^20 + 1 segments, 2^19 features);
  3. end to end on a synthetic Parquet membership index (memo_amd/synth.py) written to a temporary directory: `bin/memo features -m`
     for --features random features of a record of --positions positions, as a process, and features.bed_features in this process;
     against the only route there was: one in-process tracks.region_tracks call (one bin) per feature, the record's sidecar cache
     warm, timed on --sample of the same features and scaled to all of them.  The sample's tables are compared.
The tables of 1 and 2 are compared with NumPy."""
import argparse
import ctypes as C
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from memo_amd import _lib, features, synth, tracks  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--resident", type=int, default=1 << 24)
ap.add_argument("--positions", type=int, default=10_000_000)
ap.add_argument("--features", type=int, default=10_000)
ap.add_argument("--sample", type=int, default=200)
ap.add_argument("--num-docs", type=int, default=100)
ap.add_argument("--warm", type=int, default=5)
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--no-end-to-end", action="store_true")
a = ap.parse_args()
n, k, M = a.num_docs, 31, a.resident
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


def device_ms(call):
    """(the three device times, host ms of the blocking call) of one timed call"""
    ms = (C.c_float * 3)()
    check(lib().memo_debug_features_times(1, None))
    _, wall = timed(call)
    check(lib().memo_debug_features_times(0, ms))
    return list(ms), wall * 1e3


class Dev:
    def __init__(self, host):
        self.host = np.ascontiguousarray(host)
        self.d = C.c_void_p()
        check(lib().memo_dev_malloc(0, max(self.host.nbytes, 16), C.byref(self.d)))
        self.upload()

    def upload(self):
        check(lib().memo_dev_upload(0, self.d, self.host.ctypes.data, self.host.nbytes, None))

    def download(self):
        out = np.empty_like(self.host)
        check(lib().memo_dev_download(0, out.ctypes.data, self.d, out.nbytes, None))
        return out

    def free(self):
        lib().memo_dev_free(0, self.d)


def segment_kernel():
    rng = np.random.default_rng(1)
    vec = Dev(rng.integers(0, n + 1, M).astype(np.uint16))
    cum = np.concatenate([[0], np.cumsum(vec.host, dtype=np.int64)])
    shared = np.concatenate([[0], np.cumsum(vec.host >= n, dtype=np.int64)])
    print(f"== memo_segment_conservation_dev: {M} positions, {2 * M / 1e6:.0f} MB of uint16 values, resident; the values over 8 TB/s: "
          f"{2 * M / 8e12 * 1e3:.3f} ms", flush=True)
    try:
        for what, L, width in (("one segment", M, M), ("segments of 10^4 positions", M, 10_000), ("segments of 32 positions", M, 32),
                               ("segments of one position", min(M, 1 << 20), 1)):
            edges = np.unique(np.concatenate([np.arange(0, L, width, dtype=np.int64), [L]]))
            segs = len(edges) - 1
            table = Dev(np.zeros((2, segs), np.uint64))

            def call():
                check(lib().memo_segment_conservation_dev(vec.d, L, 0, edges.ctypes.data, segs, n, table.d, 0, None))
            times = [device_ms(call) for _ in range(a.warm + a.repeats)][a.warm:]
            table.upload()
            call()
            got = table.download().astype(np.int64)
            assert np.array_equal(got[0], cum[edges[1:]] - cum[edges[:-1]]) and np.array_equal(got[1], shared[edges[1:]] - shared[edges[:-1]]), what
            dev = median([t[0][0] for t in times])
            print(f"1. {what} ({segs} segments, {L} positions): kernel {stats([t[0][0] for t in times])}; blocking call on the host clock "
                  f"{stats([t[1] for t in times])}; {2 * L / dev / 1e9:.3f} TB/s", flush=True)
            table.free()
        print("   the four tables equal NumPy's", flush=True)
    finally:
        vec.free()


def sums_kernels():
    rng = np.random.default_rng(2)
    for what, rows, segs, count in ((f"the table of 10^4 features of {n} genomes", n, 20_001, 10_000), ("the largest conservation batch", 2, (1 << 20) + 1, 1 << 19)):
        host = rng.integers(0, 1 << 40, (rows, segs)).astype(np.uint64)
        lo = rng.integers(0, segs + 1, count)
        hi = np.minimum(lo + rng.integers(0, 64, count), segs)
        lo, hi = lo.astype(np.int32), hi.astype(np.int32)
        table, out = Dev(host), Dev(np.zeros((count, rows), np.uint64))

        def call():
            check(lib().memo_feature_sums_dev(table.d, rows, segs, lo.ctypes.data, hi.ctypes.data, count, out.d, 0, None))
        times = []
        for _ in range(a.warm + a.repeats):
            table.upload()
            times.append(device_ms(call))
        times = times[a.warm:]
        cum = np.concatenate([np.zeros((rows, 1), np.uint64), np.cumsum(host, axis=1, dtype=np.uint64)], axis=1)
        assert np.array_equal(out.download(), (cum[:, hi] - cum[:, lo]).T), what
        print(f"2. memo_feature_sums_dev, {what} ({rows} rows, {segs} segments, {count} features): the three scan launches "
              f"{stats([t[0][1] for t in times])}; the gather {stats([t[0][2] for t in times])}; blocking call on the host clock "
              f"{stats([t[1] for t in times])}", flush=True)
        table.free()
        out.free()
    print("   both tables equal numpy.cumsum's differences", flush=True)


def end_to_end():
    L, F = a.positions, a.features
    tmp = tempfile.mkdtemp(prefix="memo_features_timing_")
    try:
        path, bed_path, out = os.path.join(tmp, "synth_memb.parquet"), os.path.join(tmp, "features.bed"), os.path.join(tmp, "features.tsv")
        rows, t = timed(lambda: synth.write_parquet(path, n, L + k + 1))
        rng = np.random.default_rng(3)
        starts = rng.integers(0, L - 20_000, F)
        ends = starts + rng.integers(100, 20_000, F)
        with open(bed_path, "w") as fh:
            fh.write("".join(f"chr1\t{s}\t{e}\tf{i}\n" for i, (s, e) in enumerate(zip(starts.tolist(), ends.tolist()))))
        print(f"== end to end: a synthetic membership index of {n} genomes, {rows} rows, {os.path.getsize(path) / 1e6:.0f} MB of Parquet (written in "
              f"{t:.1f} s); {F} random features of 100 to 20000 positions on chr1:0-{L}, k = {k}", flush=True)
        exe = [sys.executable, os.path.join(ROOT, "bin", "memo")]
        # the record's sidecar cache: `memo query` builds it after its answer
        subprocess.run(exe + ["query", "-m", "-b", path, "-k", str(k), "-n", str(n), "-r", "chr1:0-10", "-o", os.path.join(tmp, "q.txt")],
                       check=True, stdout=subprocess.DEVNULL)
        bed = features.read_bed(bed_path)
        for turn in ("first", "second"):
            _, t_cli = timed(lambda: subprocess.run(exe + ["features", "-m", "-b", path, "-k", str(k), "-n", str(n), "-a", bed_path, "-o", out],
                                                    check=True, stdout=subprocess.DEVNULL))
            (table, positions), t_new = timed(lambda: features.bed_features(path, bed, k, n, membership=True))
            print(f"3. {turn} turn: `memo features -m` as a process {t_cli * 1e3:.0f} ms; features.bed_features in this process {t_new * 1e3:.0f} ms", flush=True)
        assert open(out).read() == features.format_features(bed, positions, table, True)
        sample = rng.choice(F, min(a.sample, F), replace=False)

        def one_by_one():
            return [tracks.region_tracks(path, f"chr1:{starts[f]}-{ends[f]}", k, n, 1)[0][:, 0] for f in sample.tolist()]
        one_by_one()                                          # (warm: the code objects, the cache's pages)
        got, t_old = timed(one_by_one)
        assert np.array_equal(np.array(got), table[sample]), "bed_features and region_tracks differ"
        scaled = t_old / len(sample) * F
        print(f"   one tracks.region_tracks call per feature, the record's cache warm: {t_old * 1e3:.0f} ms for {len(sample)} of the features, "
              f"{t_old / len(sample) * 1e3:.2f} ms a feature, {scaled:.1f} s scaled to {F}; ratio to bed_features {scaled / t_new:.0f}, to the "
              f"process {scaled / t_cli:.0f}; the sample's tables are equal", flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


print(f"one session on one MI355X; {lib().memo_version().decode()}", flush=True)
segment_kernel()
sums_kernels()
if not a.no_end_to_end:
    end_to_end()
