#!/usr/bin/env python3
"""What `memo tracks` costs and what it spares (GPU box; profiles/tracks_timing.txt).
  python tools/tracks_timing.py                       # a synthetic membership result of 100 genomes (W = 4)
In one process:
  1. memo_tracks_dev alone on a resident result of 2^24 positions with 500 bins: the device time of its kernel from an event pair
     (memo_debug_tracks_times of the A/B library), the median of --repeats calls after --warm calls that also ramp the clocks, the
     host clock around the whole blocking call (with the upload of the edges), and the bytes read (L x W x 4) over the kernel time;
  2. memo_cooccurrence_dev on the same buffer, alternating with 1 (memo_debug_cooc_times: sweep + reduce): what the parent commit
     already does to those rows, N^2 / 2 pair counts a position against N counts;
  3. memo_tracks_dev with 2^20 bins (16 positions a bin) on the same buffer: bins narrower than a plane word, and one atomic per
     genome and bin that holds a bit; and with one bin per position on --narrow-positions positions;
  4. end to end on a synthetic Parquet index (memo_amd/synth.py) written to a temporary directory: tracks.region_tracks on a window
     of --positions positions against `memo query -m` of the same window followed by a NumPy reduction of its text (the bytes of
     the file as a [L, 2 N] matrix of characters, every other column, np.add.reduceat over the same edges); both routes read the same Parquet file and
     both are timed a second time, when the sidecar cache of the record exists.  The tables are compared.
The tables of 1 and 3 are compared with NumPy on the downloaded rows."""
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
from memo_amd import _lib, synth, tracks, view  # noqa: E402
from memo_amd.index import words  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--resident", type=int, default=1 << 24)
ap.add_argument("--positions", type=int, default=10_000_000)
ap.add_argument("--narrow-positions", type=int, default=1 << 20)
ap.add_argument("--num-docs", type=int, default=100)
ap.add_argument("--bins", type=int, default=500)
ap.add_argument("--warm", type=int, default=5)
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--no-end-to-end", action="store_true")
a = ap.parse_args()
n, k, M = a.num_docs, 31, a.resident
W = words(n)
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


def tracks_call(d_bits, L, edges, d_counts):
    """(device ms of the kernel, host ms of the blocking call) of one call"""
    ms = (C.c_float * 1)()
    check(lib().memo_debug_tracks_times(1, None))
    _, wall = timed(lambda: check(lib().memo_tracks_dev(d_bits, L, n, 0, edges.ctypes.data, len(edges) - 1, d_counts, 0, None)))
    check(lib().memo_debug_tracks_times(0, ms))
    return ms[0], wall * 1e3


def cooc_call(d_bits, L, d_matrix):
    ms = (C.c_float * 2)()
    check(lib().memo_debug_cooc_times(1, None))
    _, wall = timed(lambda: check(lib().memo_cooccurrence_dev(d_bits, L, n, d_matrix, 0, None)))
    check(lib().memo_debug_cooc_times(0, ms))
    return ms[0] + ms[1], wall * 1e3


def host_table(rows, edges):
    """NumPy on host rows uint32 [L, W]: the counts of every genome and bin, in chunks of whole bins"""
    out = np.zeros((n, len(edges) - 1), np.int64)
    step = max(1, (len(edges) - 1) // 64)
    for b0 in range(0, len(edges) - 1, step):
        b1 = min(b0 + step, len(edges) - 1)
        lo, hi = int(edges[b0]), int(edges[b1])
        B = np.unpackbits(rows[lo:hi].view(np.uint8), axis=1, bitorder="little")[:, :n]
        out[:, b0:b1] = np.add.reduceat(B, edges[b0:b1] - lo, axis=0, dtype=np.int64).T          # (no bin is empty: bins <= positions)
    return out


def table_of(d_bits, L, edges, d_counts):
    zero = np.zeros((n, len(edges) - 1), np.uint64)
    check(lib().memo_dev_upload(0, d_counts, zero.ctypes.data, zero.nbytes, None))
    t = tracks_call(d_bits, L, edges, d_counts)
    got = np.empty_like(zero)
    check(lib().memo_dev_download(0, got.ctypes.data, d_counts, got.nbytes, None))
    return got, t


def resident():
    nbytes = 4 * W * M
    print(f"== {n} genomes (W = {W}), {M} positions, k = {k}: {nbytes / 1e6:.0f} MB of membership rows, resident", flush=True)
    ix, _ = synth.device_index(0, M, k, n, 2 * M, pack="keep")
    d_bits, d_counts, d_matrix = C.c_void_p(), C.c_void_p(), C.c_void_p()
    check(lib().memo_dev_malloc(0, nbytes, C.byref(d_bits)))
    check(lib().memo_dev_malloc(0, 8 * n * (1 << 20), C.byref(d_counts)))
    check(lib().memo_dev_malloc(0, 8 * n * n, C.byref(d_matrix)))
    try:
        with ix:
            ix.membership_dev(0, M, k, n, d_bits.value)
            ix.check()
        host = np.empty((M, W), np.uint32)
        check(lib().memo_dev_download(0, host.ctypes.data, d_bits, nbytes, None))
        print(f"present bits: {np.unpackbits(host[:1 << 20].view(np.uint8)).mean() * 32 * W / n:.3f} of all (first 2^20 positions)", flush=True)
        floor_ms = nbytes / 8e12 * 1e3
        print(f"the rows over 8 TB/s: {floor_ms:.3f} ms", flush=True)
        wide, narrow = view.bin_edges(M, a.bins), view.bin_edges(M, 1 << 20)
        zero = np.zeros((n, n), np.uint64)
        check(lib().memo_dev_upload(0, d_matrix, zero.ctypes.data, zero.nbytes, None))
        got, _ = table_of(d_bits, M, wide, d_counts)
        assert np.array_equal(got.astype(np.int64), host_table(host, wide)), "the table of 500 bins differs from NumPy's"
        t_tracks, t_cooc = [], []
        for i in range(a.warm + a.repeats):                  # alternating: the same clocks, the same neighbours
            t, c = tracks_call(d_bits, M, wide, d_counts), cooc_call(d_bits, M, d_matrix)
            if i >= a.warm:
                t_tracks.append(t)
                t_cooc.append(c)
        dev = median([d for d, _ in t_tracks])
        print(f"1. memo_tracks_dev, {a.bins} bins: kernel {stats([d for d, _ in t_tracks])}; blocking call on the host clock "
              f"{stats([w for _, w in t_tracks])}", flush=True)
        print(f"   {nbytes / 1e6:.0f} MB read over the kernel's median: {nbytes / dev / 1e9:.2f} TB/s, {dev / floor_ms:.1f} x the 8 TB/s time", flush=True)
        cooc = median([d for d, _ in t_cooc])
        print(f"2. memo_cooccurrence_dev on the same buffer (the parent commit's reduction of these rows), alternating with 1: sweep + reduce "
              f"{stats([d for d, _ in t_cooc])}; blocking call {stats([w for _, w in t_cooc])}", flush=True)
        print(f"   tracks over cooccurrence: {dev / cooc:.2f} x", flush=True)
        got, _ = table_of(d_bits, M, narrow, d_counts)
        assert np.array_equal(got.astype(np.int64), host_table(host, narrow)), "the table of 2^20 bins differs from NumPy's"
        t_narrow = [tracks_call(d_bits, M, narrow, d_counts) for _ in range(a.warm + a.repeats)][a.warm:]
        nar = median([d for d, _ in t_narrow])
        print(f"3. memo_tracks_dev, 2^20 bins of {M >> 20} positions: kernel {stats([d for d, _ in t_narrow])}; blocking call "
              f"{stats([w for _, w in t_narrow])} (8 MiB of edges uploaded per call)", flush=True)
        print(f"   {nar / dev:.1f} x the kernel of {a.bins} bins; {nbytes / nar / 1e9:.3f} TB/s; cells that hold a bit, one atomic each: "
              f"{int((got != 0).sum())} of {got.size}", flush=True)
        P = min(a.narrow_positions, 1 << 20, M)
        single = np.arange(P + 1, dtype=np.int64)
        got, _ = table_of(d_bits, P, single, d_counts)
        assert np.array_equal(got.astype(np.int64), np.unpackbits(host[:P].view(np.uint8), axis=1, bitorder="little")[:, :n].T), "one bin a position"
        t_single = [tracks_call(d_bits, P, single, d_counts) for _ in range(a.warm + a.repeats)][a.warm:]
        print(f"   one bin per position on {P} positions: kernel {stats([d for d, _ in t_single])} "
              f"({4 * W * P / median([d for d, _ in t_single]) / 1e9:.3f} TB/s)", flush=True)
        print("   the three tables equal NumPy's on the downloaded rows", flush=True)
    finally:
        for d in (d_bits, d_counts, d_matrix):
            lib().memo_dev_free(0, d)


def end_to_end():
    L = a.positions
    tmp = tempfile.mkdtemp(prefix="memo_tracks_timing_")
    try:
        path, out = os.path.join(tmp, "synth_memb.parquet"), os.path.join(tmp, "query.txt")
        rows, t = timed(lambda: synth.write_parquet(path, n, L + k + 1))
        print(f"== end to end: a synthetic index of {n} genomes, {rows} rows, {os.path.getsize(path) / 1e6:.0f} MB of Parquet (written in {t:.1f} s); "
              f"window chr1:0-{L}, k = {k}, {a.bins} bins", flush=True)
        region = f"chr1:0-{L}"
        exe = [sys.executable, os.path.join(ROOT, "bin", "memo")]
        for turn in ("first", "second (the record's sidecar cache exists)"):
            (counts, edges), t_new = timed(lambda: tracks.region_tracks(path, region, k, n, a.bins))
            _, t_query = timed(lambda: subprocess.run(exe + ["query", "-m", "-b", path, "-k", str(k), "-n", str(n), "-r", region, "-o", out],
                                                      check=True, stdout=subprocess.DEVNULL))

            def reduce_text():
                text = np.fromfile(out, np.uint8)
                assert len(text) == L * 2 * n, (len(text), L, n)           # N characters '0' / '1', a ' ' or the '\n' behind each
                B = text.reshape(L, 2 * n)[:, 0::2]
                return (np.add.reduceat(B, edges[:-1], axis=0, dtype=np.int64) - 48 * np.diff(edges)[:, None]).T
            want, t_host = timed(reduce_text)
            assert np.array_equal(counts.astype(np.int64), want), "region_tracks and the text route differ"
            print(f"4. {turn} turn: tracks.region_tracks {t_new * 1e3:.0f} ms; `memo query -m` {t_query * 1e3:.0f} ms + NumPy on its "
                  f"{os.path.getsize(out) / 1e9:.2f} GB of text {t_host * 1e3:.0f} ms = {(t_query + t_host) * 1e3:.0f} ms; "
                  f"ratio {(t_query + t_host) / t_new:.1f}; the tables are equal", flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


print(f"one session on one MI355X; {lib().memo_version().decode()}", flush=True)
resident()
if not a.no_end_to_end:
    end_to_end()
