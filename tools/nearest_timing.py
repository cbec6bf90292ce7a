#!/usr/bin/env python3
"""What `memo nearest` costs beside the kernels that read the same planes once (GPU box; profiles/nearest_timing.txt).
  python tools/nearest_timing.py                       # planes of 100 genomes x 5.4e6 positions
In one process:
  1. memo_nearest_dev alone on resident planes (uint32 [N][pitch], the layout memo_lengths_finish_dev leaves: falling ramps between
     random breaks, a mean match of --mean-match positions, every plane its own) into 500 bins: the device time of its kernel from an
     event pair (memo_debug_nearest_times of the A/B library), the median of --repeats calls after --warm calls that also ramp the
     clocks, the host clock around the whole blocking call, and the bytes read over the kernel time -- with 72 KiB of LDS a
     workgroup (the product's: two workgroups a CU, a tile of 128 positions at 100 planes) and with 120 KiB (one a CU, 256
     positions), alternating (memo_debug_nearest_lds); then the tables alone, the winner alone and all three outputs;
  2. memo_lengths_select_dev at T = 2 and memo_breaks_dev into the same 500 bins on the same buffer, alternating with 1: the parent
     commit's two kernels that read the same bytes once;
  3. memo_nearest_dev into 2^20 bins (five positions a bin): the narrow-bin walk, the runs of a tile with their own atomics;
  4. end to end on a synthetic Parquet membership index (memo_amd/synth.py) written to a temporary directory, a window of --positions
     positions: nearest.region_nearest and nearest.region_winners against lengths.region_planes + NumPy on the host.  The tables
     are compared.
The tables and the winner of 1 and 3 are compared with NumPy on the first --check positions."""
import argparse
import ctypes as C
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from memo_amd import _lib, lengths, nearest, synth, view  # noqa: E402
from memo_amd._device import DevBuffer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--resident", type=int, default=5_400_000)
ap.add_argument("--num-docs", type=int, default=100)
ap.add_argument("--mean-match", type=int, default=100)
ap.add_argument("--bins", type=int, default=500)
ap.add_argument("--check", type=int, default=300_000)
ap.add_argument("--positions", type=int, default=10_000_000)
ap.add_argument("--e2e-docs", type=int, default=20)
ap.add_argument("--warm", type=int, default=5)
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--no-end-to-end", action="store_true")
ap.add_argument("--only-end-to-end", action="store_true")
a = ap.parse_args()
CAP = 2 ** 31 - 1
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


def ramps(rng, L, mean):
    """match lengths as an index leaves them: from every break a length that falls by one a position until the next break"""
    at = np.flatnonzero(rng.random(L) < 1.0 / mean)
    at = np.concatenate([[0], at[at > 0], [L]])
    reach = at[1:] + rng.integers(0, mean, len(at) - 1)             # where the match that starts at a break ends
    return (np.repeat(reach, np.diff(at)) - np.arange(L)).astype(np.uint32)


def host_tables(v, edges, min_len=1):
    """NumPy on planes [N, L] (plane 0 the pivot's): (wins [2, N, B], sums [B], winner [L]); no bin is empty"""
    c = v[1:].astype(np.int64)
    best = c.max(axis=0)
    ok = best >= min_len
    att = (c == best[None, :]) & ok[None, :]
    sole = att & (att.sum(axis=0) == 1)[None, :]
    cut = np.asarray(edges, np.int64)[:-1]
    wins = np.zeros((2, len(v), len(cut)), np.uint64)
    wins[0, 1:], wins[1, 1:] = np.add.reduceat(att, cut, axis=1, dtype=np.int64), np.add.reduceat(sole, cut, axis=1, dtype=np.int64)
    wins[:, 0] = np.add.reduceat(~ok, cut, dtype=np.int64)
    return wins, np.add.reduceat(best, cut).astype(np.uint64), np.where(ok, att.argmax(axis=0) + 1, 0).astype(np.uint16)


def nearest_call(d_cells, L, pitch, planes, edges, d_wins, d_sums, d_winner, kib=72):
    """(device ms of the kernel, host ms of the blocking call) of one call"""
    ms = (C.c_float * 1)()
    check(lib().memo_debug_nearest_lds(kib))
    check(lib().memo_debug_nearest_times(1, None))
    tables = d_wins is not None or d_sums is not None
    _, wall = timed(lambda: check(lib().memo_nearest_dev(d_cells, L, pitch, planes, CAP, 1, None, 0, edges.ctypes.data if tables else None,
                                                         len(edges) - 1 if tables else 0, d_wins, d_sums, d_winner, 0, None)))
    check(lib().memo_debug_nearest_times(0, ms))
    check(lib().memo_debug_nearest_lds(0))
    return ms[0], wall * 1e3


def select_call(d_cells, L, pitch, planes, d_out):
    ms = (C.c_float * 7)()
    check(lib().memo_debug_lengths_times(1, None))
    _, wall = timed(lambda: check(lib().memo_lengths_select_dev(d_cells, L, pitch, planes, CAP, 2, d_out, 0, None)))
    check(lib().memo_debug_lengths_times(0, ms))
    return ms[6], wall * 1e3


def breaks_call(d_cells, L, pitch, planes, edges, d_table):
    ms = (C.c_float * 1)()
    check(lib().memo_debug_breaks_times(1, None))
    _, wall = timed(lambda: check(lib().memo_breaks_dev(d_cells, L, pitch, planes, CAP, 1, 0, 0, edges.ctypes.data, len(edges) - 1, d_table, 0, None)))
    check(lib().memo_debug_breaks_times(0, ms))
    return ms[0], wall * 1e3


def zero(buf, nbytes):
    z = np.zeros(nbytes // 8, np.uint64)
    check(lib().memo_dev_upload(0, buf.d, z.ctypes.data, z.nbytes, None))


def rows_of(buf, offset, shape, dtype):
    out = np.empty(shape, dtype)
    check(lib().memo_dev_download(0, out.ctypes.data, buf.at(offset), out.nbytes, None))
    return out


def resident():
    n, L = a.num_docs, a.resident
    pitch = lengths.pitch_of(L)
    nbytes = 4 * n * pitch
    read = 4 * (n - 1) * L                                           # (the pivot's plane is not read)
    print(f"== {n} planes of {L} positions, a mean match of {a.mean_match}: {nbytes / 1e6:.0f} MB of finished lengths, resident; "
          f"memo_nearest_dev reads the {n - 1} candidate planes, {read / 1e6:.0f} MB", flush=True)
    rng = np.random.default_rng(1)
    base = ramps(rng, pitch + 4096 * n, a.mean_match)
    host = np.empty((n, pitch), np.uint32)
    for g in range(n):
        host[g] = base[4096 * g:4096 * g + pitch]                    # (every plane its own cut of one long ramp train)
    many = 1 << 20
    m = min(a.check, L)
    with DevBuffer.of(host, 0) as cells, DevBuffer(0, 16 * n * many) as d_wins, DevBuffer(0, 8 * many) as d_sums, DevBuffer(0, 2 * pitch) as d_winner, \
            DevBuffer(0, 4 * pitch) as d_sel, DevBuffer(0, 16 * n * a.bins) as d_breaks:
        floor_ms = read / 8e12 * 1e3
        print(f"the candidate cells over 8 TB/s: {floor_ms:.3f} ms; tile {nearest.tile(n)} positions at the product's 72 KiB of LDS", flush=True)
        wide = view.bin_edges(L, a.bins)
        narrow = view.bin_edges(L, many)
        # the results against NumPy on the first positions, at both LDS sizes
        for kib in (72, 120):
            for edges in (wide, narrow):
                bins = len(edges) - 1
                zero(d_wins, 16 * n * bins), zero(d_sums, 8 * bins)
                nearest_call(cells.d, L, pitch, n, edges, d_wins.d, d_sums.d, d_winner.d, kib)
                whole = int(np.searchsorted(edges, m, "right")) - 1  # the bins that end at or before m
                want = host_tables(host[:, :int(edges[whole])], edges[:whole + 1])
                for which in range(2):
                    for g in sorted({0, 1, n // 2, n - 1}):
                        got = rows_of(d_wins, 8 * ((which * n + g) * bins), whole, np.uint64)
                        assert np.array_equal(got, want[0][which, g]), f"wins[{which}][{g}] of {bins} bins at {kib} KiB differs from NumPy's"
                assert np.array_equal(rows_of(d_sums, 0, whole, np.uint64), want[1]), f"the sums of {bins} bins differ"
                assert np.array_equal(rows_of(d_winner, 0, int(edges[whole]), np.uint16), want[2]), "the winner differs"
        print(f"   the tables of {a.bins} and 2^20 bins and the winner equal NumPy's on the first {m} positions, at 72 and at 120 KiB", flush=True)
        t = {k: [] for k in ("72", "120", "select", "breaks")}
        for i in range(a.warm + a.repeats):                          # alternating: the same clocks, the same neighbours
            got = {"72": nearest_call(cells.d, L, pitch, n, wide, d_wins.d, d_sums.d, None, 72),
                   "120": nearest_call(cells.d, L, pitch, n, wide, d_wins.d, d_sums.d, None, 120),
                   "select": select_call(cells.d, L, pitch, n, d_sel.d), "breaks": breaks_call(cells.d, L, pitch, n, wide, d_breaks.d)}
            if i >= a.warm:
                for k in t:
                    t[k].append(got[k])
        dev = {k: median([d for d, _ in t[k]]) for k in t}
        for k, what in (("72", "72 KiB of LDS, two workgroups a CU (the product's)"), ("120", "120 KiB, one a CU, a tile twice as long")):
            print(f"1. memo_nearest_dev, wins + sums into {a.bins} bins, {what}: kernel {stats([d for d, _ in t[k]])}; blocking call on the host clock "
                  f"{stats([w for _, w in t[k]])}", flush=True)
            print(f"   {read / 1e6:.0f} MB read over the kernel's median: {read / dev[k] / 1e9:.2f} TB/s, {dev[k] / floor_ms:.1f} x the 8 TB/s time", flush=True)
        print(f"2. alternating with 1 on the same buffer: memo_lengths_select_dev, T = 2: kernel {stats([d for d, _ in t['select']])} "
              f"({4 * n * L / dev['select'] / 1e9:.2f} TB/s of {4 * n * L / 1e6:.0f} MB); memo_breaks_dev, {a.bins} bins: kernel {stats([d for d, _ in t['breaks']])}",
              flush=True)
        print(f"   nearest over select: {dev['72'] / dev['select']:.2f} x; over breaks: {dev['72'] / dev['breaks']:.2f} x; "
              f"nearest at 120 KiB over nearest at 72 KiB: {dev['120'] / dev['72']:.2f} x", flush=True)
        parts = {}
        for name, args in (("wins alone", (d_wins.d, None, None)), ("sums alone", (None, d_sums.d, None)), ("the winner alone", (None, None, d_winner.d)),
                           ("all three", (d_wins.d, d_sums.d, d_winner.d))):
            parts[name] = median([nearest_call(cells.d, L, pitch, n, wide, *args)[0] for _ in range(a.warm + a.repeats)][a.warm:])
        print("   by output, kernel medians: " + ", ".join(f"{k} {v:.3f} ms" for k, v in parts.items())
              + " (the winner alone is stage + phase A; wins adds phase B)", flush=True)
        t_narrow = {"72": [], "120": []}
        for i in range(a.warm + a.repeats):
            got = {"72": nearest_call(cells.d, L, pitch, n, narrow, d_wins.d, d_sums.d, None, 72), "120": nearest_call(cells.d, L, pitch, n, narrow, d_wins.d, d_sums.d, None, 120)}
            if i >= a.warm:
                for k in got:
                    t_narrow[k].append(got[k])
        for k in t_narrow:
            nar = median([d for d, _ in t_narrow[k]])
            print(f"3. memo_nearest_dev, wins + sums into 2^20 bins of {L / many:.1f} positions, {k} KiB: kernel {stats([d for d, _ in t_narrow[k]])}; blocking call "
                  f"{stats([w for _, w in t_narrow[k]])} (8 MiB of edges uploaded per call); {read / nar / 1e9:.3f} TB/s, {nar / floor_ms:.1f} x the 8 TB/s time", flush=True)


def end_to_end():
    n, L, k = a.e2e_docs, a.positions, 31
    tmp = tempfile.mkdtemp(prefix="memo_nearest_timing_")
    try:
        path = os.path.join(tmp, "synth_memb.parquet")
        rows, t = timed(lambda: synth.write_parquet(path, n, L + k + 1))
        print(f"== end to end: a synthetic index of {n} genomes, {rows} rows, {os.path.getsize(path) / 1e6:.0f} MB of Parquet (written in {t:.1f} s); "
              f"window chr1:0-{L}, {a.bins} bins", flush=True)
        region = f"chr1:0-{L}"
        for turn in ("first", "second"):
            (wins, sums, edges, qs), t_new = timed(lambda: nearest.region_nearest(path, region, n, a.bins))
            (starts, winners, _, _), t_runs = timed(lambda: nearest.region_winners(path, region, n))

            def by_planes():
                planes = lengths.region_planes(path, region, n)
                out = [np.zeros((2, n, a.bins), np.uint64), np.zeros(a.bins, np.uint64), []]
                for b in range(a.bins):                              # bin by bin: the boolean planes of the whole window would not fit a cache
                    w, s, win = host_tables(planes[:, edges[b]:edges[b + 1]], [0, edges[b + 1] - edges[b]])
                    out[0][:, :, b], out[1][b] = w[:, :, 0], s[0]
                    out[2].append(win)
                return out[0], out[1], np.concatenate(out[2])
            (h_wins, h_sums, h_winner), t_host = timed(by_planes)
            assert np.array_equal(wins, h_wins) and np.array_equal(sums, h_sums), "region_nearest and NumPy on region_planes differ"
            at = np.concatenate([[0], np.flatnonzero(h_winner[1:] != h_winner[:-1]) + 1])
            assert np.array_equal(starts, at) and np.array_equal(winners, h_winner[at]), "region_winners and NumPy on region_planes differ"
            print(f"4. {turn} turn: nearest.region_nearest {t_new * 1e3:.0f} ms; nearest.region_winners {t_runs * 1e3:.0f} ms ({len(starts)} runs); "
                  f"lengths.region_planes + NumPy argmax of {4 * n * L / 1e6:.0f} MB {t_host * 1e3:.0f} ms (ratio {t_host / t_new:.1f}); the tables and the runs are equal",
                  flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


print(f"one session on one MI355X; {lib().memo_version().decode()}", flush=True)
if not a.only_end_to_end:
    resident()
if not a.no_end_to_end:
    end_to_end()
