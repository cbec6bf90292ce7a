#!/usr/bin/env python3
"""What reading a conservation text costs `memo view`, and what not writing it saves (GPU box; profiles/view_timing.txt).
  python tools/view_timing.py --lines 10000000 --cli      # + `memo view` from the text against `memo view -r` from a Parquet index
  python tools/view_timing.py --lines 100000000
The text is a conservation result of the synthetic pangenome (100 genomes, k = 31), emitted as `memo query` writes it; it was
just written, so every reader finds it in the page cache."""
import argparse
import ctypes as C
import mmap
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import memo_amd  # noqa: E402
from memo_amd import synth, view  # noqa: E402
from memo_amd._lib import check, lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--lines", type=int, default=10_000_000)
ap.add_argument("--num-docs", type=int, default=100)
ap.add_argument("--bins", type=int, default=500)
ap.add_argument("--cli", action="store_true", help="also time bin/memo view on the text and on a Parquet index of the same window")
a = ap.parse_args()
N, n, k = a.lines, a.num_docs, 31


def timed(fn):
    t = time.perf_counter()
    r = fn()
    return r, time.perf_counter() - t


with tempfile.TemporaryDirectory(prefix="memo_view_timing_") as work:
    text = os.path.join(work, "cons.txt")
    ix, _ = synth.device_index(0, N, k, n, N)
    with ix:
        vec = ix.conservation(0, N, k, n)
    with open(text, "wb") as fh:
        fh.write(memoryview(memo_amd.index.emit_conservation_buffer(vec)))
    nbytes = os.path.getsize(text)
    print(f"== {N} lines, {nbytes / 1e6:.0f} MB of text ({n} genomes, k = {k})", flush=True)

    host, t_host = timed(lambda: view.read_conservation_text(text))
    assert np.array_equal(host, vec)
    print(f"view.read_conservation_text (np.loadtxt, one core; unchanged since the parent commit): {t_host:.2f} s", flush=True)

    for attempt in ("first call (sets the pinned ring up)", "second call"):
        (d_vec, L, free), t_dev = timed(lambda: view.read_conservation_text_dev(text))
        got = np.empty(L, np.uint16)
        check(lib().memo_dev_download(0, got.ctypes.data, C.c_void_p(d_vec), got.nbytes, None))
        free()
        assert L == N and np.array_equal(got, vec)
        print(f"view.read_conservation_text_dev, {attempt}: {t_dev:.3f} s  ({t_host / t_dev:.0f} x)", flush=True)

    # the same steps apart: file read + copy to the device; the three kernels (one call: its scratch allocation and two waits included)
    d_text, d_out = C.c_void_p(), C.c_void_p()
    check(lib().memo_dev_malloc(0, nbytes, C.byref(d_text)))
    check(lib().memo_dev_malloc(0, 2 * (nbytes // 2 + 1), C.byref(d_out)))
    with open(text, "rb") as fh, mmap.mmap(fh.fileno(), nbytes, access=mmap.ACCESS_READ) as mm:
        buf = np.frombuffer(mm, np.uint8)
        _, t_copy = timed(lambda: check(lib().memo_dev_upload_pipelined(0, d_text, buf.ctypes.data, nbytes)))
        del buf
    lines, odd = C.c_int64(), C.c_int64()
    for attempt in range(3):
        _, t_parse = timed(lambda: check(lib().memo_parse_conservation_text_dev(d_text, nbytes, d_out, nbytes // 2 + 1, C.byref(lines),
                                                                                C.byref(odd), 0, None)))
        print(f"    memo_parse_conservation_text_dev, call {attempt + 1}: {t_parse * 1e3:.2f} ms "
              f"({2 * nbytes / t_parse / 1e9:.0f} GB/s of text read twice)", flush=True)
    assert (lines.value, odd.value) == (N, -1)
    print(f"    mmap + memo_dev_upload_pipelined: {t_copy * 1e3:.1f} ms ({nbytes / t_copy / 1e9:.1f} GB/s)", flush=True)
    (counts, _), t_bin = timed(lambda: view.bin_counts((d_out.value, N), n, a.bins))
    print(f"    memo_bin_conservation_dev ({a.bins} bins): {t_bin * 1e3:.2f} ms", flush=True)
    lib().memo_dev_free(0, d_text)
    lib().memo_dev_free(0, d_out)

    if a.cli:
        exe = os.path.join(ROOT, "bin", "memo")
        pq_path = os.path.join(work, "synth.parquet")
        rows, t_pq = timed(lambda: synth.write_parquet(pq_path, n, N))
        print(f"-- bin/memo on a Parquet index of the same window ({rows} rows, {os.path.getsize(pq_path) / 1e6:.0f} MB; MEMO_CACHE=0)", flush=True)
        env = dict(os.environ, MEMO_CACHE="0")
        region = f"chr1:0-{N}"
        out, t1, t2 = (os.path.join(work, f) for f in ("out.txt", "from_text.tsv", "from_index.tsv"))

        def run(*argv):
            r, wall = timed(lambda: subprocess.run([sys.executable, exe, *argv], capture_output=True, env=env))
            assert r.returncode == 0, r.stderr.decode()[-400:]
            return wall
        w_query = run("query", "-b", pq_path, "-k", str(k), "-n", str(n), "-r", region, "-o", out)
        w_text = run("view", "-i", out, "-n", str(n), "-b", str(a.bins), "-o", t1)
        w_index = run("view", "-i", pq_path, "-r", region, "-k", str(k), "-n", str(n), "-b", str(a.bins), "-o", t2)
        assert open(t1, "rb").read() == open(t2, "rb").read() and open(out, "rb").read() == open(text, "rb").read()
        print(f"memo query -o out.txt: {w_query:.2f} s;  memo view -i out.txt -o t.tsv: {w_text:.2f} s;  together {w_query + w_text:.2f} s")
        print(f"memo view -i index.parquet -r {region} -o t.tsv: {w_index:.2f} s  (the same table, byte for byte)", flush=True)
