#!/usr/bin/env python3
"""`memo index` end to end on a generated pangenome, per stage, against the suffix-automaton MS of tools/ms_sam.cpp.

    python tools/index_timing.py [--length 20000000] [--genomes 16] [--layout auto] [--out build/index_timing]

1. FASTA of a random pivot of --length bases and --genomes - 1 copies mutated as tools/realistic_index.py does
   (SNPs, short indels, inversions, translocations, a long deletion in every fifth genome);
2. `memo index` (memo_amd.build_index.build_index, conservation) on them: wall seconds per stage (FASTA reading and
   text building, matching statistics, DAP -> rows, Parquet write) and the device milliseconds of the MS stages from
   events (suffix arrays, LCP + hierarchy, walks; with --layout coded also the encode and decode passes, the device bytes
   held for the DAP and every genome's flagged positions);
3. tools/ms_sam.cpp (g++ -O2) on the same genomes with MS_THREADS = memo_host_threads();
4. the two MS matrices must be equal;
5. one JSON line.  Needs the GPU for step 2.  Development tool."""
import argparse
import ctypes as C
import importlib.util
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=20_000_000)
    ap.add_argument("--genomes", type=int, default=16, help="genomes in the pangenome, pivot included")
    ap.add_argument("--snp-lo", type=float, default=0.001)
    ap.add_argument("--snp-hi", type=float, default=0.01)
    ap.add_argument("--seed", type=int, default=20260)
    ap.add_argument("--chunk", type=int, default=0, help="pivot positions per MS walk thread (0: the library's)")
    ap.add_argument("--layout", default="auto", choices=["auto", "dense", "coded"], help="of the DAP on the device")
    ap.add_argument("--out", default="build/index_timing", help="working directory for the generated genomes (git-ignored)")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    spec = importlib.util.spec_from_file_location("realistic_index", os.path.join(ROOT, "tools", "realistic_index.py"))
    ri = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ri)

    t0 = time.perf_counter()
    rng = np.random.default_rng(a.seed)
    letters = np.frombuffer(b"ACGT", np.uint8)
    pivot = rng.integers(0, 4, a.length).astype(np.uint8)
    pivot.tofile(os.path.join(a.out, "pivot.bin"))
    fasta, bins = [], []

    def write_fasta(path, seq):
        with open(path, "wb") as fh:
            fh.write(b">chr1\n")
            body = letters[seq].tobytes()
            fh.write(b"\n".join(body[i:i + 80] for i in range(0, len(body), 80)) + b"\n")
        fasta.append(path)

    write_fasta(os.path.join(a.out, "pivot.fa"), pivot)
    for g in range(1, a.genomes):
        snp = float(np.exp(rng.uniform(np.log(a.snp_lo), np.log(a.snp_hi))))
        seq = ri.mutate(rng, pivot, snp, g)
        write_fasta(os.path.join(a.out, f"g{g}.fa"), seq)
        p = os.path.join(a.out, f"g{g}.bin")
        np.concatenate([seq, [4], ri.revcomp(seq), [4]]).astype(np.uint8).tofile(p)
        bins.append(p)
    lst = os.path.join(a.out, "genome_list.txt")
    with open(lst, "w") as fh:
        fh.write("".join(p + "\n" for p in fasta))
    gen_s = time.perf_counter() - t0

    import torch  # noqa: F401  (load order: torch's HIP runtime first, as bench.py and the tests do)
    from memo_amd import build_index
    from memo_amd._lib import lib
    lib()
    st = build_index.build_index(lst, a.out, "index", False, int(os.environ.get("MEMO_DEVICE", "0")), chunk=a.chunk,
                                 log=lambda s: None, keep_ms=True, layout=a.layout)
    ours = st.pop("ms")

    threads = C.c_int32()
    n_threads = lib().memo_host_threads(C.byref(threads), None)
    exe = os.path.join(a.out, "ms_sam")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", os.path.join(ROOT, "tools", "ms_sam.cpp"), "-o", exe])
    dap_path = os.path.join(a.out, "dap.i32")
    t1 = time.perf_counter()
    subprocess.check_call([exe, os.path.join(a.out, "pivot.bin"), dap_path] + bins,
                          env=dict(os.environ, MS_THREADS=str(n_threads)), stdout=subprocess.DEVNULL)
    sam_s = time.perf_counter() - t1
    sam = np.fromfile(dap_path, np.int32).reshape(a.length, a.genomes - 1)
    equal = bool(np.array_equal(ours, sam))
    out = {"length": a.length, "genomes": a.genomes, "chunk": a.chunk, "generate_s": round(gen_s, 2),
           "memo_index": {k: (round(v, 3) if isinstance(v, float) else v) for k, v in st.items()},
           "ms_sam": {"threads": n_threads, "seconds": round(sam_s, 3)},
           "ms_speedup_vs_ms_sam": round(sam_s / st["ms_s"], 2), "ms_equal": equal,
           "ms_mean": float(ours.mean()), "mismatches": int((ours != sam).sum())}
    for p in bins + [dap_path, exe]:
        os.unlink(p)
    print(json.dumps(out), flush=True)
    if not equal:
        sys.exit(1)


if __name__ == "__main__":
    main()
