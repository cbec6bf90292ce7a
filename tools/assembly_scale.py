#!/usr/bin/env python3
"""`memo index` at whole-assembly scale: a pivot region against genomes of human-assembly size, whose texts pass 2^31 bytes.

    python tools/assembly_scale.py [--genomes 2] [--scale 1.0] [--pivot-length 5000000] [--piece-bytes 0] [--check 1]
                                   [--out build/assembly_scale]

1. a random pivot of --pivot-length bases (one record) and --genomes genomes of 24 records sized like the human chromosomes
   (GRCh38 1-22, X, Y; times --scale): random sequence with mutated copies of the pivot planted forward and reverse-
   complemented, written as FASTA under --out (one line per record).  When the disk lacks the room, the genomes go to
   `memo index` as records in memory instead, and the JSON says so ("fasta": false);
2. `memo index` (build_index, conservation) on them: per genome the pieces, FASTA read seconds, device milliseconds of
   suffix arrays, LCP + hierarchy and walks, and the device memory held after it (the buffers only grow: the peak);
3. --check 1: the first genome's column against the per-record reference -- the elementwise maximum over its records of
   the one-text path (MatchingStatistics.add(genome_text([S_i])));
4. `memo query` (conservation, k = 31) over the whole pivot on the index just written;
5. one JSON line.  Needs the GPU.  Development tool."""
import argparse
import json
import os
import shutil
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# GRCh38 chromosome lengths (1-22, X, Y), bases
CHROMS = [248956422, 242193529, 198295559, 190214555, 181538259, 170805979, 159345973, 145138636, 138394717, 133797422,
          135086622, 133275309, 114364328, 107043718, 101991189, 90338345, 83257441, 80373285, 58617616, 64444167,
          46709983, 50818468, 156040895, 57227415]
LETTERS = np.frombuffer(b"ACGT", np.uint8)
COMP = np.frombuffer(bytes.maketrans(b"ACGT", b"TGCA"), np.uint8)


def genome_records(rng, pivot, scale, g):
    """24 records; a substituted copy (0.1-1 %) of the whole pivot planted forward in one and reverse-complemented in
    another, and 50 kbp pieces of it in a few more"""
    out = []
    fwd, rev = (5 + g) % 24, (11 + 3 * g) % 24
    for r, n in enumerate(CHROMS):
        n = max(int(n * scale), 2 * len(pivot) + 10)
        seq = LETTERS[rng.integers(0, 4, n, dtype=np.uint8)]
        piece = min(50_000, len(pivot) // 2)
        for which in ([0] if r == fwd else []) + ([1] if r == rev else []) + ([2] if r % 7 == 3 else []):
            if which < 2:
                copy = pivot.copy()
            else:
                b = int(rng.integers(0, len(pivot) - piece + 1))
                copy = pivot[b:b + piece].copy()
            hit = rng.random(len(copy)) < rng.uniform(0.001, 0.01)
            copy[hit] = LETTERS[rng.integers(0, 4, int(hit.sum()), dtype=np.uint8)]
            if which == 1:
                copy = COMP[copy[::-1]]
            at = int(rng.integers(0, n - len(copy)))
            seq[at:at + len(copy)] = copy
        out.append((f"chr{r + 1}", seq))
    return out


def device_used():
    import torch
    free, total = torch.cuda.mem_get_info()
    return total - free


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=2, help="genomes besides the pivot")
    ap.add_argument("--scale", type=float, default=1.0, help="chromosome lengths x this")
    ap.add_argument("--pivot-length", type=int, default=5_000_000)
    ap.add_argument("--piece-bytes", type=int, default=0, help="piece cap (0: the library's default)")
    ap.add_argument("--check", type=int, default=1, help="check the first genome against the per-record reference")
    ap.add_argument("--seed", type=int, default=31)
    ap.add_argument("--out", default="build/assembly_scale", help="working directory (git-ignored)")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    import torch  # noqa: F401  (load order: torch's HIP runtime first, as bench.py and the tests do)
    from memo_amd import build_index as bi
    from memo_amd._lib import lib
    lib()

    t0 = time.perf_counter()
    rng = np.random.default_rng(a.seed)
    pivot = LETTERS[rng.integers(0, 4, a.pivot_length, dtype=np.uint8)]
    genome_bases = sum(max(int(n * a.scale), 2 * a.pivot_length + 10) for n in CHROMS)
    need = a.genomes * (genome_bases + 32 * 24) + a.pivot_length + (1 << 30)
    to_disk = shutil.disk_usage(a.out).free > need
    paths, in_memory = [os.path.join(a.out, "pivot.fa")], []
    with open(paths[0], "wb") as fh:
        fh.write(b">pivot\n" + pivot.tobytes() + b"\n")
    first = None
    for g in range(a.genomes):
        recs = genome_records(rng, pivot, a.scale, g)
        if g == 0 and a.check:
            first = [s.tobytes() for _, s in recs]
        if to_disk:
            p = os.path.join(a.out, f"g{g + 1}.fa")
            with open(p, "wb") as fh:
                for name, s in recs:
                    fh.write(b">" + name.encode() + b"\n")
                    fh.write(s.tobytes())
                    fh.write(b"\n")
            paths.append(p)
        else:
            in_memory.append([(n, s.tobytes()) for n, s in recs])
            paths.append(f"<memory g{g + 1}>")
        del recs
    gen_s = time.perf_counter() - t0

    lst = os.path.join(a.out, "genome_list.txt")
    with open(lst, "w") as fh:
        fh.write("".join(p + "\n" for p in paths))
    if not to_disk:         # the FASTA reader hands out the records kept in memory
        real = bi.read_fasta
        bi.read_fasta = lambda p: in_memory[int(p[len("<memory g"):-1]) - 1] if p.startswith("<memory") else real(p)
    used = [device_used()]
    st = bi.build_index(lst, a.out, "index", False, int(os.environ.get("MEMO_DEVICE", "0")),
                        log=lambda s: used.append(device_used()) if s.startswith(("Finding", "Making")) else None,
                        keep_ms=bool(a.check), piece_bytes=a.piece_bytes)
    ms = st.pop("ms", None)
    per = st.pop("per_genome")
    for g, row in enumerate(per):      # used[g + 2]: at the log line after genome g (the next "Finding", or "Making")
        row["device_gb_after"] = round(used[g + 2] / 1e9, 2)
        row["text_bytes"] = 2 * (row["bases"] + row["records"])
    out = {"genomes": a.genomes, "scale": a.scale, "pivot": a.pivot_length, "piece_bytes": a.piece_bytes, "fasta": to_disk,
           "generate_s": round(gen_s, 1), "device_gb_before": round(used[0] / 1e9, 2),
           "memo_index": {k: (round(v, 3) if isinstance(v, float) else v) for k, v in st.items()},
           "per_genome": [{k: (round(v, 3) if isinstance(v, float) else v) for k, v in r.items()} for r in per]}

    if a.check:
        t1 = time.perf_counter()
        with bi.MatchingStatistics(pivot.tobytes(), np.array([0, a.pivot_length], np.int64), 1) as h:
            ref = np.zeros(a.pivot_length, np.int32)
            for s in first:
                h.add(bi.genome_text([s]), 0)
                ref = np.maximum(ref, h.fetch()[:, 0])
        out["check"] = {"equal": bool(np.array_equal(ms[:, 0], ref)), "mismatches": int((ms[:, 0] != ref).sum()),
                        "ms_mean": round(float(ref.mean()), 2), "ms_max": int(ref.max()),
                        "seconds": round(time.perf_counter() - t1, 1)}

    t2 = time.perf_counter()
    q = os.path.join(a.out, "query.txt")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "memo"), "query", "-b", os.path.join(a.out, "index.parquet"),
                        "-k", "31", "-n", str(a.genomes + 1), "-r", f"pivot:0-{a.pivot_length}", "-o", q],
                       capture_output=True, env=dict(os.environ, MEMO_CACHE="0"))
    out["query"] = {"rc": r.returncode, "seconds": round(time.perf_counter() - t2, 2)}
    if r.returncode == 0:
        cons = np.loadtxt(q, dtype=np.int64)
        out["query"]["positions"] = int(len(cons))
        out["query"]["histogram"] = np.bincount(cons, minlength=a.genomes + 2).tolist()
    else:
        out["query"]["stderr"] = r.stderr.decode()[-500:]
    for p in paths[1:] if to_disk else []:
        os.unlink(p)
    print(json.dumps(out), flush=True)
    if a.check and not out["check"]["equal"] or r.returncode:
        sys.exit(1)


if __name__ == "__main__":
    main()
