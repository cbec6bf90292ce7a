#!/usr/bin/env python3
"""`memo index` on a pivot whose DAP matrix does not fit on the device: the coded layout end to end, then `memo query`.

    python tools/pivot_scale.py [--pivot-length 1000000000] [--records 4] [--genomes 0] [--base 20000000] [--layout auto]
                                [--out build/pivot_scale]

1. a base text of --base random bases; a pivot of --records records, --pivot-length bases in all, each record a chain of
   copies of the base with substitutions (--pivot-snp); --genomes genomes besides the pivot (0: two more than the fewest whose
   matrix positions x genomes x 4 B passes the device's TOTAL memory), each one record: the base with substitutions at a rate
   drawn log-uniformly from [--snp-lo, --snp-hi].  Short genomes that are close to every part of the pivot: the MS stage stays
   cheap and every column is the low-divergence case.  FASTA under --out, one line per record;
2. `bin/memo index` (conservation) on them, as a user runs it, its figures read back through MEMO_INDEX_STATS: the layout
   taken, seconds per stage, device milliseconds of suffix arrays / LCP / walks / encode / decode, device bytes held for the
   DAP, flagged share, rows, and the command's peak RSS; the dense layout's refusal of the same shape is recorded first;
3. `memo query` (conservation, k = 31) over the whole first pivot record;
4. --compare 1: the first pivot record alone against the same genomes with --layout dense (where that fits), the same query,
   and the two outputs compared byte for byte;
5. one JSON line.  Needs the GPU.  Development tool."""
import argparse
import json
import os
import resource
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LETTERS = np.frombuffer(b"ACGT", np.uint8)


def substituted(rng, codes, rate):
    out = codes.copy()
    hit = np.flatnonzero(rng.random(len(out), dtype=np.float32) < rate)
    out[hit] = rng.integers(0, 4, len(hit), dtype=np.uint8)
    return out


def memo_index(lst, out, layout):
    """`bin/memo index -g lst -o out -p index` as a user runs it; its figures through MEMO_INDEX_STATS (the per-genome list summed
    up), its peak RSS from the children's resource usage (this process starts nothing larger before it)"""
    stats_path = os.path.join(out, "index_stats.json")
    env = dict(os.environ, MEMO_INDEX_STATS=stats_path)
    env.pop("MEMO_INDEX_DAP_LAYOUT", None)
    if layout != "auto":
        env["MEMO_INDEX_DAP_LAYOUT"] = layout
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "memo"), "index", "-g", lst, "-o", out, "-p", "index"],
                       capture_output=True, text=True, env=env)
    wall = round(time.perf_counter() - t0, 1)
    if r.returncode:
        return {"rc": r.returncode, "stderr": r.stderr[-800:], "wall_s": wall}
    st = json.load(open(stats_path))
    per = st.pop("per_genome")
    st.pop("pieces")
    flagged = [g["flagged"] for g in per]
    st["flagged_total"] = int(sum(flagged))
    st["flagged_share"] = {"mean": sum(flagged) / (len(flagged) * st["positions"]), "min": min(flagged) / st["positions"],
                           "max": max(flagged) / st["positions"]}
    st["genome_read_s"] = sum(g["read_s"] for g in per)
    st["peak_rss_children_gb"] = resource.getrusage(resource.RUSAGE_CHILDREN).ru_maxrss / 1e6
    st["wall_s"] = wall
    return {k: (round(v, 4) if isinstance(v, float) else v) for k, v in st.items()}


def query(index, region, n, out_path):
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "memo"), "query", "-b", index, "-k", "31", "-n", str(n), "-r", region,
                        "-o", out_path], capture_output=True, env=dict(os.environ, MEMO_CACHE="0"))
    return {"rc": r.returncode, "seconds": round(time.perf_counter() - t0, 2), **({"stderr": r.stderr.decode()[-500:]} if r.returncode else {})}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pivot-length", type=int, default=1_000_000_000)
    ap.add_argument("--records", type=int, default=4)
    ap.add_argument("--genomes", type=int, default=0, help="genomes besides the pivot (0: enough for the matrix to pass the device's memory)")
    ap.add_argument("--base", type=int, default=20_000_000)
    ap.add_argument("--pivot-snp", type=float, default=0.001)
    ap.add_argument("--snp-lo", type=float, default=0.0005)
    ap.add_argument("--snp-hi", type=float, default=0.002)
    ap.add_argument("--layout", default="auto", choices=["auto", "dense", "coded"])
    ap.add_argument("--compare", type=int, default=1)
    ap.add_argument("--seed", type=int, default=77)
    ap.add_argument("--out", default="build/pivot_scale", help="working directory (git-ignored)")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    import torch
    from memo_amd import _lib
    free, total = torch.cuda.mem_get_info()
    genomes = a.genomes or total // (a.pivot_length * 4) + 3
    out = {"positions": a.pivot_length, "records": a.records, "columns": genomes, "base": a.base,
           "dense_gb": round(a.pivot_length * genomes * 4 / 1e9, 1), "device_total_gb": round(total / 1e9, 1),
           "device_free_gb": round(free / 1e9, 1)}

    t0 = time.perf_counter()
    rng = np.random.default_rng(a.seed)
    base = rng.integers(0, 4, a.base, dtype=np.uint8)
    lens = [a.pivot_length // a.records + (1 if r < a.pivot_length % a.records else 0) for r in range(a.records)]
    paths = [os.path.join(a.out, "pivot.fa")]
    first_path = os.path.join(a.out, "pivot_r1.fa")
    with open(paths[0], "wb") as fh:
        for r, n in enumerate(lens):
            fh.write(b">r%d\n" % (r + 1))
            shift = int(rng.integers(0, a.base))                   # every record starts somewhere else in the base
            done, rec = 0, []
            while done < n:
                part = substituted(rng, np.roll(base, -shift)[:min(a.base, n - done)], a.pivot_snp)
                rec.append(LETTERS[part].tobytes())
                fh.write(rec[-1])
                done += len(part)
            fh.write(b"\n")
            if r == 0:
                with open(first_path, "wb") as f1:
                    f1.write(b">r1\n" + b"".join(rec) + b"\n")
            del rec
    for g in range(genomes):
        p = os.path.join(a.out, f"g{g + 1}.fa")
        snp = float(np.exp(rng.uniform(np.log(a.snp_lo), np.log(a.snp_hi))))
        with open(p, "wb") as fh:
            fh.write(b">chr1\n" + LETTERS[substituted(rng, base, snp)].tobytes() + b"\n")
        paths.append(p)
    out["generate_s"] = round(time.perf_counter() - t0, 1)

    # what the dense layout says to this shape with the memory that is free now (memo_ms_create's check, host only)
    from memo_amd import build_index as bi
    try:
        bi.plan_layout(a.pivot_length, genomes, free, "dense")
        out["dense_layout"] = "accepted"
    except _lib.MemoError as exc:
        out["dense_layout"] = str(exc)

    lst = os.path.join(a.out, "genome_list.txt")
    with open(lst, "w") as fh:
        fh.write("".join(p + "\n" for p in paths))
    out["memo_index"] = memo_index(lst, a.out, a.layout)
    ok = "rc" not in out["memo_index"]
    region = f"r1:0-{lens[0]}"
    if ok:
        out["index_file_gb"] = round(os.path.getsize(os.path.join(a.out, "index.parquet")) / 1e9, 2)
        out["query"] = query(os.path.join(a.out, "index.parquet"), region, genomes + 1, os.path.join(a.out, "query.txt"))
        ok = out["query"]["rc"] == 0
    if ok and a.compare:
        dense_dir = os.path.join(a.out, "dense_r1")
        os.makedirs(dense_dir, exist_ok=True)
        lst1 = os.path.join(dense_dir, "genome_list.txt")
        with open(lst1, "w") as fh:
            fh.write("".join(p + "\n" for p in [first_path] + paths[1:]))
        out["dense_first_record"] = memo_index(lst1, dense_dir, "dense")
        if "rc" not in out["dense_first_record"]:
            out["dense_query"] = query(os.path.join(dense_dir, "index.parquet"), region, genomes + 1, os.path.join(dense_dir, "query.txt"))
            if out["dense_query"]["rc"] == 0:
                same = subprocess.run(["cmp", "-s", os.path.join(a.out, "query.txt"), os.path.join(dense_dir, "query.txt")]).returncode == 0
                out["queries_equal"] = same
                out["query_bytes"] = os.path.getsize(os.path.join(a.out, "query.txt"))
                ok = same
    for p in paths + [first_path]:
        os.unlink(p)
    print(json.dumps(out), flush=True)
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
