#!/usr/bin/env python3
"""How much of a matching-statistics column the run code of the coded DAP layout has to store, measured on the device.

    python tools/coded_share.py [--length 20000000] [--seed 20260]

A random ACGT pivot of --length bases (two records) against: itself; copies mutated as tools/realistic_index.py does (SNPs at
0.1 %, 1 % and 10 %, with its short indels, inversions and translocations); unrelated random text; and, on a pivot with a
run of N over a fiftieth of it, the same pivot without the run.  Both strands, as `memo index` builds the text.  Per genome:
the flagged share (forced block-start flags included), the device bytes of the column per position (memo_ms_column_info),
and the encode pass's device milliseconds.  One JSON line.  Needs the GPU.  Development tool."""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LETTERS = np.frombuffer(b"ACGT", np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=20_000_000)
    ap.add_argument("--seed", type=int, default=20260)
    a = ap.parse_args()
    spec = importlib.util.spec_from_file_location("realistic_index", os.path.join(ROOT, "tools", "realistic_index.py"))
    ri = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ri)
    import torch  # noqa: F401  (load order: torch's HIP runtime first, as bench.py and the tests do)
    from memo_amd import build_index as bi
    rng = np.random.default_rng(a.seed)
    L = a.length
    pivot = rng.integers(0, 4, L).astype(np.uint8)
    rb = np.array([0, L // 3, L], np.int64)
    genomes = [("identical", pivot)]
    genomes += [(f"realistic_index mutations, SNPs {snp:g}", ri.mutate(rng, pivot, snp, g + 1)) for g, snp in enumerate((0.001, 0.01, 0.1))]
    genomes.append(("unrelated random text", rng.integers(0, 4, L).astype(np.uint8)))
    out = {"length": L, "records": 2, "genomes": []}

    def measure(ms, name, codes, column):
        before = ms.layout_info()["encode_ms"]
        ms.add_records([LETTERS[codes].tobytes()], column)
        info = ms.column_info(column)
        out["genomes"].append({"genome": name, "flagged": info["flagged"], "flagged_share": round(info["flagged"] / L, 6),
                               "bytes_per_position": round(info["bytes"] / L, 4),
                               "encode_ms": round(ms.layout_info()["encode_ms"] - before, 3)})
    with bi.MatchingStatistics(LETTERS[pivot].tobytes(), rb, len(genomes), layout="coded") as ms:
        out["block"] = ms.layout_info()["block"]
        for c, (name, codes) in enumerate(genomes):
            measure(ms, name, codes, c)
        info = ms.layout_info()
        out["device_bytes"], out["dense_bytes"] = info["device_bytes"], info["dense_bytes"]
    gapped = LETTERS[pivot].copy()
    gapped[L // 2:L // 2 + L // 50] = ord("N")
    with bi.MatchingStatistics(gapped.tobytes(), rb, 1, layout="coded") as ms:
        measure(ms, f"pivot with a run of {L // 50} N, genome without", pivot, 0)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
