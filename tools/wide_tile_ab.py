#!/usr/bin/env python3
"""A/B of the sweep on config 3's six-row k-class views: the radix-4 arrays in wide tiles (MEMO_OPT_WIDE_TILES 1, memo_sweep_cons3t.hip:
R4) against the doubling arrays (MEMO_OPT_WIDE_TILES 0).  Per k the class's view and its copy without dead groups are built first
(MEMO_OPT_BUILD_COST_PCT 0); `--plain` sweeps the view without places instead (MEMO_OPT_VIEW_PLACES 0: no flags, no copy, 4x the
rows per tile).  Then, per round and variant, `--launches` whole-window uint8 launches back to back, each between a HIP event pair;
the median of the last `--keep`.  Variants alternate `--reps` times on the same index.  `--density` (rows per genome-position, a
fraction; config 3 has 5/100) makes the rows per tile denser or sparser: the points the launcher's kR4MaxGroups stands between.  GPU box."""
import argparse
from fractions import Fraction
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="31,21,17,9")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--launches", type=int, default=600)
    ap.add_argument("--keep", type=int, default=400)
    ap.add_argument("--plain", action="store_true")
    ap.add_argument("--density", type=Fraction, default=Fraction(5, 100))
    a = ap.parse_args()
    import numpy as np
    import torch
    from memo_amd import synth
    num_docs, L = 100, 100_000_000
    out = torch.empty(L, dtype=torch.uint8, device="cuda:0")
    stream = torch.cuda.current_stream()
    ix, _ = synth.device_index(0, L, 31, num_docs, L, density=a.density, pack="dense")

    def one(k):
        ix.conservation_u8_dev(0, L, k, num_docs, out, stream.cuda_stream)

    with ix:
        ix.set_option(3, 0)                       # MEMO_OPT_BUILD_COST_PCT: the first query of a class builds
        if a.plain:
            ix.set_option(5, 0)                   # MEMO_OPT_VIEW_PLACES
        for k in [int(x) for x in a.ks.split(",")]:
            ix.prepare(k, num_docs)
            for _ in range(3):                    # (the view, its places, the copy)
                one(k)
            torch.cuda.synchronize()
            for rep in range(a.reps):
                for wide in (1, 0):
                    ix.set_option(7, wide)        # MEMO_OPT_WIDE_TILES
                    one(k)
                    torch.cuda.synchronize()
                    inf = ix.info()
                    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.launches)]
                    for e0, e1 in ev:
                        e0.record(stream)
                        one(k)
                        e1.record(stream)
                    torch.cuda.synchronize()
                    ms = [e0.elapsed_time(e1) for e0, e1 in ev][-a.keep:]
                    print(json.dumps({"k": k, "rep": rep, "wide_tiles": wide, "ms": round(float(np.median(ms)), 5),
                                      "tile_width": inf["last_tile_width"], "variant": inf["last_variant"],
                                      "rows_read": inf["last_rows_read"], "plain": a.plain, "density": str(a.density),
                                      "groups_per_tile": round(inf["last_rows_read"] / 6 * inf["last_tile_width"] / L, 1)}),
                          flush=True)
            ix.set_option(7, 1)


if __name__ == "__main__":
    main()
