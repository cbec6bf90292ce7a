#!/usr/bin/env python3
"""A/B of the wide tiles' pair kernel (memo_sweep_cons3t.hip: sweep_conservation_wide_pair_kernel, two tiles per workgroup behind one
head) against one tile per workgroup (sweep_conservation_wide_kernel) on config 3's live copy, inside ONE library:
memo_debug_set_tuning's scatter bit 11 (2048) switches pairs OFF.  `--density` as tools/wide_tile_ab.py has it, `--plain` the placed
view without a copy.  Per k the class's view and its copy are built first; then, per round and variant, `--launches` whole-window uint8 launches back
to back, each between a HIP event pair; the median of the last `--keep`.  Variants alternate `--reps` times on the same index.  Needs
libmemo_amd_ab.so.  GPU box."""
import argparse
from fractions import Fraction
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = (("one tile per workgroup", 8), ("pairs", 0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="31,21,17")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--launches", type=int, default=600)
    ap.add_argument("--keep", type=int, default=400)
    ap.add_argument("--plain", action="store_true")
    ap.add_argument("--density", type=Fraction, default=Fraction(5, 100))
    a = ap.parse_args()
    import numpy as np
    import torch
    from memo_amd import _lib, synth
    _lib.use_ab()
    num_docs, L = 100, 100_000_000
    out = torch.empty(L, dtype=torch.uint8, device="cuda:0")
    first = None
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
            first = None
            for rep in range(a.reps):
                for name, off in VARIANTS:
                    ix.debug_set_tuning(scatter=off << 8)
                    one(k)
                    torch.cuda.synchronize()
                    same = True
                    if first is None:
                        first = out.clone()
                    else:
                        same = bool(torch.equal(first, out))
                    inf, per_group = ix.info(), ix.debug_last_tiles_per_group()
                    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.launches)]
                    for e0, e1 in ev:
                        e0.record(stream)
                        one(k)
                        e1.record(stream)
                    torch.cuda.synchronize()
                    ms = [e0.elapsed_time(e1) for e0, e1 in ev][-a.keep:]
                    print(json.dumps({"k": k, "rep": rep, "variant_name": name, "off_mask": off, "ms": round(float(np.median(ms)), 5),
                                      "tile_width": inf["last_tile_width"], "variant": inf["last_variant"],
                                      "tiles_per_group": per_group, "density": str(a.density), "plain": a.plain,
                                      "groups_per_tile": round(inf["last_rows_read"] / 6 * inf["last_tile_width"] / L, 1),
                                      "same_bytes_as_first": same}), flush=True)
            ix.debug_set_tuning()


if __name__ == "__main__":
    main()
