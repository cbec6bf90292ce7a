#!/usr/bin/env python3
"""Where a wide tile's residency goes (diagnostic -DMEMO_STAMPS build only; memo_sweep_cons3t.hip: wide_tile): config 3's live copy at
k = 31, one whole-window uint8 launch, wave 0 of every workgroup stamping entry, descriptor arrived, first barrier, its first row
piece available, second barrier and end.  Prints, over all tiles, the quartiles of entry -> rows available (the head), rows available
-> end, and the whole residency, in shader cycles, and the head's share of the residency.
  MEMO_AMD_AB_LIB=$PWD/memo_amd/libmemo_amd_stamps_ab.so python tools/wide_tile_stamps.py
GPU box."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PHASES = ("entry -> descriptor", "descriptor -> first barrier", "first barrier -> rows available", "rows available -> second barrier",
          "second barrier -> end")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--length", type=int, default=100_000_000)
    a = ap.parse_args()
    import numpy as np
    import torch
    from memo_amd import _lib, synth
    _lib.use_ab()
    num_docs, L = 100, a.length
    out = torch.empty(L, dtype=torch.uint8, device="cuda:0")
    stream = torch.cuda.current_stream()
    ix, _ = synth.device_index(0, L, 31, num_docs, L, pack="dense")
    with ix:
        ix.set_option(3, 0)                       # MEMO_OPT_BUILD_COST_PCT: the first query of a class builds
        ix.prepare(a.k, num_docs)
        for _ in range(3):                        # (the view, its places, the copy)
            ix.conservation_u8_dev(0, L, a.k, num_docs, out, stream.cuda_stream)
        torch.cuda.synchronize()
        inf = ix.info()
        nblocks = 8 * ((L // inf["last_tile_width"] + 8) // 8 + 1) + 8
        buf = torch.zeros(8 * nblocks, dtype=torch.int64, device="cuda:0")
        _lib.check(_lib.lib().memo_debug_set_stamp_buffer(C.c_void_p(buf.data_ptr())))
        for _ in range(2):
            buf.zero_()
            ix.conservation_u8_dev(0, L, a.k, num_docs, out, stream.cuda_stream)
            torch.cuda.synchronize()
        _lib.check(_lib.lib().memo_debug_set_stamp_buffer(None))
        inf = ix.info()
    st = buf.cpu().numpy().reshape(-1, 8)
    st = st[st[:, 7] == 1][:, :5].astype(np.float64)
    head, rest, whole = st[:, :3].sum(axis=1), st[:, 3:].sum(axis=1), st.sum(axis=1)

    def q(v):
        return [round(float(x), 1) for x in np.percentile(v, (25, 50, 75))]

    print(json.dumps({"k": a.k, "tiles": len(st), "tile_width": inf["last_tile_width"], "variant": inf["last_variant"]}))
    for name, col in zip(PHASES, st.T):
        print(json.dumps({"phase": name, "q25_median_q75": q(col), "mean": round(float(col.mean()), 1)}))
    for name, v in (("entry -> rows available", head), ("rows available -> end", rest), ("residency", whole)):
        print(json.dumps({"span": name, "q25_median_q75": q(v), "mean": round(float(v.mean()), 1)}))
    print(json.dumps({"head_share_of_medians": round(float(np.median(head) / np.median(whole)), 4),
                      "head_share_of_means": round(float(head.mean() / whole.mean()), 4),
                      "median_of_per_tile_head_share": round(float(np.median(head / whole)), 4)}))


if __name__ == "__main__":
    main()
