#!/usr/bin/env python3
"""A/B of the sweep on config 3's placed six-row k-class view: the copy without dead groups (MEMO_OPT_VIEW_LIVE 1, memo_view_build.hip:
live_view_copy) against the flagged view swept with LIVE (MEMO_OPT_VIEW_LIVE 0).  Per round, variant and k: the views are dropped,
memo_index_prepare builds the placed view, and the live variant's copy is built by the queries that pay for it under the default
ledger (counted: `queries_to_copy`; the pass's device time: `copy_ms`).  Then `--launches` launches back to back, each between a HIP
event pair; the median of the last `--keep`.  Variants alternate `--reps` times.  GPU box; A/B library (memo_debug_view_live)."""
import argparse
import ctypes as C
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
    a = ap.parse_args()
    import numpy as np
    import torch
    from memo_amd import _lib, synth
    _lib.use_ab(True)
    lib = _lib.lib()
    num_docs, L = 100, 100_000_000
    out = torch.empty(L, dtype=torch.uint8, device="cuda:0")
    stream = torch.cuda.current_stream()
    ix, _ = synth.device_index(0, L, 31, num_docs, L, pack="dense")

    def live_state(k):
        n = C.c_uint64(0)
        return _lib.check(lib.memo_debug_view_live(ix._h, int(k), C.byref(n))), n.value

    def one(k):
        ix.conservation_u8_dev(0, L, k, num_docs, out, stream.cuda_stream)

    with ix:
        for rep in range(a.reps):
            for live in (1, 0):
                for k in [int(x) for x in a.ks.split(",")]:
                    ix.set_option(1, 0)
                    ix.set_option(1, 1)
                    ix.set_option(6, live)
                    ix.prepare(k, num_docs)
                    inf = ix.info()
                    flagged_rows = inf["last_rows_read"]
                    queries, copy_ms = 0, 0.0
                    if live:  # the default ledger: whole-window queries until one of them builds the copy (at most 64)
                        while queries < 64 and not live_state(k)[0]:
                            one(k)
                            torch.cuda.synchronize()
                            queries += 1
                            copy_ms = float(ix.info()["last_view_ms"]) if live_state(k)[0] else 0.0
                    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.launches)]
                    for e0, e1 in ev:
                        e0.record(stream)
                        one(k)
                        e1.record(stream)
                    torch.cuda.synchronize()
                    ix.check()
                    ms = np.array([e0.elapsed_time(e1) for e0, e1 in ev[a.launches - a.keep:]])
                    inf = ix.info()
                    rec = {"round": rep, "variant": "copy" if live else "flagged+LIVE", "k": k,
                           "ms_median": round(float(np.median(ms)), 4), "ms_min": round(float(ms.min()), 4),
                           "slots_read": inf["last_rows_read"], "slots_flagged_view": flagged_rows, "variant_id": inf["last_variant"],
                           "is_copy": live_state(k)[0]}
                    if live:
                        rec.update({"queries_to_copy": queries, "copy_ms": round(copy_ms, 3)})
                    print(json.dumps(rec), flush=True)
        ix.set_option(6, 1)


if __name__ == "__main__":
    main()
