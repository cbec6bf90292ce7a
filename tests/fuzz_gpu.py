#!/usr/bin/env python3
"""Time-boxed differential fuzzing of the HIP path against the oracle (GPU box):
    python tests/fuzz_gpu.py --seconds 300 [--seed S]
A loop over tests/sweep_lives.py: random lives of an index (the indexes, row formats, queries, kernel shapes, options and row changes
its docstring lists; every third life in one of its directed modes), each played on the GPU and compared with the oracle step by step.
Exits non-zero on the first mismatch and prints the case.  The same distribution at a fixed seed and count runs inside the suite:
tests/test_sweep_lives_gpu.py."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import memo_amd  # noqa: E402
from memo_amd import _lib  # noqa: E402
from oracle import memo_oracle as oracle  # noqa: E402  (the checker)
from tests import sweep_lives  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=60)
ap.add_argument("--seed", type=int, default=int(time.time()))
a = ap.parse_args()
L = _lib.use_ab(True)          # libmemo_amd_ab.so: the product objects + per-index kernel-shape switches
t_end = time.time() + a.seconds
cases = queries = 0
print("seed", a.seed, flush=True)
while time.time() < t_end:
    life = sweep_lives.seeded_life(a.seed, cases)
    cases += 1
    try:
        queries += sweep_lives.run_life(memo_amd, oracle, life, name=f"seed {a.seed} life {cases - 1}")
    except sweep_lives.LifeFailure as exc:
        print("MISMATCH", dict(seed=a.seed, case=cases, **exc.context), flush=True)
        version = exc.context["doing"][2] if exc.context["doing"][0] == "query" else len(life[0]["rows"]) - 1
        s, e, o = life[0]["rows"][version]
        np.savez("/tmp/fuzz_fail.npz", s=s, e=e, o=o)
        sys.exit(1)
print(f"fuzz ok: {cases} indexes, {queries} queries in {a.seconds:.0f} s", flush=True)
