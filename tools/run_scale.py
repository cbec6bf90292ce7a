#!/usr/bin/env python3
"""What long runs cost the MS walk of `memo index`: one pivot, one genome, per stage.

    python tools/run_scale.py [--budget B] [--cases n16,n18,n20,n22,sat] [--tree DIR] [--label NAME]
                              [--out profiles/ms_runs.txt]

Cases:
  nK    a pivot N run of 2^K bases inside ACGT (3000 random bases on either side) against a genome whose N run is twice as
        long.  The bases next to the runs are fixed so that MS inside the pivot's run is the closed form R, R - 1, .. 1,
        which the run is checked against.
  sat   a satellite array: a random 171-base monomer, 20,000 copies, 1 % of the bases substituted independently in the pivot
        and in the genome (1000 random bases on either side).  No closed form; the sum of the MS is printed, so that runs at
        different budgets can be compared.
--budget: the walk's budget (memo_ms_set_walk_budget; unset: the library's default).  2^30 or more is the walk without seed
search, which takes time in proportion to the run: it is run at n16 and n18 only, whatever --cases says.
--tree: the checkout whose memo_amd is measured (default: this one); one without the budget (an older commit) is the walk
without seed search too: n16 and n18 only, as it is, no counters.  --label: what the lines call the tree (default: its path
from this one).

Each case runs in a process of its own under --timeout seconds; the first one that fails ends the run.  One line per case, to
stdout and appended to --out.  Needs the GPU.  Development tool."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEVER = 1 << 30


def rand(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()


def mutate(rng, seq, rate):
    s = np.frombuffer(seq, np.uint8).copy()
    hit = rng.random(len(s)) < rate
    s[hit] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(hit.sum()))]
    return s.tobytes()


def make_case(name):
    """(pivot record, genome record, (first position, closed-form MS from there on) or None)"""
    if name == "sat":
        rng = np.random.default_rng(171)
        array = rand(rng, 171) * 20_000
        return (rand(rng, 1000) + mutate(rng, array, 0.01) + rand(rng, 1000),
                rand(rng, 1000) + mutate(rng, array, 0.01) + rand(rng, 1000), None)
    R = 1 << int(name[1:])
    rng = np.random.default_rng(R)
    pivot = rand(rng, 3000) + b"N" * R + b"A" + rand(rng, 2999)
    genome = rand(rng, 1999) + b"C" + b"N" * (2 * R) + b"C" + rand(rng, 1999)
    return pivot, genome, (3000, np.arange(R, 0, -1, dtype=np.int32))


def has_budget(tree):
    with open(os.path.join(tree, "memo_amd", "build_index.py")) as fh:
        return "set_walk_budget" in fh.read()


def run_case(name, budget, tree, label):
    sys.path.insert(0, tree)
    import torch  # noqa: F401  (load order: torch's HIP runtime first, as bench.py and the tests do)
    from memo_amd import build_index as bi
    pivot, genome, closed = make_case(name)
    out = {"case": name, "tree": label, "pivot": len(pivot), "genome": len(genome)}
    with bi.MatchingStatistics(pivot, np.array([0, len(pivot)], np.int64), 1) as ms:
        if hasattr(ms, "set_walk_budget"):
            ms.set_walk_budget(budget)
        elif budget is not None and budget < NEVER:
            raise SystemExit(f"{tree}: this memo_amd has no walk budget")
        ms.add(bi.genome_text([genome]), 0)
        out.update({k: round(v, 3) for k, v in ms.timings().items()})
        if hasattr(ms, "walk_info"):
            out.update(ms.walk_info())
        got = ms.fetch()[:, 0]
    out["ms_sum"] = int(got.sum(dtype=np.int64))
    if closed is not None:
        first, want = closed
        out["closed_form_equal"] = bool(np.array_equal(got[first:first + len(want)], want))
    print(json.dumps(out), flush=True)
    return 0 if out.get("closed_form_equal", True) else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--budget", type=int, default=None)
    ap.add_argument("--cases", default="n16,n18,n20,n22,sat")
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--label")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ms_runs.txt"))
    ap.add_argument("--timeout", type=int, default=240, help="seconds per case")
    ap.add_argument("--one", help=argparse.SUPPRESS)
    a = ap.parse_args()
    tree = os.path.abspath(a.tree)
    label = a.label or os.path.relpath(tree, ROOT)
    if a.one:
        sys.exit(run_case(a.one, a.budget, tree, label))
    cases = [c for c in a.cases.split(",") if c]
    if (a.budget is not None and a.budget >= NEVER) or not has_budget(tree):
        cases = [c for c in cases if c in ("n16", "n18")]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for case in cases:
        argv = [sys.executable, os.path.abspath(__file__), "--one", case, "--tree", tree, "--label", label]
        if a.budget is not None:
            argv += ["--budget", str(a.budget)]
        try:
            r = subprocess.run(argv, capture_output=True, text=True, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            sys.exit(f"{case}: not done after {a.timeout} s; stopping")
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        with open(a.out, "a") as fh:
            fh.write(r.stdout)
        if r.returncode:
            sys.stderr.write(r.stderr[-2000:])
            sys.exit(f"{case}: failed with status {r.returncode}; stopping")


if __name__ == "__main__":
    main()
