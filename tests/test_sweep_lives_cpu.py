"""The case generator of the seeded sweep fuzz (tests/sweep_lives.py), without a GPU: the lives tests/test_sweep_lives_gpu.py plays are
the same on every machine, the oracle answers every one of their queries, the queries an index of dense rows alone may refuse stay
rare, and every directed mode occurs."""
import collections

import numpy as np
import pytest

from tests import sweep_lives
from tests.test_sweep_lives_gpu import LIVES

# sha256 of the step lists and rows of the LIVES lives at sweep_lives.SEED (sweep_lives.digest): changes whenever the distribution does
DIGEST = "151b99db84ad16424c272646500c11135e5ba4978d3916c490f2e202a3c6826e"


@pytest.fixture(scope="module")
def lives():
    return [sweep_lives.seeded_life(sweep_lives.SEED, i) for i in range(LIVES)]


def test_the_seeded_lives_are_deterministic(lives):
    again = [sweep_lives.seeded_life(sweep_lives.SEED, i) for i in range(LIVES)]
    assert sweep_lives.digest(again) == sweep_lives.digest(lives)
    assert sweep_lives.digest(lives[:7]) != sweep_lives.digest(lives[1:8])
    assert sweep_lives.digest(lives) == DIGEST, "the distribution changed: run the GPU test, then commit the new digest"
    assert LIVES >= 200 and sweep_lives.SEED == 20261019


def test_the_oracle_answers_every_query(lives, oracle):
    """... or raises the IndexError the library must reproduce; nothing else.  The answer has the query's shape and type."""
    forms = collections.Counter()
    for desc, steps in lives:
        assert len(desc["rows"][0][0]) <= 200_000 and 100 <= desc["length"] <= 400_000
        for step in sweep_lives.queries(steps):
            _, form, ver, qs, qe, k, n_docs, extra, _ = step
            want, err = sweep_lives.oracle_answer(oracle, desc, step)
            forms[form, err is not None] += 1
            if err is not None:
                # (only an annot outside the matrix raises: n_docs + 1 columns for conservation, n_docs for membership)
                columns = n_docs if form in ("memb", "oneshot_memb") else n_docs + 1
                assert err is IndexError and form != "slice" and int(desc["rows"][ver][2].max()) >= columns, step
                continue
            a, b = extra if form == "slice" else (qs, qe)
            if form == "slice":                                # strictly inside, at the left edge or at the right edge of its window
                assert qs <= a < b <= qe and (a, b) != (qs, qe), step
            if form in ("cons16", "cons8", "oneshot_cons"):
                assert want.shape == (b - a,) and want.dtype == (np.uint8 if form == "cons8" else np.uint16), step
                assert int(want.max(initial=0)) <= n_docs, step
            else:
                assert want.shape == (b - a, (n_docs + 31) // 32) and want.dtype == np.uint32, step
    print(sorted(forms.items()))
    for form in ("cons16", "cons8", "memb", "slice", "oneshot_cons", "oneshot_memb"):
        assert forms[form, False] >= 50, (form, forms)
    assert sum(n for (_, raised), n in forms.items() if raised) >= 50      # (the IndexError path is played too)
    n8, n16 = forms["cons8", False] + forms["cons8", True], forms["cons16", False] + forms["cons16", True]
    assert n8 >= n16 // 4                                      # (uint8 for about half of the conservation queries with num_docs <= 255)


def test_refusals_stay_rare(lives):
    """An index that holds the dense rows alone may refuse a query -- only where memo_dense_rows_can_answer (pure host arithmetic) says
    0.  Such lives are at most a fifth of the lives, leave the tile shape and the scatter to the library, and redraw a query the
    predicate refuses three times out of four: the queries that may be refused stay under 5 % of all queries."""
    from memo_amd.index import dense_rows_can_answer
    dense_lives = total = may = 0
    for desc, steps in lives:
        dense_lives += desc["dense_only"]
        s, _, o = desc["rows"][0]
        for step in steps:
            if step[0] == "tuning" and desc["dense_only"]:
                assert step[1:] == (0, 0, 0, 0, 0), step
            if step[0] == "prepare" and not desc["dense_only"]:
                assert not step[5], step
            if step[0] != "query":
                continue
            total += 1
            may += step[8]
            _, form, ver, qs, qe, k, n_docs, extra, may_refuse = step
            if not desc["dense_only"] or form.startswith("oneshot"):
                assert not may_refuse, step
            else:
                assert ver == 0 and k <= 64, step              # (no row change without the int64 columns; dense rows answer k <= 64)
                can = dense_rows_can_answer(len(s), int(s[0]), int(s[-1]), int(o.max()), k, n_docs, form in ("memb", "slice"))
                assert may_refuse == (not can), step
    print(f"{dense_lives} of {len(lives)} lives hold the dense rows alone; {may} of {total} queries may be refused")
    assert 0 < 5 * dense_lives <= len(lives)
    assert 0 < may and 20 * may < total


def test_every_directed_mode_occurs(lives):
    modes = collections.Counter(desc["directed"] for desc, _ in lives)
    print(modes)
    for mode in sweep_lives.DIRECTED:
        assert modes[mode] >= 8, modes
    assert modes[None] >= len(lives) // 2
    # ... and every kind of step, every row change among them
    ops = collections.Counter(step[0] for _, steps in lives for step in steps)
    for op in ("pack", "pack_dense", "row_order", "switches", "prepare", "option", "tuning", "query", "upload_rows", "truncate", "finalize"):
        assert ops[op] >= 8, ops
    assert sum(1 for _, steps in lives for step in steps if step[:2] == ("pack_dense", False)) >= 8
    options = collections.Counter(step[1:3] for _, steps in lives for step in steps if step[0] == "option")
    for opt, values in sweep_lives.OPTION_VALUES.items():
        for v in set(values):
            assert options[opt, v] >= 1, (opt, v, options)
    chain = collections.Counter(step[5] >> 8 for _, steps in lives for step in steps if step[0] == "tuning")
    assert all(chain[c] >= 1 for c in range(16)), chain
    assert max(sum(1 for step in steps if step[0] in ("upload_rows", "truncate")) for _, steps in lives) <= 3
