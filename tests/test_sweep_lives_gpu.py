"""The seeded sweep fuzz inside the suite: LIVES lives of tests/sweep_lives.py at seed 20261019, played on the GPU in blocks, every
answer compared with the oracle's exactly -- and a ledger of which kernel instance answered each query (memo_debug_last_pick,
memo_debug_last_membership), so that "the fuzz passed" also says which template arguments of which family it passed ON.

REQUIRED below is written out from the pickers (memo_sweep_cons.hip: query_conservation; memo_sweep_cons3t.hip: launch_halo3t;
memo_sweep_memb.hip: memo_query_membership_dev), not from what the seed happened to reach: per kernel family every value of every
template argument its launcher can pass, every (family, row format, OutT) the code allows, every membership algorithm with every MW
and SK.  A pick the seed misses gets a directed mode in tests/sweep_lives.py (DIRECTED), never a deletion here.

Measured on one MI355X: 360 lives in 24 blocks of 15, 5571 queries, 72 of them refused (dense rows alone, the predicate 0); seconds
per block, oracle included: 0.5 0.2 0.4 0.1 0.8 0.3 0.2 0.1 0.1 0.2 0.2 0.2 0.1 0.1 0.2 0.1 0.4 0.1 0.2 0.1 0.2 0.1 0.1 0.1 (5 s in
all; the lives are small and the device is idle between their launches).  The count per pick: test_every_pick_is_reached's
docstring.  No time is asserted."""
import collections
import time

import numpy as np
import pytest

from tests import sweep_lives

pytestmark = pytest.mark.gpu

LIVES = 360
PER_BLOCK = 15
BLOCKS = LIVES // PER_BLOCK

# ---- the picks: (name, form, {field: value ...}) -- reached when some ledger entry of that form has all these values ---------------
FAMILIES = {1: "sweep_conservation_kernel", 2: "sweep_conservation_halo_kernel", 3: "sweep_conservation_r4_kernel",
            4: "sweep_conservation_mixed_kernel"}


def _required():
    req = []

    def cons(name, **fields):
        req.append((name, "cons", fields))

    def memb(name, **fields):
        req.append((name, "memb", fields))
    # sweep_conservation_kernel<Rows, W, Rows::kLoads, T, OutT> (pick_rows_clipped, pick_int<256 .. 4096>, pick_int<256, 64>)
    cons("clipped WideRows", family=1, format=0)
    for fmt in (4, 12, 6):
        for checked in (0, 1):
            cons(f"clipped PackedRows fmt {fmt} CHECKED {checked}", family=1, format=fmt, checked=checked)
    for w in (256, 512, 1024, 2048, 4096):
        cons(f"clipped W {w}", family=1, width=w)
    for t in (256, 64):
        cons(f"clipped T {t}", family=1, threads=t)
    for fmt in (0, 4, 12, 6):
        for ob in (1, 2):
            cons(f"clipped fmt {fmt} OutT {ob} B", family=1, format=fmt, out_bytes=ob)
    # sweep_conservation_halo_kernel / _r4_kernel / _mixed_kernel<Rows, kHaloLoads, T, OutT, TOP> (pick_packed<false>, pick_top,
    # pick_int<512, 256, 64>); uint8 results need num_docs <= 255 and every annot inside the matrix: format 4 alone
    for fam in (2, 3, 4):
        n = FAMILIES[fam]
        for fmt in (4, 12, 6):
            cons(f"{n} fmt {fmt} OutT 2 B", family=fam, format=fmt, out_bytes=2)
        cons(f"{n} fmt 4 OutT 1 B", family=fam, format=4, out_bytes=1)
        for t in (512, 256, 64):
            cons(f"{n} T {t}", family=fam, threads=t)
        for top in (24, 20, 0):
            cons(f"{n} TOP {top}", family=fam, top=top)
    # sweep_conservation_halo3_kernel<PackedRows3::kLoads, T, OutT, A9> (no tile table: the debug row sources 5 and 10)
    for t in (512, 256, 64):
        cons(f"halo3 T {t}", family=5, format=3, halo3=1, threads=t)
    for ob in (1, 2):
        cons(f"halo3 OutT {ob} B", family=5, format=3, halo3=1, out_bytes=ob)
    for a9 in (0, 1):
        cons(f"halo3 A9 {a9}", family=5, halo3=1, a9=a9)
    # sweep_conservation_halo3t_kernel<N, OutT, 256, A9, AW, SIX, SP, LIVE, R4>
    for nlev in (1, 2, 3, 4, 5, 6):
        cons(f"halo3t N {nlev}", kernel=1, nlev=nlev)
    for ob in (1, 2):
        cons(f"halo3t OutT {ob} B", kernel=1, format=3, out_bytes=ob)
    for f in ("a9", "aw", "six", "sp", "live", "r4"):
        for v in (0, 1):
            cons(f"halo3t {f.upper()} {v}", kernel=1, **{f: v})
    for aw in (0, 1):
        for sp in (0, 1):
            cons(f"halo3t A9 AW {aw} SP {sp}", kernel=1, a9=1, aw=aw, sp=sp)
    # sweep_conservation_wide_args_kernel<OutT, AW, SP, CH> (CH 1 .. 3), _wide_kernel<OutT, AW, SP, CH> (CH 0 .. 3),
    # _wide_pair_kernel<OutT, AW, true, 3>.
    # NOT REACHABLE, left out: SP = false of the three wide kernels (and of halo3t's R4 instance).  launch_halo3t takes the wide tile
    # only while groups_per_tile(wide tile) < kR4MaxGroups = 543, and computes sp = groups_per_tile(the same tile) < 768 afterwards:
    # r4 implies sp.  The pickers instantiate SP = false for these kernels, no input launches it.
    for kern, name, chains in ((2, "wide_args", (1, 2, 3)), (3, "wide", (0, 1, 2, 3)), (4, "wide_pair", (3,))):
        for ob in (1, 2):
            cons(f"{name} OutT {ob} B", kernel=kern, out_bytes=ob)
        for aw in (0, 1):
            cons(f"{name} AW {aw}", kernel=kern, aw=aw)
        for ch in chains:
            cons(f"{name} CH {ch}", kernel=kern, chain=ch)
        cons(f"{name} SP 1", kernel=kern, sp=1)
    cons("wide_pair pairs", kernel=4, pairs=1, r4=1, six=1)
    # membership (memo_debug_last_membership): the algorithms; the planes' T, MW and SK
    memb("membership doubling", algorithm=2, mw=-1)
    memb("membership runs", algorithm=3, mw=-1)
    for t in (64, 256):
        memb(f"membership planes T {t}", algorithm=4, threads=t)
    for mw in (0, 2, 3, 4, 8):
        memb(f"membership planes MW {mw}", algorithm=4, mw=mw)
    for mw in (0, 2):
        memb(f"membership dense planes MW {mw}", algorithm=5, mw=mw)
    for algo in (4, 5):
        for sk in (0, 1):
            memb(f"membership algorithm {algo} SK {sk}", algorithm=algo, sk=sk)
    # the other query forms
    req.append(("membership slice", "slice", {}))
    for form in ("oneshot_cons", "oneshot_memb"):
        for way in (0, 1, 2):
            req.append((f"{form} way {way}", form, {"way": way}))
    return req


REQUIRED = _required()


@pytest.fixture(scope="module")
def memo():
    """the package on the A/B library (product objects + memo_debug.o): the kernel-shape switches, the records of the picks"""
    import memo_amd
    from memo_amd import _lib
    memo_amd.build()
    assert _lib.lib().memo_device_count() > 0, "no HIP device: the product has no CPU fallback"
    _lib.use_ab(True)
    yield memo_amd
    _lib.use_ab(False)


class _Blocks:
    """runs a block once, for whichever test asks first, and keeps its ledger"""

    def __init__(self, memo, oracle):
        self.memo, self.oracle, self.done, self.device_error = memo, oracle, {}, None

    def __call__(self, b):
        if b in self.done:
            return self.done[b]
        if self.device_error:                                  # (nothing more is started on a device that reported an error)
            pytest.fail(f"not run: an earlier block ended in a device error\n{self.device_error}")
        from memo_amd import _lib
        ledger, failures, queries, t0 = [], [], 0, time.perf_counter()
        for i in range(b * PER_BLOCK, (b + 1) * PER_BLOCK):
            L = sweep_lives.seeded_life(sweep_lives.SEED, i)
            try:
                queries += sweep_lives.run_life(self.memo, self.oracle, L, ledger, name=f"seed {sweep_lives.SEED} life {i}")
            except sweep_lives.LifeFailure as exc:
                failures.append(exc)
                if getattr(exc.__cause__, "code", None) == _lib.MEMO_EHIP:
                    self.device_error = str(exc)
                    break
        counts = collections.Counter((form, tuple(sorted(pick.items()))) for form, pick in ledger)
        self.done[b] = dict(counts=counts, failures=failures, queries=queries, seconds=time.perf_counter() - t0)
        print(f"block {b}: {queries} queries in {self.done[b]['seconds']:.1f} s, {len(failures)} failures")
        return self.done[b]


@pytest.fixture(scope="module")
def blocks(memo, oracle):
    return _Blocks(memo, oracle)


def reached(counts):
    """per REQUIRED entry: how many queries of the ledger it was reached by"""
    hits = []
    for name, form, fields in REQUIRED:
        want = set(fields.items())
        hits.append(sum(n for (f, items), n in counts.items() if f == form and want <= set(items)))
    return hits


@pytest.mark.parametrize("b", range(BLOCKS))
def test_block_equals_the_oracle(blocks, b):
    """every answer of the block's lives equals the oracle's, exactly; every IndexError is the oracle's; a refusal only where the index
    holds the dense rows alone and memo_dense_rows_can_answer says 0; nothing else is raised (tests/sweep_lives.py: run_life)"""
    got = blocks(b)
    assert not got["failures"], "\n\n".join(str(f) for f in got["failures"])


def test_every_pick_is_reached(blocks):
    """the union of the blocks' ledgers holds every entry of REQUIRED (blocks not yet run are run); prints the count per pick.

    Queries per pick measured on an MI355X, in REQUIRED's order (129 entries; the smallest: 2 for the dense planes' MW 2, 6 for
    halo3t's LIVE and for the clipped kernel on format 12 with uint8 results):
      clipped     795 216 30 108 84 17 45 | W 351 145 475 186 138 | T 704 591 | fmt x OutT 233 562 118 128 6 186 14 48
      halo        170 136 14 160 | T 153 208 119 | TOP 309 131 40
      r4           80 50 12 58 | T 58 86 56 | TOP 124 48 28
      mixed       121 70 9 97 | T 94 137 66 | TOP 200 70 27
      halo3       T 13 23 20 | OutT 9 47 | A9 22 34
      halo3t      N 15 56 84 95 129 56 | OutT 175 260 | A9 339 96 | AW 205 230 | SIX 307 128 | SP 93 342 | LIVE 429 6 | R4 421 14 |
                  A9 x AW x SP 20 38 8 30
      wide_args   OutT 14 23 | AW 9 28 | CH 11 12 14 | SP 37
      wide        OutT 37 40 | AW 13 64 | CH 11 19 10 37 | SP 77
      wide_pair   OutT 80 48 | AW 31 97 | CH 128 | SP 128 | pairs 128
      membership  doubling 414, runs 712 | planes T 86 375 | MW 295 79 10 48 29 | dense planes MW 21 2 | SK 241 220, 12 11
      slices 339 | one-shot conservation by way 73 70 96, membership 45 42 46"""
    counts, seconds, queries = collections.Counter(), [], 0
    for b in range(BLOCKS):
        got = blocks(b)
        counts.update(got["counts"])
        seconds.append(got["seconds"])
        queries += got["queries"]
    hits = reached(counts)
    print(f"{LIVES} lives, {BLOCKS} blocks, {queries} queries; seconds per block: " + " ".join(f"{s:.1f}" for s in seconds))
    for (name, form, _), n in zip(REQUIRED, hits):
        print(f"  {n:6d}  {form:12s} {name}")
    refused = sum(n for (f, _), n in counts.items() if f == "refused")
    print(f"  {refused:6d}  refused (dense rows alone, memo_dense_rows_can_answer 0)")
    missed = [name for (name, _, _), n in zip(REQUIRED, hits) if not n]
    assert not missed, f"{len(missed)} picks of {len(REQUIRED)} not reached: {missed}"
    assert np.isfinite(seconds).all()
