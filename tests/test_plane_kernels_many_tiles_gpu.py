"""`memo matrix`, `memo collect` and `memo tracks` where MANY genomes meet MANY tiles: more than one genome word, and every workgroup
taking a run of several tiles with its counts alive across them -- the crossing of the two axes that the kernels' own suites walk one at
a time (num_docs > 32 only up to 2 T + 1 rows there, many tiles only at num_docs = 8).

The three kernels (memo_cooc.hip, memo_collect.hip, memo_tracks.hip; `memo features -m` reaches the third) stage per-genome bit planes
in LDS tile after tile (memo_planes.h) and keep 32-bit counts in registers or LDS over all their tiles.  What runs here for the first
time with more than one genome word:
  - the staging rotation blk = (tid + 64 (t & 3)) & 255 at every t & 3, followed by another tile that overwrites the planes behind
    the second barrier;
  - cooc_kernel<2> with its 32 accumulators over several tiles, gy > 1 (the vwave rotation, a triangle workgroup's shortened
    `staged`), the scratch cap of the partials, cooc_reduce_kernel's loop at gx > 16, and the launches of num_docs > 512 taking the
    scratch in turn;
  - collect_kernel<16> at gy > 1, <8> and <4> with their LDS accumulators read and written tile after tile; the batching of orders
    in memo_collect_dev (batch < P, gx_cap);
  - tracks_kernel<16,1>, <16,2>, <8,4>, <4,8> with a bin's counts staying in registers from tile to tile, and their search for a
    workgroup's first bin.

Every case derives its launch shape here, by the launchers' own arithmetic on constants named after their source lines, and asserts
the regime before it calls the device: a changed constant fails the case and cannot move it out of its regime unseen.  The references
are tests/planes_oracle.py's (on the packed rows; held against the definitions by tests/test_planes_oracle_cpu.py).  Every comparison
is exact.

Left out on purpose:
  - cooc_kernel<1> (KU = 1) over many tiles with several genome words: at num_docs = 513 the thin chunk launches (64, 64 and 1 units)
    stay at one tile a workgroup, because their cap is kMaxGridX and 1024 tiles of 17 words behind the full launches' two tiles would
    not pass in seconds.  KU = 1 with many tiles is the ground of test_matrix_gpu's num_docs = 8 test.
  - kMaxTilesPerWg (2^22 tiles a workgroup, 2^31 positions): out of reach of a test of seconds.
  - memo_tracks_dev's reachable instances are the four above: PW follows the genome words and KG the genomes, so <16,4>, <8,1> and the
    like cannot be launched."""
import functools

import numpy as np
import pytest

from tests import planes_oracle as PO
from tests.test_tracks_gpu import Resident

pytestmark = pytest.mark.gpu

kThreads = 256                           # memo_cooc.hip, memo_collect.hip, memo_tracks.hip: lanes of a workgroup
kTile = 512                              # memo_cooc.hip: positions per tile
kMaxStaged = 16                          # memo_cooc.hip: genome words a launch stages at most
kMaxGridX = 1024                         # all three: workgroups along the positions at most
kScratchCap = 64 << 20                   # memo_cooc.hip, memo_collect.hip: bytes of partials at most
kLdsBudget = 120 << 10                   # memo_collect.hip: LDS of the planes and a block of orders at most
kStepChunk = 8                           # memo_collect.hip: steps a lane takes at a time
kPlaneBlockPitch = 36                    # memo_planes.h: LDS words from one staged genome word to the next
R = 77                                   # the ragged tail
ORIGIN = 1_000_003                       # `first` of the tracks cases: no multiple of anything


def position_words(W):                   # memo_collect.hip, memo_tracks.hip
    return 16 if W <= 16 else 8 if W <= 32 else 4


def cdiv(a, b):
    return -(-a // b)


def words(N):
    return cdiv(N, 32)


@pytest.fixture(scope="module")
def memo():
    import memo_amd
    from memo_amd import _lib
    memo_amd.build()                     # make: a no-op when libmemo_amd.so is up to date
    assert _lib.lib().memo_device_count() > 0, "no HIP device: the product has no CPU fallback"
    return memo_amd


def same(got, want):
    return got.dtype == np.uint64 and got.shape == want.shape and np.array_equal(got.astype(np.int64), want)


# ---------------------------------------------------------------------------------------
# the rows: generated once for each (genomes, length), and never written to afterwards
# ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def structured_rows(L, N, T):
    """(rows, {name: genome}): densities from 1/8 to 63/64 genome by genome, and planes_oracle.structure's eight columns"""
    levels = np.random.default_rng([1, N]).choice(np.array([-3, -2, -1, 1, 2, 3, 6]), N)
    bits = PO.density_rows(L, N, levels, seed=1)
    at = PO.structure(bits, N, T)
    bits.setflags(write=False)
    return bits, at


@functools.lru_cache(maxsize=None)
def conserved_rows(L, N):
    """densities from 7/8 to 63/64 and one position in 16 that holds every genome: a long order's core does not die out"""
    levels = np.random.default_rng([2, N]).choice(np.array([3, 4, 5, 6]), N)
    bits = PO.density_rows(L, N, levels, seed=2, conserved=4)
    bits.setflags(write=False)
    return bits


# ---------------------------------------------------------------------------------------
# matrix
# ---------------------------------------------------------------------------------------
def matrix_launches(L, N, partials=True):
    """memo_cooccurrence_dev and plan() of memo_cooc.hip: one dict per launch, in launch order"""
    W = words(N)
    cw = W if W <= kMaxStaged else kMaxStaged // 2
    chunks, ntiles = cdiv(W, cw), cdiv(L, kTile)
    groups = lambda w0, nw: (min(N - 32 * w0, 32 * nw) + 3) // 4
    out = []
    for ca in range(chunks):
        for cb in range(ca, chunks):
            nwa = min(cw, W - ca * cw)
            n4a = groups(ca * cw, nwa)
            nwb = min(cw, W - cb * cw) if cb != ca else 0
            units = n4a * groups(cb * cw, nwb) if cb != ca else n4a * (n4a + 1) // 2
            ku = 1 if units <= kThreads else 2
            gy = cdiv(units, kThreads * ku)
            slots = gy * kThreads * ku
            scratch_cap = max(1, kScratchCap // (slots * 64))
            cap = min(kMaxGridX, ntiles, scratch_cap) if partials else min(kMaxGridX, ntiles)
            per = cdiv(ntiles, cap)
            out.append(dict(staged=nwa + nwb, rectangle=cb != ca, units=units, ku=ku, gy=gy, scratch_cap=scratch_cap, per=per,
                            gx=cdiv(ntiles, per)))
    return out


def matrix_structure_holds(want, at, L, T):
    """the reference alone: what the structured columns say about the matrix"""
    d = np.diag(want)
    assert np.array_equal(want[at["everywhere"]], d) and d[at["everywhere"]] == L
    assert not want[at["absent"]].any() and not want[:, at["absent"]].any()
    assert d[at["tile_ends"]] == L // T and d[at["tail"]] == L % T == R and want[at["tile_ends"], at["tail"]] == 0
    assert np.array_equal(want[at["twin_a"]], want[at["twin_b"]]) and want[at["twin_a"], at["twin_b"]] == d[at["twin_a"]]
    assert want[at["mirror_a"], at["mirror_b"]] == 0 and d[at["mirror_a"]] + d[at["mirror_b"]] == L
    assert np.array_equal(want, want.T) and len(np.unique(d)) > len(d) // 2


#                N, runs of `cap` tiles, whole tiles more, per, the atomic flush too
MATRIX_CASES = ((100, 2, 2, 3, True),
                (100, 4, 2, 5, True),
                (500, 2, 2, 3, False),
                (500, 4, 3, 5, False))


@pytest.mark.parametrize("N,runs,more,per,atomics", MATRIX_CASES)
def test_matrix_one_launch_many_tiles(memo, N, runs, more, per, atomics):
    """cooc_kernel<2>, its 32 accumulators a lane alive over per = 3 and per = 5 tiles; per = 5 is every value of t & 3 in the staging
    rotation and the first again, each tile's planes overwritten by the next behind the second barrier.
      N = 100: W = 4, the staging is one wave's work and rotates over the waves; gy = 1; kMaxGridX bounds gx, not the scratch.  Both
               flushes: partials + cooc_reduce_kernel (its loop x += 16 takes 43 and 52 steps: gx = 684, 820), and the 64-bit atomics
               of memo_debug_cooc_flush.
      N = 500: W = 16, gy = 16: the vwave rotation by blockIdx.x, the triangle workgroups of small blockIdx.y staging fewer words than
               16 tile after tile; the scratch cap (128 < kMaxGridX) binds; gx = 87 and 104 > 16 in cooc_reduce_kernel.
    Then a second call into the first one's counts: twice the matrix.
    The reference (planes_oracle.cooccurrence) took 0.3 s, 0.7 s, 1.4 s and 0.5 s on the eight CPU cores this was written on."""
    from memo_amd import _lib, matrix
    W, T = words(N), matrix.tile(words(N))
    assert T == kTile
    cap = min(kMaxGridX, matrix_launches(T, N)[0]["scratch_cap"])
    L = (runs * cap + more) * T + R
    (launch,) = matrix_launches(L, N)
    assert launch["per"] == per and launch["ku"] == 2 and not launch["rectangle"] and L % T == R
    if N == 100:
        assert W == 4 and W * (kTile // 32) <= 64 and launch["gy"] == 1 and launch["scratch_cap"] > kMaxGridX == cap
        assert launch["gx"] == cdiv(cdiv(L, T), per) > 16 * 40
    else:
        assert W == kMaxStaged and launch["gy"] == 16 and launch["scratch_cap"] == cap == 128 < kMaxGridX
        assert launch["gx"] == {3: 87, 5: 104}[per] > 16
    assert matrix_launches(L, N, partials=False)[0]["per"] == (per if N == 100 else 1)
    bits, at = structured_rows(L, N, T)
    want = PO.cooccurrence(bits, N)
    matrix_structure_holds(want, at, L, T)
    with Resident(bits) as rows:
        first = matrix.cooccurrence(rows.part(0, L), N)
        assert same(first, want), "partials"
        assert same(matrix.cooccurrence(rows.part(0, L), N, counts=first), 2 * want), "a second call adds to the first one's counts"
        if not atomics:
            return
        _lib.use_ab(True)
        try:
            _lib.check(_lib.lib().memo_debug_cooc_flush(1))
            got = matrix.cooccurrence(rows.part(0, L), N, counts=first)
            _lib.check(_lib.lib().memo_debug_cooc_flush(0))
            assert same(got, 2 * want), "atomics"
            assert same(matrix.cooccurrence(rows.part(0, L), N), want), "partials, from the A/B library"
        finally:
            _lib.lib().memo_debug_cooc_flush(0)
            _lib.use_ab(False)


def test_matrix_chunked_launches_share_the_scratch_over_two_tiles(memo):
    """N = 513: 17 genome words in chunks of 8 + 8 + 1, six launches that take the one scratch buffer in turn, each followed by its
    cooc_reduce_kernel.  Both full triangles (scratch cap 409) and the full rectangle (cap 256) take two tiles a workgroup, gx = 206;
    the three thin launches (64, 64 and 1 units, KU = 1) stay at one tile (the module's docstring says why).  Then a second call into
    the first one's counts.  The reference took 0.4 s."""
    from memo_amd import matrix
    N = 513
    T = matrix.tile(words(N))
    assert T == kTile and words(N) == kMaxStaged + 1
    caps = [l["scratch_cap"] for l in matrix_launches(T, N)]
    L = (caps[0] + 2) * T + R
    launches = matrix_launches(L, N)
    ntiles = cdiv(L, T)
    assert [(l["staged"], l["rectangle"], l["units"], l["ku"]) for l in launches] == [
        (8, False, 2080, 2), (16, True, 4096, 2), (9, True, 64, 1), (8, False, 2080, 2), (9, True, 64, 1), (1, False, 1, 1)]
    assert [l["scratch_cap"] for l in launches] == caps == [409, 256, 4096, 409, 4096, 4096]
    assert [l["per"] for l in launches] == [2, 2, 1, 2, 1, 1]
    assert [l["gx"] for l in launches] == [206, 206, ntiles, 206, ntiles, ntiles] and ntiles <= kMaxGridX
    assert [l["gy"] for l in launches] == [5, 8, 1, 5, 1, 1]
    bits, at = structured_rows(L, N, T)
    want = PO.cooccurrence(bits, N)
    matrix_structure_holds(want, at, L, T)
    assert want[:512, 512].any() and want[512, 512] > 0                             # the thin launches have something to count
    with Resident(bits) as rows:
        first = matrix.cooccurrence(rows.part(0, L), N)
        assert same(first, want)
        assert same(matrix.cooccurrence(rows.part(0, L), N, counts=first), 2 * want), "a second call adds to the first one's counts"


# ---------------------------------------------------------------------------------------
# collect
# ---------------------------------------------------------------------------------------
def collect_launch(L, N, P, M):
    """memo_collect_dev of memo_collect.hip"""
    W = words(N)
    pw = position_words(W)
    ntiles = cdiv(L, 32 * pw)
    Mp = cdiv(M, kStepChunk) * kStepChunk
    plane_bytes, order_bytes = pw * (kPlaneBlockPitch * W + 4) * 4, Mp * (8 + 2)
    ob = min(kThreads // pw, P, max(1, (kLdsBudget - plane_bytes) // order_bytes))
    step_bytes = M * 2 * 4
    gx_cap = max(1, kScratchCap // (step_bytes * min(P, 256)))
    per = cdiv(ntiles, min(kMaxGridX, ntiles, gx_cap))
    gx = cdiv(ntiles, per)
    batch = min(P, kScratchCap // (step_bytes * gx))
    if batch < P:
        batch = batch // ob * ob
    return dict(pw=pw, ob=ob, lds=plane_bytes + ob * order_bytes, gx_cap=gx_cap, per=per, gx=gx, batch=batch,
                gy=[cdiv(min(batch, P - q0), ob) for q0 in range(0, P, batch)])


def orders_from_every_word(N, P, M, seed):
    """P orders of M distinct genomes drawn from all N, so from every genome word"""
    rng = np.random.default_rng([seed, N, P, M])
    table = np.array([rng.permutation(N)[:M] for _ in range(P)])
    if N - 1 not in table[0]:
        table[0, M // 2] = N - 1                             # (the last word may hold one genome)
    assert len(np.unique(table >> 5)) == words(N)
    return table


def collect_case(memo, L, N, P, M):
    """the curves of conserved_rows(L, N) over P orders of M steps against the reference, into seeded outputs"""
    from memo_amd import collect
    bits = conserved_rows(L, N)
    table = orders_from_every_word(N, P, M, seed=3)
    core, covered = PO.curves(bits, N, table)
    # the reference alone: the curves carry information
    assert core[:, -1].max() > 0 and covered[:, 0].max() < L and len(np.unique(core, axis=0)) >= 2 and len(np.unique(covered, axis=0)) >= 2
    assert (np.diff(core, axis=1) <= 0).all() and (np.diff(covered, axis=1) >= 0).all() and (core <= covered).all()
    cell = np.arange(P * M, dtype=np.uint64).reshape(P, M)
    # no two rows of the seeds alike: a batch that adds into the wrong rows shows
    seed_core, seed_covered = 3 * cell + 1, np.uint64(2 ** 32 - 5) + 7 * cell
    got = collect.curves(bits, N, table, core=seed_core, covered=seed_covered)
    assert same(got[0] - seed_core, core), "core"
    assert same(got[1] - seed_covered, covered), "covered"


#                 N, P, M, runs of `cap` tiles, whole tiles more, per, PW, gy
COLLECT_CASES = ((100, 65, 99, 2, 2, 3, 16, 5),
                 (100, 65, 99, 4, 2, 5, 16, 5),
                 (513, 5, 130, 2, 2, 3, 8, 1),
                 (1030, 5, 130, 2, 2, 3, 4, 1))


@pytest.mark.parametrize("N,P,M,runs,more,per,pw,gy", COLLECT_CASES)
def test_collect_one_batch_many_tiles(memo, N, P, M, runs, more, per, pw, gy):
    """collect_kernel<16> at gy = 5 (65 orders in blocks of 16, the last block one order), <8> and <4>: the LDS accumulators of every
    (order, step) are read and written again tile after tile, over per = 3 tiles, and at N = 100 over per = 5: every value of t & 3 in
    the staging rotation and the first again, with W = 4 (one wave stages) -- and with 17 and 33 words (every lane stages, some two
    blocks a tile).  One batch, kMaxGridX bounds gx.  The reference (planes_oracle.curves) took 0.9 s, 2.6 s, 1.0 s and 0.9 s."""
    from memo_amd import collect
    T = collect.tile(words(N))
    assert T == 32 * pw == 32 * position_words(words(N))
    L = (runs * kMaxGridX + more) * T + R
    launch = collect_launch(L, N, P, M)
    assert launch["pw"] == pw and launch["per"] == per and launch["gx"] == cdiv(cdiv(L, T), per) and launch["gx_cap"] > kMaxGridX
    assert launch["batch"] == P and launch["gy"] == [gy] and launch["ob"] == min(kThreads // pw, P) and launch["lds"] <= 64 << 10
    collect_case(memo, L, N, P, M)


#                  N, P, M, tiles = 2 gx_cap + this, per, gx, batch, ob
BATCHED_CASES = ((100, 300, 100, 0, 2, 327, 256, 16),
                 (2048, 400, 2048, 2, 3, 12, 340, 4))


@pytest.mark.parametrize("N,P,M,more,per,gx,batch,ob", BATCHED_CASES)
def test_collect_batches_of_orders_many_tiles(memo, N, P, M, more, per, gx, batch, ob):
    """the batching of memo_collect_dev: batch < P, the loop for (q0 ...; q0 += batch) twice with a partial last batch, the batches
    taking the partials in turn and adding into their own rows of core and covered (seeded, no two rows alike).
      N = 100, 300 orders of 100 steps: gx_cap = 327 binds (below kMaxGridX and the tiles), two tiles a workgroup, batches of 256 and 44
      N = 2048, 400 orders of 2048 steps: PW = 4, ob = 4 by kLdsBudget, batch = 341 / 4 * 4 = 340 and 60; 116 KiB of LDS, above the
                64 KiB a launch gets without asking; gx_cap = 16 binds, three tiles a workgroup
    The reference took 0.8 s and 0.4 s."""
    from memo_amd import collect
    T = collect.tile(words(N))
    assert T == 32 * position_words(words(N))
    gx_cap = collect_launch(T, N, P, M)["gx_cap"]
    L = (2 * gx_cap - 1 + more) * T + R
    launch = collect_launch(L, N, P, M)
    assert launch["gx_cap"] == gx_cap < min(kMaxGridX, cdiv(L, T)), "gx_cap binds"
    assert (launch["per"], launch["gx"], launch["batch"], launch["ob"]) == (per, gx, batch, ob)
    assert launch["batch"] < P and launch["batch"] % launch["ob"] == 0 and len(launch["gy"]) == 2 and P % launch["batch"]
    assert launch["gy"] == [batch // ob, cdiv(P - batch, ob)]
    assert (launch["lds"] > 64 << 10) == (N == 2048) and launch["lds"] <= kLdsBudget
    collect_case(memo, L, N, P, M)


# ---------------------------------------------------------------------------------------
# tracks
# ---------------------------------------------------------------------------------------
def tracks_launch(L, N):
    """memo_tracks_dev of memo_tracks.hip"""
    pw = position_words(words(N))
    ntiles = cdiv(L, 32 * pw)
    per = cdiv(ntiles, min(kMaxGridX, ntiles))
    kg = cdiv(N, kThreads)
    return dict(pw=pw, kg=1 if kg <= 1 else 2 if kg <= 2 else 4 if kg <= 4 else 8, per=per, gx=cdiv(ntiles, per))


def hand_made_edges(L, run, T, seed):
    """(edges in slice coordinates, k, the narrow stretch [lo, hi) across the start of run k and its first tile boundary).  From left
    to right: two edges before the rows; two bins several runs wide; 200 bins about a tile wide; an edge exactly on a run boundary;
    0- to 40-position bins, a third of them empty, from 300 positions before a run boundary to 300 behind the tile boundary that
    follows it; a wide bin; narrow bins again over the last 500 positions, the ragged tail among them; three edges behind the rows."""
    rng = np.random.default_rng([seed, L, run])
    assert run >= 2 * T

    def narrow(lo, hi):
        steps = rng.integers(0, 41, 2 * (hi - lo) // 20 + 50)
        steps[rng.random(len(steps)) < 1 / 3] = 0
        at = lo + np.cumsum(steps)
        return [lo] + at[at < hi].tolist()
    edges = [-1000, -5, int(7.3 * run) + 11, 13 * run - 9]
    tile_wide = edges[-1] + np.cumsum(np.resize(np.array([T - 1, T, T + 1, T + 40, T - 40]), 200))
    edges += tile_wide.tolist()
    boundary = (cdiv(edges[-1], run) + 1) * run
    edges.append(boundary)                                   # exactly on a run boundary
    k = boundary // run + 3
    lo, hi = k * run - 300, k * run + T + 300
    assert boundary < lo and edges[-2] < boundary and hi < L - 10 * run
    edges += narrow(lo, hi)
    edges.append(hi + 3 * run + 5)
    edges += narrow(L - 500, L)
    edges += [L + 3, L + 3, L + 2000]
    edges = np.asarray(edges, np.int64)
    assert (np.diff(edges) >= 0).all() and edges[0] < 0 and edges[-1] > L
    inside = edges[(edges > lo) & (edges < hi)]
    assert (np.diff(inside) == 0).sum() >= 10 and np.diff(inside).max() <= 40          # empty bins among the narrow ones
    assert ((inside > k * run - 40) & (inside < k * run + 40)).sum() >= 1             # ... across the two workgroups' runs
    assert ((inside > k * run + T - 40) & (inside < k * run + T + 40)).sum() >= 1     # ... and across a tile boundary inside a run
    return edges, k, (lo, hi)


def cut_inside_a_narrow_bin(edges, stretch, W, after):
    """a row strictly inside a bin of the narrow stretch, behind `after`: no multiple of 32 rows, but 16-byte aligned in rows of W words"""
    for cut in range(after + 1, stretch[1]):
        b = np.searchsorted(edges, cut, side="right") - 1
        if edges[b] < cut < edges[b + 1] <= edges[b] + 40 and cut % 32 and (cut * W * 4) % 16 == 0:
            return cut
    raise AssertionError("no cut")


def tracks_shape(N, runs):
    from memo_amd import tracks
    T = tracks.tile(words(N))
    assert T == 32 * position_words(words(N))
    return T, (runs * kMaxGridX + 2) * T + R


#                N, runs of kMaxGridX tiles, per, PW, KG
TRACKS_CASES = ((100, 2, 3, 16, 1),
                (100, 4, 5, 16, 1),
                (300, 2, 3, 16, 2),
                (513, 2, 3, 8, 4),
                (1100, 2, 3, 4, 8))


@pytest.mark.parametrize("N,runs,per,pw,kg", TRACKS_CASES)
def test_tracks_every_instance_many_tiles(memo, N, runs, per, pw, kg):
    """tracks_kernel<16,1> with W = 4 (one wave stages, and rotates) at per = 3 and per = 5 (every t & 3, and the first again),
    <16,2> (W = 10), <8,4> (W = 17) and <4,8> (W = 35): KG counts a lane that stay in registers from one tile to the next when a bin
    goes on, and leave once when it ends; the binary search for a workgroup's first bin among empty bins and on an edge that is the
    workgroup's first position.  One table of hand-made edges (hand_made_edges) with `first` = 1 000 003.  Whole, then as two slices
    cut inside a narrow bin behind a run boundary, at a row that is no multiple of 32 but 16-byte aligned, the second slice into the
    counts of the first.  The reference (planes_oracle.tracks) took 1.5 s, 2.8 s, 3.6 s, 2.6 s and 2.2 s."""
    from memo_amd import tracks
    T, L = tracks_shape(N, runs)
    W = words(N)
    launch = tracks_launch(L, N)
    assert (launch["pw"], launch["kg"], launch["per"]) == (pw, kg, per) and launch["gx"] == cdiv(cdiv(L, T), per) and L % T == R
    run = per * T
    edges, k, stretch = hand_made_edges(L, run, T, seed=4)
    assert len(edges) < 4000
    bits, at = structured_rows(L, N, T)
    want = PO.tracks(bits, N, edges + ORIGIN, first=ORIGIN)
    # the reference alone
    sums = PO.column_counts(bits, N)
    assert np.array_equal(want.sum(axis=1), sums), "every set bit lies in one bin"
    assert sums[at["everywhere"]] == L and sums[at["absent"]] == 0 and sums[at["tile_ends"]] == L // T and sums[at["tail"]] == R
    assert np.array_equal(want[at["everywhere"]], np.diff(np.clip(edges, 0, L))) and np.array_equal(want[at["twin_a"]], want[at["twin_b"]])
    assert np.array_equal(want[at["mirror_a"]] + want[at["mirror_b"]], want[at["everywhere"]])
    cut = cut_inside_a_narrow_bin(edges, stretch, W, after=k * run)
    assert cut % 32 and cut % T and (cut * W * 4) % 16 == 0 and tracks_launch(L - cut, N)["per"] >= 2
    with Resident(bits) as rows:
        assert same(tracks.bin_tracks(rows.part(0, L), N, edges + ORIGIN, first=ORIGIN), want), "whole"
        head = tracks.bin_tracks(rows.part(0, cut), N, edges + ORIGIN, first=ORIGIN)
        both = tracks.bin_tracks(rows.part(cut, L), N, edges + ORIGIN, first=ORIGIN + cut, counts=head)
        assert same(both, want), "two slices"
        b = np.searchsorted(edges, cut, side="right") - 1
        assert not head[:, b + 1:].any() and np.array_equal(head[:, :b], both[:, :b]) and head[at["everywhere"], b] == cut - edges[b]


def test_features_segments_as_bins_many_tiles(memo):
    """`memo features -m`: memo_tracks_dev as memo_amd/features.py calls it -- the segments between the endpoints of overlapping,
    nested and repeated features as its bins, `first` the least start, into a zeroed table on the device -- and memo_feature_sums_dev
    behind it.  N = 300: tracks_kernel<16,2> over three tiles a workgroup.  Against planes_oracle.tracks summed per feature (3.9 s)."""
    import ctypes as C
    from memo_amd import features
    from memo_amd._device import DevBuffer
    from memo_amd._lib import check, lib
    N = 300
    T, L = tracks_shape(N, 2)
    launch = tracks_launch(L, N)
    assert (launch["pw"], launch["kg"], launch["per"]) == (16, 2, 3)
    run = launch["per"] * T
    rng = np.random.default_rng(5)
    F = 1500
    starts = rng.integers(0, L - 1, F)
    length = np.choose(rng.integers(0, 4, F), [rng.integers(1, 41, F), rng.integers(T - 40, T + 41, F), rng.integers(run, 6 * run, F),
                                               rng.integers(1, 41, F)])
    ends = np.minimum(starts + length, L)
    starts[:3], ends[:3] = (0, 0, 10 * run), (L, L, 10 * run + 1)                 # the whole window, twice; one position on a run boundary
    starts[3:6] = (5 * run - 100, 5 * run - 50, 5 * run - 50)                      # nested, repeated
    ends[3:6] = (5 * run + T + 100, 5 * run + 50, 5 * run + 50)
    starts, ends = starts + ORIGIN, ends + ORIGIN
    edges, lo, hi = features.segments(starts, ends)
    qs, qe, segs = int(edges[0]), int(edges[-1]), len(edges) - 1
    assert (qs, qe) == (ORIGIN, ORIGIN + L) and 2000 < segs <= 2 * F - 1 and (hi - lo).max() == segs and (hi - lo > 3).sum() > F // 8
    bits, at = structured_rows(L, N, T)
    per_segment = PO.tracks(bits, N, edges, first=qs)
    cum = np.concatenate([np.zeros((N, 1), np.int64), np.cumsum(per_segment, axis=1)], axis=1)
    want = (cum[:, hi] - cum[:, lo]).T
    assert np.array_equal(want[:, at["everywhere"]], ends - starts) and np.array_equal(want[0], PO.column_counts(bits, N))
    with Resident(bits) as rows, DevBuffer.of(np.zeros((N, segs), np.uint64), 0) as d_table, DevBuffer(0, 8 * F * N) as d_out:
        check(lib().memo_tracks_dev(C.c_void_p(rows.d.value), qe - qs, N, qs, edges.ctypes.data, segs, d_table.d, 0, None))
        assert same(d_table.to_host((N, segs), np.uint64), per_segment), "the segment table"
        features._feature_sums(d_table.d, N, segs, lo, hi, d_out.d, 0)
        assert same(d_out.to_host((F, N), np.uint64), want), "the feature table"
