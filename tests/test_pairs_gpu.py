"""`memo pairs` on the GPU: the kernel (memo_amd/csrc/memo_pairs.hip) against NumPy on the host, the window route against `memo matrix`
and `memo breaks` on the device, the command line against the README's tables.

The oracle is tests/pairs_oracle.py; every comparison is exact."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import golden_util as G
from tests import pairs_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "memo")
CAP_MAX = 2 ** 31 - 1
MEMB = os.path.join(G.GOLD, "example_memb.parquet")
GROUP, UNITS_PER_WG = 8, 64                                    # genomes a group, units a workgroup (memo_pairs.hip: kGroup, kUnitsPerWg)
GRID_X = 1024                                                   # runs of tiles at most (memo_pairs.hip: kMaxGridX)
POISON = 0xFFFFFFFF
GUARD = 64                                                      # words around a poisoned buffer, and behind L in its planes


@pytest.fixture(scope="module")
def memo():
    import memo_amd
    from memo_amd import _lib
    memo_amd.build()                     # make: a no-op when libmemo_amd.so is up to date
    assert _lib.lib().memo_device_count() > 0, "no HIP device: the product has no CPU fallback"
    return memo_amd


@pytest.fixture(scope="module")
def consts(memo):
    """(T, C, S*): the tile, the most genomes of one launch, the largest narrow span"""
    from memo_amd import pairs
    T, Cn, S = pairs.tile(), pairs.chunk(), pairs.narrow_span()
    assert T % 4 == 0 and Cn % GROUP == 0 and S == (2 ** 32 - 1) // T and S * T < 2 ** 32 <= (S + 1) * T
    return T, Cn, S


def same(got, want, note=None):
    assert got.dtype == np.uint64 and got.shape == want.shape, (note, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert not len(bad), (note, bad[:5].tolist(), [int(got[tuple(i)]) for i in bad[:5]], [int(want[tuple(i)]) for i in bad[:5]])


def poisoned(cells):
    """(DevBuffer, the tuple plane_sums takes): the planes at pitch = L rounded up to 4, + 64, every word of [L, pitch) and 64 words
    before and behind the planes 0xFFFFFFFF -- read, they would count as kmax"""
    from memo_amd._device import DevBuffer
    from memo_amd.lengths import pitch_of
    cells = np.asarray(cells, np.uint32)
    planes, L = cells.shape
    pitch = pitch_of(L) + GUARD
    host = np.full(GUARD + planes * pitch + GUARD, POISON, np.uint32)
    host[GUARD:GUARD + planes * pitch].reshape(planes, pitch)[:, :L] = cells
    buf = DevBuffer.of(host, 0)
    return buf, (buf.d.value + 4 * GUARD, L, pitch, planes)


def both(v, kmin, kmax, sums=None):
    """the kernel on a host array (pitch = L rounded up to 4) and on the poisoned layout: the two matrices, equal"""
    from memo_amd import pairs
    v = np.asarray(v, np.uint32)
    tight = pairs.plane_sums(v, kmin=kmin, kmax=kmax, sums=sums)
    buf, where = poisoned(v)
    with buf:
        loose = pairs.plane_sums(where, kmin=kmin, kmax=kmax, sums=sums)
    same(loose, tight, ("poisoned", v.shape, kmin, kmax))
    return tight


def by_levels(v, kmin, kmax):
    """the same matrix as the oracle's, for small spans, as the sum over k of the 0/1 co-occurrences (identity 2, in float64 -- exact
    below 2^53): what keeps 2048 genomes' reference quick"""
    w = O.weights(v, kmin, kmax)
    out = np.zeros((len(w), len(w)))
    for t in range(1, int(w.max(initial=0)) + 1):
        b = (w >= t).astype(np.float64)
        out += b @ b.T
    return out.astype(np.uint64)


def ramps(rng, planes, L, mean=40):
    """lengths as an index leaves them: falling ramps between random breaks"""
    v = np.empty((planes, L), np.int64)
    for g in range(planes):
        ends = np.flatnonzero(rng.random(L) < 1.0 / mean)
        nxt = np.append(ends, L + mean)[np.searchsorted(ends, np.arange(L), side="left")]
        v[g] = nxt - np.arange(L)
    return v.astype(np.uint32)


# ---------------------------------------------------------------------------------------
# the kernel against the oracle
# ---------------------------------------------------------------------------------------
def test_every_genome_count_at_every_length(memo, consts):
    T, Cn, _ = consts
    first_two_wgs = next(n for n in range(1, Cn) if ((n + GROUP - 1) // GROUP) * ((n + GROUP - 1) // GROUP + 1) // 2 > UNITS_PER_WG)
    assert first_two_wgs == 81
    rng = np.random.default_rng(20261021)
    calls = 0
    for n in (1, 2, 3, 4, 5, 8, 9, 33, 100, first_two_wgs - 1, first_two_wgs, Cn, Cn + 1):
        for L in (0, 1, 3, 4, 5, T - 1, T, T + 1, 2 * T + 1):
            v = rng.integers(0, 5, (n, L)).astype(np.uint32)
            kmin, kmax = ((1, 4), (2, 4), (3, 3))[calls % 3]
            want = O.sums(v, kmin, kmax)
            same(both(v, kmin, kmax), want, (n, L, kmin, kmax))
            assert np.array_equal(want, by_levels(v, kmin, kmax))
            calls += 1
    assert calls == 13 * 9


def test_2048_genomes(memo, consts):
    T, _, _ = consts
    rng = np.random.default_rng(2048)
    v = rng.integers(0, 5, (2048, T + 1)).astype(np.uint32)
    v[7], v[2047] = 4, v[1000]                                      # a genome that holds everything, two that are identical
    got = both(v, 1, 4)
    same(got, by_levels(v, 1, 4), 2048)
    w = v.astype(np.int64)
    assert np.array_equal(np.diag(got), w.sum(axis=1).astype(np.uint64)) and np.array_equal(got[7], np.diag(got)) and got[2047, 1000] == got[1000, 1000]
    same(got[:40, 2000:], O.sums(np.vstack([v[:40], v[2000:]]), 1, 4)[:40, 40:], "against the oracle itself")


def test_many_tiles_a_workgroup_and_a_tail(memo, consts):
    """N = 8: more than two tiles for each of the grid's runs, and a last tile of five positions; with a span of S* every tile's 32-bit
    sums are added to the partials in memory, with half of it every second tile's"""
    T, _, S = consts
    rng = np.random.default_rng(8)
    L = (2 * GRID_X + 3) * T + 5
    small = rng.integers(0, 5, (8, L)).astype(np.uint32)
    same(both(small, 1, 4), O.sums(small, 1, 4), "small")
    big = rng.integers(0, S + 9, (8, L)).astype(np.uint32)
    big[3] = S + 7                                                  # every cell above the cap: the 32-bit sums are full at every tile
    big[5] = big[3]
    for kmin, kmax in ((1, S), (1, S // 2), (S // 2, S - 1), (1, S + 1)):
        same(both(big, kmin, kmax), O.sums(big, kmin, kmax), (kmin, kmax))


def _packed(present):
    """membership rows uint32 [L, W] of a boolean [N, L]"""
    n, L = present.shape
    bits = np.zeros((L, (n + 31) // 32), np.uint32)
    for g in range(n):
        bits[:, g // 32] |= present[g].astype(np.uint32) << np.uint32(g % 32)
    return bits


@pytest.mark.parametrize("n", (9, 33))
def test_contents(memo, consts, n):
    from memo_amd import matrix
    T, _, _ = consts
    rng = np.random.default_rng([3, n])
    L, cap = 2 * T + 1, 12
    disjoint = np.zeros((n, L), np.uint32)
    disjoint[np.arange(L) % n, np.arange(L)] = rng.integers(1, cap + 1, L)         # a position is held by one genome only
    identical = np.tile(rng.integers(0, cap + 1, L).astype(np.uint32), (n, 1))
    above = rng.integers(0, 3 * cap, (n, L)).astype(np.uint32)
    above[0] = POISON                                                               # cells above the cap, the largest word among them
    inputs = {"zeros": np.zeros((n, L), np.uint32), "at the cap": np.full((n, L), cap, np.uint32), "above the cap": above,
              "in [0, 4]": rng.integers(0, 5, (n, L)).astype(np.uint32), "ramps": ramps(rng, n, L), "identical": identical, "disjoint": disjoint}
    for name, v in inputs.items():
        for kmin, kmax in ((1, cap), (cap, cap), (5, cap), (2, 2)):
            got = both(v, kmin, kmax)
            same(got, O.sums(v, kmin, kmax), (name, kmin, kmax))
            assert np.array_equal(got, got.T), name                                 # symmetric, and the diagonal is the genome's own weight
            assert np.array_equal(np.diag(got), O.weights(v, kmin, kmax).sum(axis=1).astype(np.uint64)), name
            if kmin == kmax:                                                        # weights of 0 and 1: `memo matrix`'s kernel on the packed bits
                same(got, matrix.cooccurrence(_packed(v >= kmin), n), (name, "cooccurrence", kmin))
    z = both(inputs["zeros"], 1, cap)
    assert not z.any() and (both(inputs["at the cap"], 1, cap) == L * cap).all() and (both(inputs["at the cap"], 5, cap) == L * (cap - 4)).all()
    d = both(disjoint, 1, cap)
    assert np.array_equal(d, np.diag(np.diag(d))) and d.any()
    i = both(identical, 1, cap)
    assert (i == i[0, 0]).all() and i[0, 0] == identical[0].sum()


def test_both_sides_of_the_narrow_span(memo, consts):
    """the same cells at spans S* - 1, S* (the last narrow one), S* + 1 and 2^31 - 1 (wide), from kmin = 1 and up to kmax = 2^31 - 1;
    with every cell at the cap a pair's sum passes 2^32 inside one workgroup"""
    T, _, S = consts
    rng = np.random.default_rng(31)
    L = 2 * T + 1
    v = rng.integers(0, 2 ** 31, (10, L)).astype(np.uint32)
    v[1] = np.where(rng.random(L) < 0.5, v[1], rng.integers(0, 2 * S, L)).astype(np.uint32)      # (values on both sides of S* too)
    v[2] = rng.integers(0, 2 ** 32, L, dtype=np.uint64).astype(np.uint32)
    full = np.full((9, L), CAP_MAX, np.uint32)
    for span in (S - 1, S, S + 1, CAP_MAX):
        for kmin, kmax in ((1, span), (CAP_MAX - span + 1, CAP_MAX)):
            same(both(v, kmin, kmax), O.sums(v, kmin, kmax), (span, kmin))
            got = both(full, kmin, kmax)
            assert (got == L * span).all(), (span, kmin)
    assert L * CAP_MAX > 2 ** 32 and L * S > 2 ** 32


def test_the_matrix_is_added_to_and_slices_accumulate(memo, consts):
    T, _, S = consts
    rng = np.random.default_rng(13)
    n, L = 11, 2 * T + 40
    v = ramps(rng, n, L)
    for kmin, kmax in ((1, 31), (3, CAP_MAX)):
        want = O.sums(v, kmin, kmax)
        for seed in (2 ** 32 - 5, 2 ** 62):
            before = np.full((n, n), seed, np.uint64)
            same(both(v, kmin, kmax, sums=before), before + want, (kmin, kmax, seed))
        wraps = rng.integers(0, 2 ** 63, (n, n), dtype=np.int64).astype(np.uint64) * np.uint64(2)      # (the adds are modulo 2^64)
        same(both(v, kmin, kmax, sums=wraps), wraps + want, "wraps")
        for cut in (1, T - 1, T, L // 2, L - 1):                                    # two parts of the positions against the whole
            same(both(v[:, cut:], kmin, kmax, sums=both(v[:, :cut], kmin, kmax)), want, (kmin, kmax, cut))


def test_refusals_and_empty_calls_leave_the_matrix_as_it_was(memo):
    from memo_amd import _lib
    from memo_amd._device import DevBuffer
    L_ = _lib.lib()
    v = np.arange(96, dtype=np.uint32).reshape(3, 32) % 7
    before = np.arange(9, dtype=np.uint64).reshape(3, 3) + np.uint64(7)
    big = 2 ** 31
    with DevBuffer.of(v, 0) as cells, DevBuffer.of(np.append(before.ravel(), np.uint64(0)), 0) as sums:
        d, t = cells.d.value, sums.d.value
        ok = dict(d=d, L=32, pitch=32, planes=3, kmin=1, kmax=6, t=t)

        def call(**kw):
            a = dict(ok, **kw)
            return L_.memo_pairs_dev(a["d"], a["L"], a["pitch"], a["planes"], a["kmin"], a["kmax"], a["t"], 0, None)
        refused = (dict(d=d + 4), dict(d=d + 8), dict(d=None), dict(pitch=34, L=30), dict(pitch=28), dict(L=big + 1, pitch=big + 4), dict(L=-1),
                   dict(planes=-1), dict(planes=2049), dict(kmax=0), dict(kmax=2 ** 31), dict(kmax=2 ** 32 - 1), dict(kmin=0), dict(kmin=7),
                   dict(kmin=2 ** 31, kmax=2 ** 31), dict(t=None), dict(t=t + 4))
        for kw in refused:
            assert call(**kw) == _lib.MEMO_EINVAL, kw
            assert L_.memo_last_error(), kw
            assert np.array_equal(sums.to_host(before.shape, np.uint64), before), kw
        # nothing to add: nothing is launched, the matrix stays
        for kw in (dict(L=0), dict(planes=0), dict(L=0, d=None, pitch=0), dict(planes=0, d=None), dict(L=0, planes=0)):
            assert call(**kw) == _lib.MEMO_OK, kw
            assert np.array_equal(sums.to_host(before.shape, np.uint64), before), kw
        # and the call as it stands is taken
        assert call() == _lib.MEMO_OK
        same(sums.to_host(before.shape, np.uint64), before + O.sums(v, 1, 6), "taken")
        assert call(pitch=36, L=30, planes=1, t=t + 8) == _lib.MEMO_OK and call(kmin=6) == _lib.MEMO_OK


def test_the_lap_timer_is_the_ab_library_s(memo):
    from memo_amd import _lib, pairs
    assert not hasattr(_lib.lib(), "memo_debug_pairs_times")
    ab = _lib.use_ab(True)
    try:
        ms = (C.c_float * 2)()
        assert ab.memo_debug_pairs_times(1, ms) == 0
        v = np.ones((2, 5000), np.uint32)
        assert pairs.plane_sums(v, kmax=4).tolist() == [[5000, 5000], [5000, 5000]]
        assert ab.memo_debug_pairs_times(0, ms) == 0 and ms[0] > 0.0 and ms[1] > 0.0
    finally:
        _lib.use_ab(False)


# ---------------------------------------------------------------------------------------
# region_pairs
# ---------------------------------------------------------------------------------------
def _usable_windows():
    """(index, region, n, the k the goldens ask of it) of every membership golden window whose index has only rows with end >= start"""
    out = {}
    for c in G.cases(raises=False, membership=True):
        rec, _, _ = G.region(c)
        s, e, _ = G.index_columns(c["index"], rec)
        if (e >= s).all():
            out.setdefault((c["index"], c["region"], c["n"]), set()).add(int(c["k"]))
    return [(*key, sorted(ks)) for key, ks in sorted(out.items())]


def test_identity_1_on_every_golden_window(memo):
    """S(k, k) is `memo matrix -k k`'s matrix, at the goldens' own k and at others up to three a window"""
    from memo_amd import matrix, pairs
    windows = _usable_windows()
    assert sum(len(ks) for *_, ks in windows) == 139
    checked = 0
    for index, region, n, ks in windows:
        path = os.path.join(G.GOLD, index)
        for k in (ks + [k for k in (3, 31, 64) if k not in ks])[:3]:
            same(pairs.region_pairs(path, region, n, kmin=k, kmax=k), matrix.region_matrix(path, region, k, n), (index, region, k))
            checked += 1
    assert checked == 3 * len(windows)


def test_identities_2_and_3_on_the_example(memo):
    from memo_amd import breaks, matrix, pairs
    whole = pairs.region_pairs(MEMB, "ref_1:0-20", 5, kmax=8)
    assert whole.tolist() == [[160, 52, 82, 83, 64], [52, 52, 49, 51, 49], [82, 49, 82, 72, 61], [83, 51, 72, 83, 61], [64, 49, 61, 61, 64]]
    same(whole, sum(matrix.region_matrix(MEMB, "ref_1:0-20", k, 5) for k in range(1, 9)), "identity 2")
    same(pairs.region_pairs(MEMB, "ref_1:0-20", 5, kmin=3, kmax=8), sum(matrix.region_matrix(MEMB, "ref_1:0-20", k, 5) for k in range(3, 9)), "identity 2, 3 .. 8")
    for region, cap in (("ref_1:0-20", 8), ("ref_1:7-19", None), ("ref_1:0-20", None)):
        table, _, _ = breaks.region_breaks(MEMB, region, 5, 1, membership=True, cap=cap)
        assert np.array_equal(np.diag(pairs.region_pairs(MEMB, region, 5, kmax=cap)), table[1, :, 0]), (region, cap)      # identity 3
    top = pairs.region_pairs(MEMB, "ref_1:0-20", 5)
    assert top[0, 0] == 42949672940 and np.array_equal(top[0], np.diag(top)) and np.array_equal(top[1:, 1:], whole[1:, 1:])
    assert not pairs.region_pairs(MEMB, "ref_1:5-5", 5).any()
    with pytest.raises(OSError):
        pairs.region_pairs(os.path.join(G.GOLD, "no_such.parquet"), "ref_1:0-20", 5)


def test_the_slices_do_not_show(memo):
    from memo_amd import pairs
    s, e, a = G.index_columns("example_memb.parquet", "ref_1")
    for region, qs, qe in (("ref_1:0-20", 0, 20), ("ref_1:3-19", 3, 19)):
        for kmin, kmax in ((1, None), (2, 6)):
            want = O.window_sums(s, e, a, qs, qe, kmin, kmax or CAP_MAX, 5)
            for step in (None, 1, 7, 64):
                same(pairs.region_pairs(MEMB, region, 5, kmin=kmin, kmax=kmax, slice_positions=step), want, (region, kmin, kmax, step))
    c = next(c for c in G.cases(membership=True, raises=False) if c["name"] == "rnd_n40_memb_k31_c0w1")
    rec, qs, qe = G.region(c)
    path = os.path.join(G.GOLD, c["index"])
    want = O.window_sums(*G.index_columns(c["index"], rec), qs, qe, 1, 300, c["n"])
    for step in (None, 64, 1000):
        same(pairs.region_pairs(path, c["region"], c["n"], kmax=300, slice_positions=step), want, (c["name"], step))


def test_a_window_past_2_to_the_32(memo, tmp_path):
    """the rows of a golden index shifted past 2^32: the matrix of the shifted window is the origin's"""
    import pyarrow as pa
    import pyarrow.parquet as pq
    from memo_amd import pairs
    c = next(c for c in G.cases(membership=True, raises=False) if c["name"] == "rnd_n40_memb_k31_c0w1")
    rec, qs, qe = G.region(c)
    s, e, o = G.index_columns(c["index"], rec)
    want = O.window_sums(s, e, o, qs, qe, 2, 300, c["n"])
    D = 2 ** 32 + 12_345
    path = str(tmp_path / "far.parquet")
    pq.write_table(pa.table({"f0": pa.array([rec] * len(s), pa.utf8()), "f1": s + D, "f2": e + D, "f3": o}), path, compression="ZSTD")
    for step in (None, 1000):
        same(pairs.region_pairs(path, f"{rec}:{qs + D}-{qe + D}", c["n"], kmin=2, kmax=300, slice_positions=step), want, step)


# ---------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------
def _memo(*argv, env=None):
    return subprocess.run([sys.executable, EXE, *argv], capture_output=True, timeout=300, env=dict(os.environ, **(env or {})))


README = {("-l", "3", "-K", "3"): "20 10 16 20 18 / 10 10 8 10 8 / 16 8 16 16 16 / 20 10 16 20 18 / 18 8 16 18 18",
          ("-l", "4", "-K", "4"): "20 2 12 12 6 / 2 2 1 1 1 / 12 1 12 10 5 / 12 1 10 12 3 / 6 1 5 3 6",
          ("-K", "8"): "160 52 82 83 64 / 52 52 49 51 49 / 82 49 82 72 61 / 83 51 72 83 61 / 64 49 61 61 64",
          ("-l", "3", "-K", "8"): "120 12 42 43 24 / 12 12 9 11 9 / 42 9 42 32 21 / 43 11 32 43 21 / 24 9 21 21 24"}


def _run(tmp_path, *flags, region="ref_1:0-20"):
    out = str(tmp_path / "p.tsv")
    r = _memo("pairs", "-b", MEMB, "-n", "5", "-r", region, "-o", out, *flags)
    assert (r.returncode, r.stdout) == (0, b"MEMO - pairs\n"), (flags, r.stderr)
    return open(out).read()


def test_cli_writes_the_readme_s_tables(memo, tmp_path):
    for flags, rows in README.items():
        assert _run(tmp_path, *flags) == "".join(row.replace(" ", "\t") + "\n" for row in rows.split(" / ")), flags
    top = [ln.split("\t") for ln in _run(tmp_path).splitlines()]                   # the default cap
    assert top[0] == ["42949672940", "52", "82", "83", "64"] and [ln[1:] for ln in top[1:]] == [r.split()[1:] for r in README[("-K", "8")].split(" / ")[1:]]
    assert _run(tmp_path, region="ref_1:5-5") == ""                                # an empty window: an empty file
    assert sorted(os.listdir(tmp_path)) == ["p.tsv"]                               # written beside its name and renamed


def test_cli_distances_means_and_labels(memo, tmp_path):
    from memo_amd import matrix
    s8 = np.array([[int(x) for x in row.split()] for row in README[("-K", "8")].split(" / ")], np.uint64)
    text = _run(tmp_path, "-K", "8", "-j")
    assert text == matrix.format_matrix(matrix.jaccard(s8))
    d = [[float(x) for x in ln.split("\t")] for ln in text.splitlines()]
    assert [round(x, 4) for x in d[1]] == [0.675, 0.0, 0.4235, 0.3929, 0.2687] and round(d[2][3], 4) == 0.2258
    assert _run(tmp_path, "-K", "8", "-f").splitlines()[:2] == ["8.0\t2.6\t4.1\t4.15\t3.2", "2.6\t2.6\t2.45\t2.55\t2.45"]
    genomes = tmp_path / "genomes.txt"
    genomes.write_text("ref/pivot.fa\nasm/g1.fa.gz\ng2.fasta\n\ng3.fa\ng4.fna\n")
    text = _run(tmp_path, "-K", "8", "-g", str(genomes))
    assert text == matrix.format_matrix(s8, ["pivot", "g1", "g2", "g3", "g4"]) and text.startswith("\tpivot\tg1\tg2\tg3\tg4\npivot\t160\t")
    never = str(tmp_path / "never.tsv")
    r = _memo("pairs", "-b", os.path.join(G.GOLD, "no_such.parquet"), "-n", "5", "-r", "ref_1:0-20", "-o", never)
    assert r.returncode == 1 and r.stderr.startswith(b"memo pairs: ") and not os.path.exists(never)
    assert sorted(os.listdir(tmp_path)) == ["genomes.txt", "p.tsv"]
