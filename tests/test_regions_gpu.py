"""`memo regions` on the GPU: the run kernels (memo_amd/csrc/memo_runs.hip) against NumPy on the host, the window route against
the sweeps and the goldens, the command line against `memo query`.

The oracle everywhere: a boundary is a position whose key differs from the key before it --
np.flatnonzero(np.r_[True, key[1:] != key[:-1]]) -- with the position before the window counting as outside a band.  Every
comparison is exact."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import golden_util as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "memo")
SMALL = (0, 1, 2, 7, 8, 9, 63, 64, 65, 255, 256, 257)
KINDS = ("equal", "alternating", "rand4", "rand501", "at8", "at64", "atT", "near8", "near64", "nearT")
DOCS = (1, 32, 33, 64, 100, 130, 500)          # W = 1, 1, 2, 2, 4, 5 (rows off the 16-byte grid), 16


@pytest.fixture(scope="module")
def memo():
    import memo_amd
    from memo_amd import _lib
    memo_amd.build()                     # make: a no-op when libmemo_amd.so is up to date
    assert _lib.lib().memo_device_count() > 0, "no HIP device: the product has no CPU fallback"
    return memo_amd


# ---------------------------------------------------------------------------------------
# the oracle, and the vectors
# ---------------------------------------------------------------------------------------
def value_boundaries(key):
    """starts of the maximal runs of a vector, or of the rows of a matrix"""
    key = np.asarray(key)
    if len(key) == 0:
        return np.zeros(0, np.int64)
    differs = key[1:] != key[:-1]
    if key.ndim == 2:
        differs = differs.any(axis=1)
    return np.flatnonzero(np.r_[True, differs]).astype(np.int64)


def band_boundaries(vec, lo, hi):
    inside = (np.asarray(vec) >= lo) & (np.asarray(vec) <= hi)
    return np.flatnonzero(np.r_[False, inside][1:] != np.r_[False, inside][:-1]).astype(np.int64)


def lengths(T):
    return SMALL + (T - 1, T, T + 1, 2 * T - 1, 2 * T + 1)


def symbols(kind, L, T, seed=0):
    """a vector of small integers with the run structure `kind` names; the at* / near* kinds alternate 0 and 1, so that every run
    boundary is a band boundary of [1, 1] too"""
    rng = np.random.default_rng([seed, L, KINDS.index(kind)])
    if kind == "equal":
        return np.full(L, 3, np.int64)
    if kind == "alternating":
        return np.arange(L, dtype=np.int64) & 1
    if kind in ("rand4", "rand501"):
        return rng.integers(0, 4 if kind == "rand4" else 501, L)
    step = {"8": 8, "64": 64, "T": T}[kind.lstrip("atner")]
    flag = np.zeros(L + 2, bool)
    marks = np.arange(step, L + 2, step)
    if kind.startswith("at"):
        flag[marks] = True
    else:
        flag[marks - 1] = True
        flag[marks[marks + 1 < L + 2] + 1] = True
    return np.cumsum(flag[:L]) & 1


BAND_OF = {"equal": (3, 3), "alternating": (1, 1), "rand4": (1, 2), "rand501": (100, 300)}


def rows_of(sym, num_docs, seed=1):
    """membership rows [L, W]: one row per symbol value, bits at or above num_docs 0; symbols 0 and 1 differ only in bit num_docs - 1"""
    from memo_amd.index import words
    W = words(num_docs)
    rng = np.random.default_rng([seed, num_docs])
    table = rng.integers(0, 2 ** 32, (502, W), dtype=np.uint64).astype(np.uint32)
    if num_docs & 31:
        table[:, -1] &= np.uint32((1 << (num_docs & 31)) - 1)
    table[1] = table[0]
    table[1, -1] ^= np.uint32(1 << ((num_docs - 1) & 31))
    return np.ascontiguousarray(table[np.asarray(sym)])


# ---------------------------------------------------------------------------------------
# kernels: every length around the load, the wave, the tile; every run structure; the three keys
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_value_and_band_runs_equal_numpy(memo, kind):
    from memo_amd import regions
    T = regions.tile()
    assert T >= 512 and T % 64 == 0
    lo, hi = BAND_OF.get(kind, (1, 1))
    for L in lengths(T):
        vec = symbols(kind, L, T).astype(np.uint16)
        starts, values = regions.runs(vec)
        want = value_boundaries(vec)
        assert starts.dtype == np.int64 and values.dtype == np.uint16
        assert np.array_equal(starts, want) and np.array_equal(values, vec[want]), (kind, L)
        assert np.array_equal(regions.expand(starts, values, L), vec)
        got = regions.runs(vec, "band", lo, hi)
        assert got.dtype == np.int64 and np.array_equal(got, band_boundaries(vec, lo, hi)), (kind, L, lo, hi)
    if kind == "alternating":                            # the largest output there is: every position a run
        assert len(starts) == 2 * T + 1


@pytest.mark.parametrize("num_docs", DOCS)
@pytest.mark.parametrize("kind", KINDS)
def test_membership_runs_equal_numpy(memo, kind, num_docs):
    from memo_amd import regions
    from memo_amd.index import words
    W = words(num_docs)
    T = regions.tile(W)
    assert T >= 512 and T % 64 == 0
    for L in lengths(T):
        bits = rows_of(symbols(kind, L, T), num_docs)
        starts, run_bits = regions.membership_runs(bits, num_docs)
        want = value_boundaries(bits)
        assert run_bits.shape == (len(want), W) and run_bits.dtype == np.uint32
        assert np.array_equal(starts, want) and np.array_equal(run_bits, bits[want]), (kind, num_docs, L)


def test_more_tiles_than_one_round_of_the_scan(memo):
    """about one boundary in ten; totals cross tile bases.  The scan takes 1024 tiles a round: 3 * 2^21 positions are the 768 tiles
    of conservation values, so a vector of 1024 tiles and a half is run too"""
    from memo_amd import regions
    T = regions.tile()
    for L in (3 << 21, 1024 * T + T // 2 + 3):
        rng = np.random.default_rng(L)
        vec = (np.cumsum(rng.random(L) < 0.1) % 7).astype(np.uint16)
        want = value_boundaries(vec)
        assert len(want) > L // 11
        starts, values = regions.runs(vec)
        assert np.array_equal(starts, want) and np.array_equal(values, vec[want])
        assert np.array_equal(regions.runs(vec, "band", 2, 4), band_boundaries(vec, 2, 4))
    assert (1024 * T + T // 2 + 3 + T - 1) // T > 1024


def test_more_membership_tiles_than_one_round_of_the_scan(memo):
    from memo_amd import regions
    L, num_docs = 1 << 21, 100                           # W = 4
    assert L // regions.tile(4) > 1024
    rng = np.random.default_rng(5)
    bits = rows_of(np.cumsum(rng.random(L) < 0.1) % 400, num_docs)
    want = value_boundaries(bits)
    starts, run_bits = regions.membership_runs(bits, num_docs)
    assert np.array_equal(starts, want) and np.array_equal(run_bits, bits[want])


# ---------------------------------------------------------------------------------------
# bands
# ---------------------------------------------------------------------------------------
def test_band_cases(memo):
    from memo_amd import regions
    N = 12
    rng = np.random.default_rng(3)
    vec = rng.integers(0, N + 1, 5000).astype(np.uint16)
    for lo, hi in ((4, 4), (0, 0), (N, N), (3, 9)):
        assert np.array_equal(regions.runs(vec, "band", lo, hi), band_boundaries(vec, lo, hi)), (lo, hi)
    assert regions.runs(vec, "band", 0, N).tolist() == [0]                        # one interval, closed by L
    assert regions.runs(np.zeros(0, np.uint16), "band", 0, N).tolist() == []      # or none
    assert regions.runs(vec, "band", N + 1, 65535).tolist() == []
    inside_first, outside_first = np.array([5, 5, 1, 5, 1, 1], np.uint16), np.array([1, 5, 5, 1, 1, 5, 5], np.uint16)
    assert regions.runs(inside_first, "band", 5, 5).tolist() == [0, 2, 3, 4]       # even: every interval closed
    assert regions.runs(outside_first, "band", 5, 5).tolist() == [1, 3, 5]         # odd: the last interval ends at L
    begin, end = regions.band_intervals(regions.runs(outside_first, "band", 5, 5), len(outside_first))
    assert begin.tolist() == [1, 5] and end.tolist() == [3, 7]


def test_a_band_no_value_lies_in_returns_no_buffers(memo):
    from memo_amd._lib import check, lib
    vec = np.arange(3000, dtype=np.uint16) % 7
    d_vec = C.c_void_p()
    check(lib().memo_dev_malloc(0, vec.nbytes, C.byref(d_vec)))
    try:
        check(lib().memo_dev_upload(0, d_vec, vec.ctypes.data, vec.nbytes, None))
        d_starts, d_values, n = C.c_void_p(1), C.c_void_p(1), C.c_uint64(99)
        check(lib().memo_runs_conservation_dev(d_vec, len(vec), 1, 8, 20, C.byref(d_starts), C.byref(d_values), C.byref(n), 0, None))
        assert (d_starts.value, d_values.value, n.value) == (None, None, 0)
        d_starts, d_values, n = C.c_void_p(1), C.c_void_p(1), C.c_uint64(99)
        check(lib().memo_runs_conservation_dev(d_vec, 0, 0, 0, 0, C.byref(d_starts), C.byref(d_values), C.byref(n), 0, None))
        assert (d_starts.value, d_values.value, n.value) == (None, None, 0)        # L = 0: nothing launched, no runs
        assert lib().memo_runs_conservation_dev(d_vec, len(vec), 1, 5, 4, C.byref(d_starts), None, C.byref(n), 0, None) == -1
        assert lib().memo_runs_conservation_dev(d_vec, len(vec), 2, 0, 0, C.byref(d_starts), C.byref(d_values), C.byref(n), 0, None) == -1
    finally:
        lib().memo_dev_free(0, d_vec)


# ---------------------------------------------------------------------------------------
# membership rows
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_docs", DOCS)
def test_rows_that_differ_in_one_place_only(memo, num_docs):
    from memo_amd import regions
    from memo_amd.index import words
    W, L = words(num_docs), 3001
    rng = np.random.default_rng(num_docs)
    base = rows_of(np.full(L, 7), num_docs)
    flip = rng.random(L) < 0.2
    last_bit = base.copy()                               # bit num_docs - 1 and no other
    last_bit[flip, -1] ^= np.uint32(1 << ((num_docs - 1) & 31))
    last_word = base.copy()                              # any bits of the last word below num_docs, the words before it equal
    mask = np.uint32((1 << (num_docs & 31)) - 1) if num_docs & 31 else np.uint32(0xFFFFFFFF)
    last_word[flip, -1] ^= rng.integers(1, 2 ** 32, int(flip.sum()), dtype=np.uint64).astype(np.uint32) & mask
    for bits in (last_bit, last_word):
        want = value_boundaries(bits)
        starts, run_bits = regions.membership_runs(bits, num_docs)
        assert np.array_equal(starts, want) and np.array_equal(run_bits, bits[want]) and run_bits.shape[1] == W
    assert len(value_boundaries(last_bit)) > 500


# ---------------------------------------------------------------------------------------
# what the kernels may read
# ---------------------------------------------------------------------------------------
def test_misaligned_vector_is_refused_before_any_launch(memo):
    from memo_amd import regions
    from memo_amd._lib import MEMO_EINVAL, MemoError, check, lib
    d = C.c_void_p()
    check(lib().memo_dev_malloc(0, 4096, C.byref(d)))
    try:
        assert d.value % 16 == 0
        for call in (lambda: regions.runs((d.value + 2, 100)), lambda: regions.runs((d.value + 2, 100), "band", 0, 3),
                     lambda: regions.membership_runs((d.value + 4, 100), 40)):
            with pytest.raises(MemoError) as exc:
                call()
            assert exc.value.code == MEMO_EINVAL and "16-byte aligned" in str(exc.value)
    finally:
        lib().memo_dev_free(0, d)


def _inside_a_larger_buffer(host, before, after):
    """device pointer of `host` uploaded between 64 bytes of `before` and 64 bytes of `after`; the buffer to free"""
    from memo_amd._lib import check, lib
    whole = np.concatenate([np.full(64 // host.itemsize, before, host.dtype), host.reshape(-1), np.full(64 // host.itemsize, after, host.dtype)])
    d = C.c_void_p()
    check(lib().memo_dev_malloc(0, whole.nbytes, C.byref(d)))
    check(lib().memo_dev_upload(0, d, whole.ctypes.data, whole.nbytes, None))
    return d.value + 64, d


def test_nothing_before_or_behind_the_vector_is_used(memo):
    """the vector lies inside a larger buffer whose bytes on either side would make a boundary (and lie inside the band): the result
    is still the oracle's"""
    from memo_amd import regions
    from memo_amd._lib import lib
    T = regions.tile()
    for L in (1, 7, 9, 63, 65, 257, T - 1, T + 1, 2 * T - 3):
        vec = np.full(L, 2, np.uint16)
        vec[L // 2:] = 3
        ptr, d = _inside_a_larger_buffer(vec, 9, 9)
        try:
            starts, values = regions.runs((ptr, L))
            assert np.array_equal(starts, value_boundaries(vec)) and np.array_equal(values, vec[starts]), L
            for lo, hi in ((9, 9), (3, 3), (2, 9)):      # nothing inside; 9 behind would close at L; 9 before would hide the opening at 0
                assert np.array_equal(regions.runs((ptr, L), "band", lo, hi), band_boundaries(vec, lo, hi)), (L, lo, hi)
        finally:
            lib().memo_dev_free(0, d)
    for num_docs in (20, 40, 100, 130):
        Tm = regions.tile((num_docs + 31) // 32)
        for L in (1, 3, 5, 63, 65, Tm - 1, Tm + 1):
            bits = rows_of(np.full(L, 5), num_docs)
            ptr, d = _inside_a_larger_buffer(bits, 0xFFFF, 0xFFFF)
            try:
                starts, run_bits = regions.membership_runs((ptr, L), num_docs)
                assert starts.tolist() == [0] and np.array_equal(run_bits, bits[:1]), (num_docs, L)
            finally:
                lib().memo_dev_free(0, d)


# ---------------------------------------------------------------------------------------
# end to end: the window route against the sweeps and the goldens
# ---------------------------------------------------------------------------------------
CONS_INDEXES = ("example_cons.parquet", "rnd_n8.parquet", "rnd_n40.parquet", "rnd_n130.parquet", "rnd_n70_sparse.parquet",
                "rnd_negoverlap.parquet")


def _swept(c):
    """DeviceIndex.conservation / .membership of the case's window"""
    from memo_amd import memo_query
    rec, qs, qe = G.region(c)
    with memo_query.region_index(os.path.join(G.GOLD, c["index"]), rec, qs, qe + c["k"], device=0, k=c["k"], num_docs=c["n"],
                                 membership=c["membership"]) as ix:
        return (ix.membership if c["membership"] else ix.conservation)(qs, qe, c["k"], c["n"])


@pytest.mark.parametrize("index", CONS_INDEXES)
def test_region_runs_expand_to_the_sweep(memo, index):
    from memo_amd import regions
    cases = [c for c in G.cases(membership=False, raises=False) if c["index"] == index]
    assert cases
    for c in cases:
        path, n = os.path.join(G.GOLD, index), c["n"]
        vec = _swept(c)
        assert np.array_equal(vec, G.load(c)["vec"]), c["name"]
        r = regions.region_runs(path, c["region"], c["k"], n)
        rec, qs, qe = G.region(c)
        assert (r.record, r.qs, r.L, r.run_bits) == (rec, qs, len(vec), None)
        assert np.array_equal(r.starts, value_boundaries(vec)) and np.array_equal(regions.expand(r.starts, r.values, r.L), vec), c["name"]
        for lo, hi in ((n, None), (None, 0), (max(n // 3, 1), max(2 * n // 3, 1))):      # -t N, -T 0, a middle band
            b = regions.region_runs(path, c["region"], c["k"], n, lo=lo, hi=hi)
            want = band_boundaries(vec, 0 if lo is None else lo, n if hi is None else hi)
            assert b.values is None and np.array_equal(b.starts, want), (c["name"], lo, hi)


def test_region_runs_of_membership_expand_to_the_sweep(memo):
    from memo_amd import regions
    cases = [c for c in G.cases(membership=True, raises=False) if c["index"] == "example_memb.parquet"]
    assert cases
    for c in cases:
        bits = _swept(c)
        r = regions.region_runs(os.path.join(G.GOLD, c["index"]), c["region"], c["k"], c["n"], membership=True)
        assert r.values is None and r.L == len(bits)
        assert np.array_equal(r.starts, value_boundaries(bits)) and np.array_equal(regions.expand(r.starts, r.run_bits, r.L), bits), c["name"]


def test_region_runs_raise_what_memo_query_raises(memo):
    from memo_amd import regions
    path = os.path.join(G.GOLD, "example_cons.parquet")
    with pytest.raises(ValueError):
        regions.region_runs(path, "ref_1:20-0", 3, 5)
    with pytest.raises(ValueError):
        regions.region_runs(path, "ref_1:0:20", 3, 5)
    with pytest.raises(IndexError):                      # the sweep's own: an annot outside the result columns
        regions.region_runs(path, "ref_1:0-20", 3, 2)
    with pytest.raises(ValueError):
        regions.region_runs(os.path.join(G.GOLD, "example_memb.parquet"), "ref_1:0-20", 3, 5, membership=True, lo=1)


def test_a_window_that_starts_past_2_to_the_32(memo):
    from memo_amd import regions
    qs, L = 2 ** 32 + 5, 1000
    vec = (np.arange(L) // 37 % 6).astype(np.uint16)
    starts, values = regions.runs(vec)
    ends = np.append(starts[1:], L)
    text = bytes(regions.emit_runs("chrFar", qs, L, starts, values))
    want = "".join(f"chrFar\t{qs + s}\t{qs + e}\t{v}\n" for s, e, v in zip(starts.tolist(), ends.tolist(), values.tolist()))
    assert text == want.encode() and text.startswith(b"chrFar\t4294967301\t4294967338\t0\n")
    band = regions.runs(vec, "band", 5, 5)
    begin, end = regions.band_intervals(band, L)
    assert int(end[-1]) == L or vec[-1] != 5
    want = "".join(f"chrFar\t{qs + s}\t{qs + e}\n" for s, e in zip(begin.tolist(), end.tolist()))
    assert bytes(regions.emit_runs("chrFar", qs, L, band)) == want.encode()


# ---------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------
def _memo(*argv, env=None):
    return subprocess.run([sys.executable, EXE, *argv], capture_output=True, timeout=300, env=dict(os.environ, **(env or {})))


def _expand_bedgraph(data, membership=False):
    """the lines `memo query` writes for the same window: the value (the characters, a blank between them) once per position"""
    out, at = [], None
    for line in data.decode().splitlines():
        rec, start, end, value = line.split("\t")
        assert rec == "ref_1" and (at is None or int(start) == at) and int(end) > int(start)
        at = int(end)
        out.append(((" ".join(value) if membership else value) + "\n") * (int(end) - int(start)))
    return "".join(out).encode()


def test_cli_writes_what_memo_query_writes_run_coded(memo, tmp_path):
    cons, memb = (os.path.join(G.GOLD, f) for f in ("example_cons.parquet", "example_memb.parquet"))
    q, r = str(tmp_path / "q.txt"), str(tmp_path / "r.bed")
    common = ("-r", "ref_1:0-20", "-k", "3", "-n", "5")
    assert _memo("query", "-b", cons, *common, "-o", q).returncode == 0
    got = _memo("regions", "-b", cons, *common, "-o", r)
    assert (got.returncode, got.stdout) == (0, b"MEMO - regions\n"), got.stderr
    text = open(r, "rb").read()
    assert _expand_bedgraph(text) == open(q, "rb").read() and text.count(b"\n") < 20
    vec = np.array(open(q).read().split(), np.int64)
    # -t 5 on the five-genome example: the intervals of value 5
    assert _memo("regions", "-b", cons, *common, "-o", r, "-t", "5").returncode == 0
    begin, end = (band_boundaries(vec, 5, 5).tolist() + [20])[0::2], (band_boundaries(vec, 5, 5).tolist() + [20])[1::2]
    assert open(r).read() == "".join(f"ref_1\t{b}\t{e}\n" for b, e in zip(begin, end)) and begin
    assert _memo("regions", "-b", cons, *common, "-o", r, "-T", "2", "-t", "1").returncode == 0
    got = [tuple(map(int, ln.split("\t")[1:])) for ln in open(r).read().splitlines()]
    inside = (vec >= 1) & (vec <= 2)
    assert sorted(p for b, e in got for p in range(b, e)) == np.flatnonzero(inside).tolist()
    # membership
    assert _memo("query", "-m", "-b", memb, *common, "-o", q).returncode == 0
    assert _memo("regions", "-m", "-b", memb, *common, "-o", r).returncode == 0
    assert _expand_bedgraph(open(r, "rb").read(), membership=True) == open(q, "rb").read()
    # an empty window: an empty file (memo query: the reference's lone newline)
    assert _memo("regions", "-b", cons, "-r", "ref_1:7-7", "-k", "3", "-n", "5", "-o", r).returncode == 0
    assert open(r, "rb").read() == b""


def test_cli_refusals(memo, tmp_path):
    cons = os.path.join(G.GOLD, "example_cons.parquet")
    out = str(tmp_path / "never.bed")
    common = ("-b", cons, "-r", "ref_1:0-20", "-k", "3", "-n", "5", "-o", out)
    for extra, env, message in ((("-m", "-t", "3"), None, b"-m cannot be combined"), (("-t", "6"), None, b"-t must be an integer in [0, 5]"),
                                (("-T", "x"), None, b"-T must be an integer in [0, 5]"), (("-t", "4", "-T", "3"), None, b"-t 4 is above -T 3"),
                                ((), {"WORLD_SIZE": "2"}, b"sharded"), ((), {"MEMO_FORCE_SHARDED": "1"}, b"sharded")):
        r = _memo("regions", *common, *extra, env=env)
        assert r.returncode == 1 and message in r.stderr and r.stderr.startswith(b"memo regions: "), (extra, r.stderr)
        assert r.stdout == b"MEMO - regions\n" and not os.path.exists(out)
    r = _memo("regions", "-b", cons, "-r", "ref_1:20-0", "-k", "3", "-n", "5", "-o", out)      # what memo query raises, as a message
    assert r.returncode == 1 and b"negative dimensions" in r.stderr and not os.path.exists(out)
    r = _memo("regions", "-b", cons, "-r", "ref_1:0-20", "-k", "3", "-n", "2", "-o", out)
    assert r.returncode == 1 and b"IndexError" in r.stderr and os.listdir(tmp_path) == []
