"""`memo tracks` on the GPU: the kernel (memo_amd/csrc/memo_tracks.hip) against NumPy on the host, the window route against the
goldens, the command line against the formatter.

The oracle everywhere (tests/tracks_oracle.py): B = the unpacked bits [L, N]; counts[g][b] = B[edges[b]:edges[b + 1], g].sum().
Every comparison is exact."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import golden_util as G
from tests import tracks_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "memo")
DOCS = (1, 2, 32, 33, 64, 65, 100, 513, 2048)                  # W = 1, 1, 1, 2, 2, 3, 4, 17, 64: the word reaches, the largest
GRID_X = 1024                                                   # workgroups at most (memo_tracks.hip: kMaxGridX)


@pytest.fixture(scope="module")
def memo():
    import memo_amd
    from memo_amd import _lib
    memo_amd.build()                     # make: a no-op when libmemo_amd.so is up to date
    assert _lib.lib().memo_device_count() > 0, "no HIP device: the product has no CPU fallback"
    return memo_amd


class Resident:
    """rows uploaded once; prefixes and slices of them are (device pointer, L) pairs"""

    def __init__(self, rows):
        from memo_amd._lib import check, lib
        self.rows = np.ascontiguousarray(rows, np.uint32)
        self.W = self.rows.shape[1]
        self.d = C.c_void_p()
        check(lib().memo_dev_malloc(0, max(self.rows.nbytes, 16), C.byref(self.d)))
        check(lib().memo_dev_upload(0, self.d, self.rows.ctypes.data, self.rows.nbytes, None))

    def part(self, lo, hi):
        assert (lo * self.W * 4) % 16 == 0, "a slice of the resident rows must begin 16-byte aligned"
        return (self.d.value + lo * self.W * 4, hi - lo)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        from memo_amd._lib import lib
        lib().memo_dev_free(0, self.d)


def same(got, want):
    return got.dtype == np.uint64 and got.shape == want.shape and np.array_equal(got.astype(np.int64), want)


def lengths(T):
    return tuple(sorted({1, 31, 32, 33, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1}))


def bin_counts(L):
    return tuple(sorted({b for b in (1, 2, 3, 7, L - 1, L) if 1 <= b <= L}))


# ---------------------------------------------------------------------------------------
# the kernel: every genome count around the word, every length around the word and the tile, every bin count down to one position
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_docs", DOCS)
def test_every_length_and_bin_count_equals_numpy(memo, num_docs):
    from memo_amd import tracks, view
    from memo_amd.index import words
    T = tracks.tile(words(num_docs))
    assert T >= 64 and T % 32 == 0
    Ls = lengths(T)
    B = O.random_bits(Ls[-1], num_docs, 0.5)
    with Resident(O.pack(B)) as rows:
        for L in Ls:
            for bins in bin_counts(L):
                edges = view.bin_edges(L, bins)
                assert edges[0] == 0 and edges[-1] == L and len(edges) == bins + 1
                got = tracks.bin_tracks(rows.part(0, L), num_docs, edges)
                assert same(got, O.tracks_fast(B[:L], edges)), (num_docs, L, bins)
    assert np.array_equal(O.tracks_fast(B, view.bin_edges(len(B), 7)), O.tracks(B, view.bin_edges(len(B), 7)))     # the two oracles agree


def test_tile_sizes(memo):
    from memo_amd import tracks
    assert [tracks.tile(w) for w in (1, 4, 16, 17, 32, 33, 64)] == [512, 512, 512, 256, 256, 128, 128]


@pytest.mark.parametrize("num_docs", (5, 100, 513))
def test_hand_made_edges(memo, num_docs):
    from memo_amd import tracks
    from memo_amd.index import words
    T = tracks.tile(words(num_docs))
    L = 2 * T + 1
    B = O.random_bits(L, num_docs, 0.5, seed=11)
    with Resident(O.pack(B)) as rows:
        for name, edges in (("empty bins", [0, 0, 10, 10, 10, 40, L, L]),
                            ("five edges inside one 32-position block", [0, 33, 34, 40, 41, 63, L]),
                            ("an edge at T - 1, at T and at T + 1", [0, T - 1, T, T + 1, L]),
                            ("every edge on a word", [0, 32, 64, 96, T, T + 32, L]),
                            ("before the rows and behind them", [-1000, -5, 17, L + 3, L + 3, L + 2000])):
            got = tracks.bin_tracks(rows.part(0, L), num_docs, edges)
            assert same(got, O.tracks(B, edges)), (num_docs, name)
            assert int(got.sum()) == int(B.sum()), (num_docs, name)                 # the edges cover the rows: every set bit is counted once
        # ... and with the rows somewhere inside the edges: a first that is no multiple of 32
        for first, edges in ((77, [0, 50, 77, 78, 100, 77 + T, 77 + L, 5000]), (1000003, [1000000, 1000003 + T - 1, 1000003 + L])):
            got = tracks.bin_tracks(rows.part(0, L), num_docs, edges, first=first)
            assert same(got, O.tracks(B, edges, first)) and int(got.sum()) == int(B.sum()), (num_docs, first)


@pytest.mark.parametrize("num_docs", (40, 100, 2048))
def test_slices_accumulate_to_the_whole(memo, num_docs):
    """the same window cut at 1, 31, 32, 33, T and T + 5, each slice with its `first`: the table of the whole; a slice may end inside
    a bin, and begin where no plane word begins"""
    from memo_amd import tracks, view
    from memo_amd.index import words
    W = words(num_docs)
    T = tracks.tile(W)
    L, origin = 2 * T + 41, 123457
    B = O.random_bits(L, num_docs, 0.5, seed=12)
    packed = O.pack(B)
    for bins in (1, 5, L):
        edges = view.bin_edges(L, bins) + origin
        want = O.tracks_fast(B, edges, origin)
        assert same(tracks.bin_tracks(packed, num_docs, edges, first=origin), want), (num_docs, bins)
        for cut in (1, 31, 32, 33, T, T + 5):
            head = tracks.bin_tracks(packed[:cut], num_docs, edges, first=origin)
            assert same(head, O.tracks_fast(B[:cut], edges, origin)), (num_docs, bins, cut)
            both = tracks.bin_tracks(packed[cut:], num_docs, edges, first=origin + cut, counts=head)
            assert same(both, want), (num_docs, bins, cut)


def test_counts_passed_in_are_the_starting_value(memo):
    from memo_amd import tracks, view
    num_docs, L = 70, 3 * tracks.tile(3) + 11
    B = O.random_bits(L, num_docs, 0.5, seed=13)
    edges = view.bin_edges(L, 9)
    seed = np.full((num_docs, 9), 2 ** 32 - 5, np.uint64)
    got = tracks.bin_tracks(O.pack(B), num_docs, edges, counts=seed)
    assert got.dtype == np.uint64 and np.array_equal(got, seed + O.tracks(B, edges).astype(np.uint64)) and int(got.max()) >= 2 ** 32   # a 64-bit add
    untouched = tracks.bin_tracks(O.pack(B)[:0], num_docs, [0, 0, 0, 0, 0, 0, 0, 0, 0, 0], counts=seed)
    assert np.array_equal(untouched, seed)                                         # L == 0: nothing launched


@pytest.mark.parametrize("num_docs", (1, 31, 33, 100, 513))
def test_garbage_at_or_above_num_docs_is_masked(memo, num_docs):
    from memo_amd import tracks, view
    L = tracks.tile((num_docs + 31) // 32) + 37
    B = O.random_bits(L, num_docs, 0.5, seed=3)
    clean, dirty = O.pack(B), O.pack(B, garbage=1)
    assert not np.array_equal(clean, dirty)
    edges = view.bin_edges(L, 6)
    want = O.tracks(B, edges)
    assert same(tracks.bin_tracks(clean, num_docs, edges), want) and same(tracks.bin_tracks(dirty, num_docs, edges), want)
    rnd = O.pack(B, garbage=O.random_bits(L, 32 * clean.shape[1] - num_docs, 0.5, seed=4))
    assert same(tracks.bin_tracks(rnd, num_docs, edges), want)


@pytest.mark.parametrize("num_docs", (33, 100, 300))
def test_all_zeros_and_all_ones(memo, num_docs):
    from memo_amd import tracks, view
    L = 2 * tracks.tile((num_docs + 31) // 32) + 1
    ones, zeros = np.ones((L, num_docs), np.uint8), np.zeros((L, num_docs), np.uint8)
    for bins in (1, 7, L):
        edges = view.bin_edges(L, bins)
        width = np.diff(edges)
        assert same(tracks.bin_tracks(O.pack(ones), num_docs, edges), np.tile(width, (num_docs, 1))), bins     # all ones: the bin widths
        assert same(tracks.bin_tracks(O.pack(zeros), num_docs, edges), np.zeros((num_docs, bins), np.int64)), bins
    for p in (0, L - 1):                                     # one set bit at each corner
        for g in (0, 31, 32, num_docs - 1):
            B = zeros.copy()
            B[p, g] = 1
            edges = view.bin_edges(L, 3)
            want = np.zeros((num_docs, 3), np.int64)
            want[g, 0 if p == 0 else 2] = 1
            assert same(tracks.bin_tracks(O.pack(B), num_docs, edges), want), (p, g)


def test_every_workgroup_more_than_one_tile_and_a_ragged_tail(memo):
    """2050 tiles and 77 positions: 683 workgroups of three tiles and one of one tile and the tail; wide bins (a workgroup's counts
    leave once or twice), bins about a tile wide, and bins narrower than a plane word"""
    from memo_amd import tracks, view
    num_docs = 8                                             # (a question about positions: few genomes keep the oracle quick)
    T = tracks.tile(1)
    L = (2 * GRID_X + 2) * T + 77
    per = -(-(-(-L // T)) // GRID_X)
    assert per >= 2 and (-(-L // T)) % per >= 2 and L % T
    B = O.random_bits(L, num_docs, 0.63)
    with Resident(O.pack(B)) as rows:
        assert rows.rows.nbytes < 8 << 20
        for bins in (1, 500, 2051, L // 5):
            edges = view.bin_edges(L, bins)
            got = tracks.bin_tracks(rows.part(0, L), num_docs, edges)
            assert same(got, O.tracks_fast(B, edges)), bins
            assert np.array_equal(got.sum(axis=1).astype(np.int64), B.sum(axis=0, dtype=np.int64)), bins


# ---------------------------------------------------------------------------------------
# what the kernel may read, what the call refuses
# ---------------------------------------------------------------------------------------
def test_nothing_before_or_behind_the_rows_is_read(memo):
    """the rows lie inside a larger buffer whose neighbours are all ones: the table is still the oracle's"""
    from memo_amd import tracks, view
    for num_docs in (20, 100, 1100):
        W = (num_docs + 31) // 32
        T = tracks.tile(W)
        for L in (1, 33, T - 1, T + 1):
            B = O.random_bits(L, num_docs, 0.5, seed=8)
            whole = np.concatenate([np.full(16, 0xFFFFFFFF, np.uint32), O.pack(B).reshape(-1), np.full(64 * W + 16, 0xFFFFFFFF, np.uint32)])
            with Resident(whole.reshape(1, -1)) as buf:
                edges = view.bin_edges(L, min(L, 3))
                assert same(tracks.bin_tracks((buf.d.value + 64, L), num_docs, edges), O.tracks(B, edges)), (num_docs, L)


def test_what_is_refused_before_any_launch(memo):
    """MEMO_EINVAL, and the table as it was"""
    from memo_amd._lib import MEMO_EINVAL, check, lib
    num_docs, L, bins = 40, 100, 4
    seed = np.arange(num_docs * bins, dtype=np.uint64).reshape(num_docs, bins) + 7
    good = np.array([0, 25, 50, 75, 100], np.int64)
    with Resident(np.full((L + 8, 2), 0xFFFFFFFF, np.uint32)) as rows, Resident(seed.view(np.uint32).reshape(num_docs, -1)) as table:
        assert rows.d.value % 16 == 0 and table.d.value % 8 == 0

        def call(d_bits, n, first, edges, nb, d_counts, length=L):
            edges = np.ascontiguousarray(edges, np.int64)
            return lib().memo_tracks_dev(d_bits, length, n, first, edges.ctypes.data, nb, d_counts, 0, None)
        for what, rc in (("rows 4 bytes off", call(rows.d.value + 4, num_docs, 0, good, bins, table.d)),
                         ("a table 4 bytes off", call(rows.d, num_docs, 0, good, bins, table.d.value + 4)),
                         ("no table", call(rows.d, num_docs, 0, good, bins, None)),
                         ("num_docs 0", call(rows.d, 0, 0, good, bins, table.d)),
                         ("num_docs 2049", call(rows.d, 2049, 0, good, bins, table.d)),
                         ("bins 0", call(rows.d, num_docs, 0, good, 0, table.d)),
                         ("bins above 2^20", call(rows.d, num_docs, 0, good, (1 << 20) + 1, table.d)),
                         ("decreasing edges", call(rows.d, num_docs, 0, [0, 50, 49, 75, 100], bins, table.d)),
                         ("a slice that begins before the edges", call(rows.d, num_docs, -1, good, bins, table.d)),
                         ("a slice that ends behind the edges", call(rows.d, num_docs, 1, good, bins, table.d)),
                         ("an empty slice behind the edges", call(rows.d, num_docs, 101, good, bins, table.d, length=0))):
            assert rc == MEMO_EINVAL, what
            assert lib().memo_last_error(), what
        after = np.empty_like(seed)
        check(lib().memo_dev_download(0, after.ctypes.data, table.d, after.nbytes, None))
        assert np.array_equal(after, seed)
        assert call(rows.d, num_docs, 0, good, bins, table.d) == 0               # and the same call with nothing to refuse counts
        check(lib().memo_dev_download(0, after.ctypes.data, table.d, after.nbytes, None))
        assert np.array_equal(after, seed + 25)


# ---------------------------------------------------------------------------------------
# end to end: the window route against the goldens
# ---------------------------------------------------------------------------------------
MEMB_INDEXES = sorted({c["index"] for c in G.cases(membership=True, raises=False)})


@pytest.mark.parametrize("index", MEMB_INDEXES)
def test_region_tracks_equals_the_goldens_whatever_the_slices(memo, index):
    """slices of 1, 7 and 64 positions end inside bins and at word and tile edges: the four tables are equal"""
    from memo_amd import tracks, view
    cases = [c for c in G.cases(membership=True, raises=False) if c["index"] == index]
    assert cases
    swept = 0
    for c in cases:
        _, qs, qe = G.region(c)
        L = qe - qs
        if L == 0:
            continue
        path, B = os.path.join(G.GOLD, index), G.expected_matrix(c, G.load(c))
        for bins in sorted({1, min(L, 3), min(L, 50)}):
            whole, edges = tracks.region_tracks(path, c["region"], c["k"], c["n"], bins)
            assert np.array_equal(edges, view.bin_edges(L, bins)), (c["name"], bins)
            assert same(whole, O.tracks(B, edges)), (c["name"], bins)
            for step in (1, 7, 64):
                again, _ = tracks.region_tracks(path, c["region"], c["k"], c["n"], bins, slice_positions=step)
                assert np.array_equal(again, whole), (c["name"], bins, step)
            swept += 1
    assert swept


def test_every_membership_golden_is_covered():
    assert len(MEMB_INDEXES) >= 6 and sum(1 for _ in G.cases(membership=True, raises=False)) >= 100


EXAMPLES = {(3, 4): [[5, 5, 5, 5], [3, 2, 3, 2], [4, 5, 3, 4], [5, 5, 5, 5], [4, 5, 4, 5]],
            (4, 4): [[5, 5, 5, 5], [0, 1, 1, 0], [3, 5, 1, 3], [3, 4, 2, 3], [1, 2, 2, 1]],
            (3, 3): [[6, 7, 7], [3, 4, 3], [5, 6, 5], [6, 7, 7], [5, 6, 7]],
            (4, 3): [[6, 7, 7], [0, 2, 0], [4, 5, 3], [3, 5, 4], [2, 2, 2]]}


@pytest.mark.parametrize("k,bins", sorted(EXAMPLES))
def test_the_readme_example(memo, k, bins):
    from memo_amd import matrix, tracks
    path = os.path.join(G.GOLD, "example_memb.parquet")
    counts, edges = tracks.region_tracks(path, "ref_1:0-20", k, 5, bins)
    assert edges.tolist() == ([0, 5, 10, 15, 20] if bins == 4 else [0, 6, 13, 20])
    assert counts.dtype == np.uint64 and counts.tolist() == EXAMPLES[k, bins]
    if k == 3:
        assert counts.sum(axis=1).tolist() == [20, 10, 16, 20, 18]
        assert np.array_equal(counts.sum(axis=1), np.diag(matrix.region_matrix(path, "ref_1:0-20", k, 5)))      # the diagonal of memo matrix


def test_region_tracks_raises_what_memo_query_raises(memo):
    from memo_amd import tracks
    path = os.path.join(G.GOLD, "example_memb.parquet")
    with pytest.raises(ValueError):
        tracks.region_tracks(path, "ref_1:20-0", 3, 5, 4)
    with pytest.raises(ValueError):
        tracks.region_tracks(path, "ref_1:0:20", 3, 5, 4)
    with pytest.raises(IndexError):                      # the sweep's own: an annot outside the result columns
        tracks.region_tracks(path, "ref_1:0-20", 3, 2, 4)
    for bins in (0, 21):                                 # fewer than one bin, more bins than positions: both numbers are named
        with pytest.raises(ValueError) as exc:
            tracks.region_tracks(path, "ref_1:0-20", 3, 5, bins)
        assert str(bins) in str(exc.value) and "20" in str(exc.value)
    counts, edges = tracks.region_tracks(path, "ref_1:7-7", 3, 5, 4)            # an empty window: no bins
    assert counts.shape == (5, 0) and edges.tolist() == [0]


def test_a_window_past_2_to_the_32(memo, tmp_path):
    """the rows of a golden index shifted past 2^32 and 2^33: the table of the shifted window is the origin's"""
    import pyarrow as pa
    import pyarrow.parquet as pq
    from memo_amd import tracks
    c = next(c for c in G.cases(membership=True, raises=False) if c["name"] == "rnd_n40_memb_k31_c0w1")
    rec, qs, qe = G.region(c)
    s, e, o = G.index_columns(c["index"], rec)
    bins = min(qe - qs, 11)
    want, edges = tracks.region_tracks(os.path.join(G.GOLD, c["index"]), c["region"], c["k"], c["n"], bins)
    assert same(want, O.tracks(G.expected_matrix(c, G.load(c)), edges)) and int(want.sum()) > 0
    for D in (2 ** 32, 2 ** 33 + 12_345):
        path = str(tmp_path / f"far{D}.parquet")
        pq.write_table(pa.table({"f0": pa.array([rec] * len(s), pa.utf8()), "f1": s + D, "f2": e + D, "f3": o}), path, compression="ZSTD")
        for step in (1 << 24, 1000):
            got, far_edges = tracks.region_tracks(path, f"{rec}:{qs + D}-{qe + D}", c["k"], c["n"], bins, slice_positions=step)
            assert np.array_equal(got, want) and np.array_equal(far_edges, edges), (D, step)


# ---------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------
def _memo(*argv, env=None):
    return subprocess.run([sys.executable, EXE, *argv], capture_output=True, timeout=300, env=dict(os.environ, **(env or {})))


def test_cli_writes_counts_fractions_and_labels(memo, tmp_path):
    from memo_amd import tracks, view
    c = next(c for c in G.cases(membership=True, raises=False) if c["name"] == "ex_memb_k3_0_20")
    assert (c["index"], c["region"], c["k"], c["n"]) == ("example_memb.parquet", "ref_1:0-20", 3, 5)
    edges = view.bin_edges(20, 4)
    want = O.tracks(G.expected_matrix(c, G.load(c)), edges)
    memb, out = os.path.join(G.GOLD, "example_memb.parquet"), str(tmp_path / "t.tsv")
    common = ("-b", memb, "-k", "3", "-n", "5", "-r", "ref_1:0-20", "-B", "4", "-o", out)
    r = _memo("tracks", *common)
    assert (r.returncode, r.stdout) == (0, b"MEMO - tracks\n"), r.stderr
    text = open(out).read()
    assert text == tracks.format_tracks(want, 0, edges) and text.startswith("genome\t0-5\t5-10\t10-15\t15-20\n0\t5\t5\t5\t5\n1\t3\t2\t3\t2\n")
    assert _memo("tracks", *common, "-f").returncode == 0
    assert open(out).read() == tracks.format_tracks(tracks.fractions(want, edges), 0, edges)
    genomes = tmp_path / "genomes.txt"
    genomes.write_text("ref/pivot.fa\nasm/g1.fa.gz\ng2.fasta\n\ng3.fa\ng4.fna\n")
    assert _memo("tracks", *common, "-g", str(genomes)).returncode == 0
    labels = ["pivot", "g1", "g2", "g3", "g4"]
    text = open(out).read()
    assert text == tracks.format_tracks(want, 0, edges, labels) and "\npivot\t5\t5\t5\t5\ng1\t3\t" in text
    assert sorted(os.listdir(tmp_path)) == ["genomes.txt", "t.tsv"]                       # written beside its name and renamed
    # a window that does not begin at 0: absolute coordinates in the header; the default of 500 bins is too many for it
    r = _memo("tracks", "-b", memb, "-k", "3", "-n", "5", "-r", "ref_1:5-18", "-B", "2", "-o", out)
    assert r.returncode == 0 and open(out).read().startswith("genome\t5-11\t11-18\n0\t6\t7\n")
    os.unlink(out)
    # an empty window: an empty file
    r = _memo("tracks", "-b", memb, "-k", "3", "-n", "5", "-r", "ref_1:7-7", "-o", out)
    assert r.returncode == 0 and open(out).read() == "", r.stderr
    # what memo query raises, as a message; nothing is written
    never = str(tmp_path / "never.tsv")
    r = _memo("tracks", "-b", memb, "-k", "3", "-n", "5", "-r", "ref_1:20-0", "-o", never)
    assert r.returncode == 1 and b"negative dimensions" in r.stderr and not os.path.exists(never)
    r = _memo("tracks", "-b", memb, "-k", "3", "-n", "2", "-r", "ref_1:0-20", "-B", "4", "-o", never)
    assert r.returncode == 1 and b"IndexError" in r.stderr and not os.path.exists(never)
    r = _memo("tracks", "-b", memb, "-k", "3", "-n", "5", "-r", "ref_1:0-20", "-o", never)          # 500 bins for 20 positions
    assert r.returncode == 1 and b"500 bins" in r.stderr and b"20 positions" in r.stderr and not os.path.exists(never)
    assert sorted(os.listdir(tmp_path)) == ["genomes.txt", "t.tsv"]


def test_cli_draws_the_heat_map(memo, tmp_path):
    pytest.importorskip("matplotlib")
    memb, out = os.path.join(G.GOLD, "example_memb.parquet"), str(tmp_path / "tracks.png")
    genomes = tmp_path / "genomes.txt"
    genomes.write_text("pivot.fa\ng1.fa\ng2.fa\ng3.fa\ng4.fa\n")
    r = _memo("tracks", "-b", memb, "-k", "3", "-n", "5", "-r", "ref_1:0-20", "-B", "4", "-d", "50", "-g", str(genomes), "-o", out)
    assert (r.returncode, r.stdout) == (0, b"MEMO - tracks\n"), r.stderr
    assert open(out, "rb").read(8) == b"\x89PNG\r\n\x1a\n" and os.path.getsize(out) > 1000
    assert sorted(os.listdir(tmp_path)) == ["genomes.txt", "tracks.png"]
