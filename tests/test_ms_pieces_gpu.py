"""Matching statistics of genomes given as records (memo_ms_add_records): the device assembles each genome's text in pieces
of whole strings and merges the pieces' MS by elementwise maximum.  Checked against the one-text path (add(genome_text(...)),
which stays limited to texts under 2^31 - 1 bytes), the suffix-automaton oracle, the device-built piece texts byte for byte,
a genome whose text passes 2^31 bytes, and `memo index` with forced pieces against the golden Parquet files."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import ms_oracle as M
from tests import golden_util as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "memo")
EXAMPLE = [os.path.join(G.GOLD, "example_fa", f"ref_{i}.fa") for i in range(1, 6)]
IUPAC = b"ACGTACGTACGTRYKMBVDHSWN"


@pytest.fixture(scope="module")
def bi():
    from memo_amd import _lib, build_index
    _lib.lib()
    return build_index


def _rand(rng, n, alpha=b"ACGT"):
    a = np.frombuffer(alpha, np.uint8)
    return a[rng.integers(0, len(a), n)].tobytes()


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert not len(bad), (f"{what}: {len(bad)} positions differ, first {bad[:8].tolist()}: "
                          f"got {got[bad[:8]].tolist()}, want {want[bad[:8]].tolist()}")


def _pangenome(rng, n_genomes=5):
    """pivot records and genomes of random ACGT / IUPAC / N, with empty records, 1-base records, hundreds of tiny records,
    pieces of the pivot copied forward and reverse-complemented"""
    from memo_amd.build_index import revcomp
    pivot = [_rand(rng, 3000), _rand(rng, 1, IUPAC), _rand(rng, 777, IUPAC)] + [_rand(rng, int(rng.integers(1, 9)))
                                                                             for _ in range(200)]
    whole = b"".join(pivot)
    genomes = []
    for g in range(n_genomes):
        recs = []
        for _ in range(int(rng.integers(1, 12))):
            kind = int(rng.integers(0, 6))
            if kind == 0:
                recs.append(b"")
            elif kind == 1:
                recs.append(_rand(rng, 1, IUPAC))
            elif kind == 2:
                recs.append(_rand(rng, int(rng.integers(50, 3000)), IUPAC))
            else:
                a = int(rng.integers(0, len(whole) - 200))
                seg = whole[a:a + int(rng.integers(20, 1500))]
                seg = revcomp(seg) if kind == 3 else seg
                recs.append(_rand(rng, int(rng.integers(0, 40))) + seg + _rand(rng, int(rng.integers(0, 40)), IUPAC))
        if g == 1:
            recs += [_rand(rng, int(rng.integers(0, 4)), IUPAC) for _ in range(300)]   # hundreds of tiny records
        if g == 2:
            recs = [b""] * 3 + recs + [b""]
        genomes.append(recs)
    genomes.append([b"N" * 500, b""])
    return pivot, genomes


def _longest(recs):
    return max((len(s) for s in recs), default=0)


def _cap(recs, what):
    """a forced cap: the longest string (+ 1 or + 2 bytes), or a fixed size where every string fits"""
    fit = max(2, _longest(recs) + 1)
    return {"longest+1": fit, "longest+2": fit + 1}.get(what, 0) if isinstance(what, str) \
        else max(what, fit)


def _expected_pieces(bi, recs, cap):
    """the piece texts the plan gives, built on the host from genome_text's strings"""
    strings = list(recs) + [bi.revcomp(s) for s in recs]
    n, piece = bi.plan_pieces([len(s) for s in recs], cap)
    return [b"".join(s + b"\0" for s, p in zip(strings, piece) if p == k) for k in range(n)]


def _piece_text(ms, recs, cap, piece):
    from memo_amd import _lib
    L = _lib.lib()
    seq = b"".join(recs)
    rb = np.zeros(len(recs) + 1, np.int64)
    rb[1:] = np.cumsum([len(s) for s in recs])
    n = C.c_int64()
    np_ = _lib.check(L.memo_debug_ms_piece_text(ms._h, seq, rb.ctypes.data, len(recs), cap, piece, None, 0, C.byref(n)))
    out = np.full(n.value + 64, 0xAA, np.uint8)
    _lib.check(L.memo_debug_ms_piece_text(ms._h, seq, rb.ctypes.data, len(recs), cap, piece, out.ctypes.data, len(out),
                                          C.byref(n)))
    assert not out[n.value:].any(), "the pad behind a piece is not zero"
    return np_, out[:n.value].tobytes()


@pytest.fixture
def ab(bi):
    """libmemo_amd_ab.so (the product objects + memo_debug_*) for the handles made inside the test"""
    from memo_amd import _lib
    _lib.use_ab()
    yield
    _lib.use_ab(False)


def test_device_piece_texts_equal_genome_text(bi, ab):
    rng = np.random.default_rng(11)
    pivot, genomes = _pangenome(rng)
    seq, rb = M.records_layout(pivot)
    every = bytes(range(1, 256)) * 3
    genomes += [[every, every[::-1], b""], [b"ACGTRYKMBVDHSWN" * 7, b"acgtn"], [b""], [b"", b"A"]]
    with bi.MatchingStatistics(seq, rb, 1) as ms:
        for recs in genomes:
            np_, text = _piece_text(ms, recs, 0, 0)
            assert np_ == 1 and text == bi.genome_text(recs)
            for what in ("longest+1", "longest+2", 64, 1000):
                cap = _cap(recs, what)
                want = _expected_pieces(bi, recs, cap)
                assert b"".join(want) == bi.genome_text(recs)
                for k, w in enumerate(want):
                    np_, text = _piece_text(ms, recs, cap, k)
                    assert np_ == len(want) and text == w, (cap, k)


@pytest.mark.parametrize("chunk", [1, 7, 0])
def test_add_records_equals_the_whole_text_at_every_cap(bi, chunk):
    rng = np.random.default_rng(100 + chunk)
    pivot, genomes = _pangenome(rng)
    seq, rb = M.records_layout(pivot)
    with bi.MatchingStatistics(seq, rb, len(genomes), 0, chunk) as ms:
        for c, recs in enumerate(genomes):
            ms.add(bi.genome_text(recs), c)
        want = ms.fetch()
        for c, recs in enumerate(genomes):
            _same(want[:, c], M.ms(bi.genome_text(recs), seq, rb), f"add() genome {c}")
    for what in ("default", "longest+1", "longest+2", 64, 1000):
        with bi.MatchingStatistics(seq, rb, len(genomes), 0, chunk) as ms:
            for c, recs in enumerate(genomes):
                cap = _cap(recs, what)
                n_pieces = ms.add_records(recs, c, cap)
                assert n_pieces == (bi.plan_pieces([len(s) for s in recs], cap)[0] if cap else 1), (what, c)
            got = ms.fetch()
            print(f"cap {what} chunk {chunk}: {ms.timings()}")
        _same(got, want, f"add_records at cap {what}, chunk {chunk}")


def test_strand_split_across_pieces(bi):
    """S_i and rc(S_i) in different pieces, down to one piece per string (cap 401): a pivot made of a genome's reverse
    complements"""
    rng = np.random.default_rng(5)
    recs = [_rand(rng, 400, IUPAC) for _ in range(4)]
    pivot = [bi.revcomp(recs[1]) + recs[2][:100], recs[0][50:300], bi.revcomp(recs[3])[10:]]
    seq, rb = M.records_layout(pivot)
    want = M.ms(bi.genome_text(recs), seq, rb)
    for cap in (401, 802, 1203, 1604, 3208):
        with bi.MatchingStatistics(seq, rb, 1) as ms:
            n = ms.add_records(recs, 0, cap)
            assert n == bi.plan_pieces([400] * 4, cap)[0]
            _same(ms.fetch()[:, 0], want, f"cap {cap}")
    assert bi.plan_pieces([400] * 4, 1203)[1].tolist() == [0, 0, 0, 1, 1, 1, 2, 2]
    assert bi.plan_pieces([400] * 4, 401)[1].tolist() == list(range(8))


def test_reused_handle_and_refused_records(bi):
    from memo_amd._lib import MemoError
    rng = np.random.default_rng(3)
    pivot, genomes = _pangenome(rng, 3)
    seq, rb = M.records_layout(pivot)
    with bi.MatchingStatistics(seq, rb, 3) as ms:
        for c in range(3):
            ms.add_records(genomes[c], c, _cap(genomes[c], 300 + 100 * c))
        before = ms.fetch()
        for c in range(3):
            _same(before[:, c], M.ms(bi.genome_text(genomes[c]), seq, rb), f"genome {c}")
        # column 1 rewritten by another genome: equals that genome alone, its neighbours unchanged
        ms.add_records(genomes[0], 1, 0)
        after = ms.fetch()
        _same(after[:, 1], before[:, 0], "column 1 rewritten")
        _same(after[:, 0], before[:, 0], "column 0")
        _same(after[:, 2], before[:, 2], "column 2")
        # an empty genome zeroes its column
        assert ms.add_records([], 1) == 0
        assert not ms.fetch()[:, 1].any()
        ms.add_records(genomes[1], 1, 0)
        _same(ms.fetch(), before, "column 1 restored")
        # a record longer than the cap: refused before anything is written
        big = [b"ACGT" * 100, b"A" * 2000]
        with pytest.raises(MemoError, match="genome record 1 of 2000 bases needs 2001 bytes"):
            ms.add_records(big, 1, 2000)
        for bad in (1, (1 << 31) - 1):
            with pytest.raises(MemoError, match=r"outside \[2, 2\^31 - 2\]"):
                ms.add_records(big, 1, bad)
        with pytest.raises(MemoError, match="outside"):
            ms.add_records(big, 3, 0)
        _same(ms.fetch(), before, "after the refusals")


def _past_2_31(rng, bi):
    """17 records of 2^26 random bases (a text of 2^31 + 2^27 + 34 bytes) and a pivot whose planted segments match only
    inside rc(S_17), past text byte 2^31"""
    n_rec, L = 17, 1 << 26
    letters = np.frombuffer(b"ACGT", np.uint8)
    recs = [letters[rng.integers(0, 4, L, dtype=np.uint8)] for _ in range(n_rec)]
    pivot = [bytearray(_rand(rng, 60_000)), bytearray(_rand(rng, 40_000))]
    plants = []          # (pivot record, a, length)
    last = recs[-1]
    comp = {ord(a): ord(b) for a, b in zip("ACGT", "TGCA")}
    for k, (r, a, ln) in enumerate([(0, 1000, 5000), (0, 30_000, 777), (1, 5, 20_000), (1, 39_000, 1000), (0, 59_000, 1000)]):
        ln = min(ln, len(pivot[r]) - a)
        seg = bytes(pivot[r][a:a + ln])
        at = 1_000_000 + k * 10_000_000          # S_17[at, at + ln) = rc(seg), so rc(S_17) holds seg
        last[at:at + ln] = np.frombuffer(bi.revcomp(seg), np.uint8)
        # flanks: the byte after seg inside rc(S_17) is comp(S_17[at - 1]); make it differ from the pivot's next byte
        if a + ln < len(pivot[r]):
            nxt = pivot[r][a + ln]
            while comp[int(last[at - 1])] == nxt:
                last[at - 1] = letters[(np.where(letters == last[at - 1])[0][0] + 1) % 4]
        # and the byte before seg (comp(S_17[at + ln])) differ from the pivot's previous byte: the match starts at a
        if a > 0:
            prv = pivot[r][a - 1]
            while comp[int(last[at + ln])] == prv:
                last[at + ln] = letters[(np.where(letters == last[at + ln])[0][0] + 1) % 4]
        plants.append((r, a, ln))
    return [bytes(p) for p in pivot], [x.tobytes() for x in recs], plants


def test_text_past_2_31_equals_the_per_record_reference(bi):
    rng = np.random.default_rng(2031)
    pivot, recs, plants = _past_2_31(rng, bi)
    text_bytes = 2 * sum(len(s) + 1 for s in recs)
    assert text_bytes == (1 << 31) + (1 << 27) + 34 > bi.MAX_TEXT
    seq, rb = M.records_layout(pivot)
    with bi.MatchingStatistics(seq, rb, 2) as ms:
        n = ms.add_records(recs, 0, 1 << 28)
        assert n == 12 == bi.plan_pieces([len(s) for s in recs], 1 << 28)[0]
        got = ms.fetch()[:, 0].copy()
        print(f"past 2^31: {n} pieces, {ms.timings()}")
        ref = np.zeros_like(got)
        for i, s in enumerate(recs):          # the existing one-text path, one record at a time
            ms.add(bi.genome_text([s]), 1)
            ref = np.maximum(ref, ms.fetch()[:, 1])
    _same(got, ref, "add_records past 2^31 vs the per-record maximum")
    # closed form where the planted segments lie
    checked = 0
    for r, a, ln in plants:
        for j in range(ln):
            if ln - j >= 40:
                assert got[rb[r] + a + j] == ln - j, (r, a, ln, j, got[rb[r] + a + j])
                checked += 1
    assert checked > 20_000
    assert got.max() >= 20_000


def test_memo_index_with_forced_pieces_equals_the_golden_index(bi, tmp_path):
    import pyarrow.parquet as pq
    longest = max(len(s) for p in EXAMPLE for _, s in bi.read_fasta(p))
    lst = tmp_path / "genome_list.txt"
    lst.write_text("".join(p + "\n" for p in EXAMPLE))
    env = dict(os.environ, MEMO_INDEX_PIECE_BYTES=str(longest + 1))
    for flag, prefix, golden in (([], "test", "example_cons.parquet"), (["-m"], "memb", "example_memb.parquet")):
        r = subprocess.run([sys.executable, EXE, "index", "-g", str(lst), "-o", str(tmp_path / "w"), "-p", prefix] + flag,
                           capture_output=True, timeout=300, env=env)
        assert r.returncode == 0, r.stderr
        assert r.stdout.decode().splitlines()[-1] == "DONE"
        got, want = pq.read_table(str(tmp_path / "w" / (prefix + ".parquet"))), pq.read_table(os.path.join(G.GOLD, golden))
        assert got.schema.names == ["f0", "f1", "f2", "f3"]
        for col in ("f0", "f1", "f2", "f3"):
            assert got.column(col).to_pylist() == want.column(col).to_pylist(), (prefix, col)
    # the pieces that ran: one string per piece
    st = bi.build_index(str(lst), str(tmp_path / "w2"), "x", False, log=lambda s: None, piece_bytes=longest + 1)
    assert st["pieces"] == [2 * len(bi.read_fasta(p)) for p in EXAMPLE[1:]]
    st = bi.build_index(str(lst), str(tmp_path / "w2"), "x", False, log=lambda s: None)
    assert st["pieces"] == [1] * (len(EXAMPLE) - 1)
    # a record longer than the cap: the CLI names the file and the record
    env = dict(os.environ, MEMO_INDEX_PIECE_BYTES=str(longest))
    r = subprocess.run([sys.executable, EXE, "index", "-g", str(lst), "-o", str(tmp_path / "w3"), "-p", "t"],
                       capture_output=True, timeout=300, env=env)
    assert r.returncode == 1 and b"record '" in r.stderr and b"piece cap" in r.stderr, r.stderr
