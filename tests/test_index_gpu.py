"""`memo index` on the GPU: suffix arrays, matching statistics (MS) against brute force and against the suffix-
automaton dev tool (tools/ms_sam.cpp), the example walkthrough of the reference (FASTA -> index -> query, the golden
bytes), what an index built this way means, and the refusals."""
import ctypes as C
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle.ms_oracle import brute_ms as _brute_ms  # tools/make_golden.py's definition
from tests import golden_util as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "memo")
EXAMPLE = [os.path.join(G.GOLD, "example_fa", f"ref_{i}.fa") for i in range(1, 6)]


@pytest.fixture(scope="module")
def bi():
    from memo_amd import _lib, build_index
    _lib.lib()
    return build_index


# ---- the example walkthrough ------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def example(tmp_path_factory, bi):
    work = tmp_path_factory.mktemp("example")
    lst = work / "genome_list.txt"
    lst.write_text("".join(p + "\n" for p in EXAMPLE))
    out = {}
    for flag, prefix in (([], "test"), (["-m"], "memb")):
        r = subprocess.run([sys.executable, EXE, "index", "-g", str(lst), "-o", str(work / "w"), "-p", prefix] + flag,
                           capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr
        lines = r.stdout.decode().splitlines()
        assert lines[-1] == "DONE"
        assert ("Making membership index" if flag else "Making conservation index") in lines
        out[prefix] = str(work / "w" / (prefix + ".parquet"))
    return out


def test_example_ms_equal_the_golden_dap(bi):
    recs = [bi.read_fasta(p) for p in EXAMPLE]
    got = bi.matching_statistics([s for _, s in recs[0]], [[s for _, s in r] for r in recs[1:]])
    want = np.loadtxt(os.path.join(G.GOLD, "example_dap.txt"), dtype=np.int64)
    assert np.array_equal(want[:, 0], np.arange(len(want)))
    assert np.array_equal(got, want[:, 1:])


@pytest.mark.parametrize("prefix,golden", [("test", "example_cons.parquet"), ("memb", "example_memb.parquet")])
def test_example_parquet_equals_the_golden_index(example, prefix, golden):
    import pyarrow.parquet as pq
    got, want = pq.read_table(example[prefix]), pq.read_table(os.path.join(G.GOLD, golden))
    assert got.schema.names == ["f0", "f1", "f2", "f3"]
    assert [str(t) for t in got.schema.types] == ["string", "int64", "int64", "int64"]
    assert pq.ParquetFile(example[prefix]).metadata.row_group(0).column(1).compression == "ZSTD"
    for col in ("f0", "f1", "f2", "f3"):
        assert got.column(col).to_pylist() == want.column(col).to_pylist(), col


@pytest.mark.parametrize("c", [c for c in G.cases() if c["name"].startswith("ex_")], ids=lambda c: c["name"])
def test_example_queries_on_the_built_index(example, c, tmp_path):
    """the README flow: `memo query` on the freshly built index writes the reference's bytes"""
    index = example["test" if c["index"] == "example_cons.parquet" else "memb"]
    out = tmp_path / "out.txt"
    argv = [sys.executable, EXE, "query", "-b", index, "-k", str(c["k"]), "-n", str(c["n"]), "-r", c["region"],
            "-o", str(out)] + (["-m"] if c["membership"] else [])
    r = subprocess.run(argv, capture_output=True, timeout=300)
    if "raises" in c:
        assert r.returncode != 0 and c["raises"].encode() in r.stderr
    else:
        assert r.returncode == 0, r.stderr
        assert G.sha(out.read_bytes()) == c["sha256"]


# ---- suffix array -------------------------------------------------------------------------------------------

def _texts():
    rng = np.random.default_rng(11)
    yield "random_acgt", bytes(rng.choice(list(b"ACGT"), 3000).astype(np.uint8))
    yield "random_bytes", bytes(rng.integers(0, 256, 2000).astype(np.uint8))
    yield "homopolymer", b"A" * 5000
    yield "acgt_repeat", b"ACGT" * 1000
    yield "all_n", b"N" * 3001
    yield "separators", bytes(rng.choice(list(b"AC\0"), 2500, p=[0.3, 0.3, 0.4]).astype(np.uint8))
    yield "one", b"G"
    yield "two_runs", b"\0" * 700 + b"A" * 700 + b"\0" * 5


@pytest.mark.parametrize("name,text", list(_texts()), ids=[n for n, _ in _texts()])
def test_suffix_array_equals_a_sort_of_the_suffixes(bi, name, text):
    from memo_amd._lib import check, lib
    sa = np.empty(len(text), np.int32)
    check(lib().memo_suffix_array(text, len(text), sa.ctypes.data, 0))
    assert sa.tolist() == sorted(range(len(text)), key=lambda i: text[i:])


# ---- MS against brute force -----------------------------------------------------------------------------------

def _mutate(rng, seq, rate, alphabet=b"ACGT"):
    out = bytearray()
    for ch in seq:
        r = rng.random()
        if r < rate / 3:
            continue
        if r < 2 * rate / 3:
            out.append(alphabet[rng.integers(len(alphabet))])
            continue
        out.append(ch)
        if r > 1 - rate / 3:
            out.append(alphabet[rng.integers(len(alphabet))])
    return bytes(out)


def _cases():
    rng = np.random.default_rng(3)
    rnd = lambda n, a=b"ACGT": bytes(rng.choice(list(a), n).astype(np.uint8))  # noqa: E731
    piv = [rnd(900), rnd(300), rnd(5)]
    yield "multi_record", piv, [[_mutate(rng, s, 0.05) for s in piv], [_mutate(rng, piv[0], 0.2)], [rnd(50), rnd(70)]]
    iupac = b"ACGTNNNNRYKMBVDHSW"
    piv = [rnd(600, iupac), b"N" * 40 + rnd(100) + b"N" * 40]
    yield "n_runs_iupac", piv, [[_mutate(rng, s, 0.05, iupac) for s in piv], [b"N" * 500], [rnd(400, b"RYKM")]]
    piv = [rnd(1000), rnd(400)]
    yield "identical_genome", piv, [list(piv), [piv[1], piv[0]]]
    yield "absent", [rnd(300, b"AC")], [[rnd(300, b"GT")], [b"T" * 50]]
    a = rnd(200)
    yield "record_ends", [a[:100], a[100:]], [[a], [a + a]]          # matches that would run on into the next record
    yield "empty_genome", [rnd(100)], [[], [b""], [rnd(100)]]


@pytest.mark.parametrize("name,pivot,genomes", list(_cases()), ids=[n for n, _, _ in _cases()])
def test_ms_equal_brute_force(bi, name, pivot, genomes):
    got = bi.matching_statistics(pivot, genomes)
    for c, recs in enumerate(genomes):
        text = bi.genome_text(recs)
        assert np.array_equal(got[:, c], _brute_ms(pivot, text)), (name, c)
    if name == "identical_genome":
        assert got[:len(pivot[0]), 0].tolist() == list(range(len(pivot[0]), 0, -1))


def test_chunk_lengths_give_identical_matrices(bi):
    rng = np.random.default_rng(17)
    piv = [bytes(rng.choice(list(b"ACGT"), n).astype(np.uint8)) for n in (150_000, 33_333, 1)]
    genomes = [[_mutate(rng, s, 0.002 * (g + 1)) for s in piv] for g in range(3)]
    genomes.append([piv[0][::-1], piv[1] * 2])
    base = bi.matching_statistics(piv, genomes)
    assert base.max() > 1000
    for chunk in (1, 7, 64):
        assert np.array_equal(bi.matching_statistics(piv, genomes, chunk=chunk), base), chunk


# ---- MS against tools/ms_sam.cpp on a realistic pangenome ----------------------------------------------------

def test_ms_equal_the_suffix_automaton(bi, tmp_path):
    spec = importlib.util.spec_from_file_location("realistic_index", os.path.join(ROOT, "tools", "realistic_index.py"))
    ri = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ri)
    rng = np.random.default_rng(2026)
    L, N = 2_000_000, 4
    pivot = rng.integers(0, 4, L).astype(np.uint8)
    pivot.tofile(tmp_path / "pivot.bin")
    letters = np.frombuffer(b"ACGT", np.uint8)
    genomes, paths = [], []
    for g in range(1, N + 1):
        seq = ri.mutate(rng, pivot, 0.001 * g, g)
        np.concatenate([seq, [4], ri.revcomp(seq), [4]]).astype(np.uint8).tofile(tmp_path / f"g{g}.bin")
        paths.append(str(tmp_path / f"g{g}.bin"))
        genomes.append([letters[seq].tobytes()])
    exe = str(tmp_path / "ms_sam")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", os.path.join(ROOT, "tools", "ms_sam.cpp"), "-o", exe])
    subprocess.run([exe, str(tmp_path / "pivot.bin"), str(tmp_path / "dap.i32")] + paths, check=True, timeout=600,
                   capture_output=True, env=dict(os.environ, MS_THREADS="4"))
    want = np.fromfile(tmp_path / "dap.i32", np.int32).reshape(L, N)
    got = bi.matching_statistics([letters[pivot].tobytes()], genomes)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]


# ---- what the index means ---------------------------------------------------------------------------------------

def _revcomp(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


@pytest.fixture(scope="module")
def pangenome(tmp_path_factory, bi):
    """as tests/test_end_to_end_semantics.py, but FASTA files through `memo index`"""
    rng = np.random.default_rng(2024)
    work = tmp_path_factory.mktemp("pan_fa")
    records = [("chrA", 1500), ("chrB", 700)]
    pivot = [(name, "".join("ACGT"[x] for x in rng.integers(0, 4, n))) for name, n in records]
    files, texts = [], []

    def write(path, recs):
        with open(path, "w") as fh:
            for name, seq in recs:
                fh.write(f">{name} genome\n" + "".join(seq[i:i + 60].lower() + "\n" for i in range(0, len(seq), 60)))
        files.append(str(path))

    write(work / "pivot.fa", pivot)
    for g in range(6):
        recs = [(name, _mutate(rng, seq.encode(), 0.02 * (g + 1)).decode()) for name, seq in pivot]
        if g == 3:
            recs[1] = (recs[1][0], "")                   # one genome lacks chrB altogether
        write(work / f"g{g}.fa", recs)
        texts.append("$".join(r + "$" + _revcomp(r) for _, r in recs))
    (work / "list.txt").write_text("".join(f + "\n" for f in files))
    idx = {}
    for prefix, flags in (("cons", []), ("memb", ["-m"])):
        r = subprocess.run([sys.executable, EXE, "index", "-g", str(work / "list.txt"), "-o", str(work), "-p", prefix]
                           + flags, capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr
        idx[prefix] = str(work / (prefix + ".parquet"))
    return dict(work=work, pivot=pivot, genomes=texts, n_docs=len(texts) + 1, idx=idx)


@pytest.mark.parametrize("k", [4, 12, 31])
def test_built_index_counts_genomes_containing_the_kmer(pangenome, k):
    from memo_amd import memo_query as mq
    P = pangenome
    for name, seq in P["pivot"]:
        L = len(seq)
        truth = np.ones(L, np.int64)
        for p in range(L - k + 1):
            truth[p] += sum(seq[p:p + k] in text for text in P["genomes"])
        out = os.path.join(P["work"], f"c_{name}_{k}.txt")
        mq.main(mq.parse_arguments(["-b", P["idx"]["cons"], "-k", str(k), "-n", str(P["n_docs"]), "-r", f"{name}:0-{L}",
                                    "-o", out]))
        assert np.array_equal(np.loadtxt(out, dtype=np.int64), truth), (name, k)


@pytest.mark.parametrize("k", [4, 31])
def test_built_index_membership_is_kmer_presence(pangenome, k):
    from memo_amd import memo_query as mq
    P = pangenome
    for name, seq in P["pivot"]:
        L = len(seq)
        truth = np.zeros((L, P["n_docs"]), np.int64)
        truth[:, 0] = 1
        for p in range(L - k + 1):
            truth[p, 1:] = [seq[p:p + k] in text for text in P["genomes"]]
        out = os.path.join(P["work"], f"m_{name}_{k}.txt")
        mq.main(mq.parse_arguments(["-m", "-b", P["idx"]["memb"], "-k", str(k), "-n", str(P["n_docs"]),
                                    "-r", f"{name}:0-{L}", "-o", out]))
        assert np.array_equal(np.loadtxt(out, dtype=np.int64, ndmin=2), truth), (name, k)


# ---- refusals --------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing(bi):
    from memo_amd._lib import MemoError, check, lib
    small = b"ACGT" * 4
    with pytest.raises(MemoError, match="limit is 2\\^31"):         # declared length: checked before the text is read
        with bi.MatchingStatistics(small, np.array([0, 16]), 1) as ms:
            check(lib().memo_ms_add_genome(ms._h, small, 1 << 31, 0))
    with pytest.raises(MemoError, match="outside"):
        check(lib().memo_suffix_array(small, 1 << 31, None, 0))
    h = C.c_void_p()
    huge = np.array([0, (1 << 30) - 1], np.int64)                 # x 4096 genomes: 17.6 TB of DAP
    with pytest.raises(MemoError, match="device memory"):          # refused before the (16-byte) pivot is read
        check(lib().memo_ms_create(small, huge.ctypes.data, 1, 4096, 0, 0, C.byref(h)))
    assert not h.value
    four = np.array([0, 4], np.int64)
    with pytest.raises(MemoError, match="NUL"):
        check(lib().memo_ms_create(b"AC\0T", four.ctypes.data, 1, 1, 0, 0, C.byref(h)))
    assert not h.value
