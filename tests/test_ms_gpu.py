"""`memo index`'s HIP stage (memo_amd/csrc/memo_ms.hip) against references that share no algorithm with it, where
such code goes wrong: suffix arrays (prefix doubling) against the Burkhardt-Kaerkkaeinen checker and sorted(), and
matching statistics (SA + PLCP + 64-ary min hierarchy + interval walk) against the byte-level suffix automaton of
oracle/ms_oracle.c, both proved in tests/test_ms_oracle.py.

The inputs aim at the kernel's branches: every round-0 key width (alphabet sizes), pair-key widths at powers of two,
texts that keep groups active for many doubling rounds, SA intervals wide enough that the hierarchy searches climb
2, 3 and 4 levels (tandem arrays, homopolymers, N runs), texts of lengths at 64^k +- 1 and 256 m +- 1 (hierarchy
levels, PLCP chunks), thousands of tiny pivot records at every walk-chunk length, every byte value, one handle
reused across genomes of very different sizes, and a DAP matrix past 2^31 entries.  Every case is seeded and sized
to run in seconds; each prints MatchingStatistics.timings()."""
import numpy as np
import pytest

from oracle import dap_oracle
from oracle import ms_oracle as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bi():
    from memo_amd import _lib, build_index
    _lib.lib()
    return build_index


def _rand(rng, n, alpha=b"ACGT"):
    a = np.frombuffer(alpha, np.uint8)
    return a[rng.integers(0, len(a), n)].tobytes()


def _mutate(rng, seq, rate, alpha=b"ACGT"):
    """substitutions at `rate` (vectorised; lengths stay)"""
    s = np.frombuffer(seq, np.uint8).copy()
    hit = rng.random(len(s)) < rate
    a = np.frombuffer(alpha, np.uint8)
    s[hit] = a[rng.integers(0, len(a), int(hit.sum()))]
    return s.tobytes()


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert not len(bad), (f"{what}: {len(bad)} positions differ, first {bad[:8].tolist()}: "
                          f"got {got[bad[:8]].tolist()}, want {want[bad[:8]].tolist()}")


def _ms(bi, records, texts, name, chunk=0, want=None):
    """MS matrix of pivot records against raw texts (one column each), checked column by column against `want`
    (the oracle's columns when not given)"""
    seq, rb = M.records_layout(records)
    with bi.MatchingStatistics(seq, rb, len(texts), 0, chunk) as ms:
        for c, t in enumerate(texts):
            ms.add(t, c)
        got = ms.fetch()
        print(f"timings {name} chunk={chunk}: {ms.timings()}")
    for c, t in enumerate(texts):
        _same(got[:, c], M.ms(t, seq, rb) if want is None else want[c], f"{name} column {c}")
    return got


# ---- suffix arrays ------------------------------------------------------------------------------------------

def _sa(text):
    from memo_amd._lib import check, lib
    sa = np.empty(len(text), np.int32)
    check(lib().memo_suffix_array(text, len(text), sa.ctypes.data, 0))
    return sa


def _check_sa(text, what):
    sa = _sa(text)
    err = M.check_sa(text, sa)
    assert err is None, f"{what} (n = {len(text)}): {err}"
    if len(text) <= 5000:
        assert sa.tolist() == sorted(range(len(text)), key=lambda i: text[i:]), what


def _cpk(sigma):  # memo_ms.hip's round-0 characters per key: 64 // bits to hold 0 .. sigma
    return 64 // int(sigma).bit_length()


@pytest.mark.parametrize("sigma", [1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 255, 256])
def test_suffix_array_key_widths(bi, sigma):
    rng = np.random.default_rng(sigma)
    alpha = rng.choice(256, sigma, replace=False).astype(np.uint8)
    cpk = _cpk(sigma)
    for n in sorted({1, cpk - 1, cpk, cpk + 1, 3 * cpk + 1, 4000}):
        if n < 1:
            continue
        body = alpha[rng.integers(0, sigma, n)]
        if n >= sigma:
            body[:sigma] = alpha                        # every symbol present: the key width is sigma's
        # below sigma bytes not every symbol fits: those texts run at the narrower width of the symbols they hold
        # (for sigma 255 and 256 only n = 4000 has the full width; cpk +- 1 is then covered by smaller sigmas)
        _check_sa(body.tobytes(), f"sigma {sigma} random")
        _check_sa(np.repeat(body[:max(1, n // 50)], 50)[:n].tobytes(), f"sigma {sigma} runs")


@pytest.mark.parametrize("n", [2 ** 16 - 1, 2 ** 16, 2 ** 16 + 1, 2 ** 20 + 1])
def test_suffix_array_powers_of_two(bi, n):
    rng = np.random.default_rng(n)
    t = bytearray(_rand(rng, n, b"ACGTN"))
    t[n // 3:n // 3 + n // 10] = (b"ACA" * n)[:n // 10]      # a tandem block: groups survive many rounds
    _check_sa(bytes(t), "acgtn + tandem")


def _fibonacci(n):
    a, b = b"A", b"AB"
    while len(b) < n:
        a, b = b, b + a
    return b[:n]


def _many_round_text(name):
    rng = np.random.default_rng(5)
    if name == "homopolymer":
        return b"A" * (1 << 20)
    if name == "fibonacci":
        return _fibonacci(1 << 20)
    if name == "block_x1000":
        return _mutate(rng, _rand(rng, 4096) * 1000, 0.001)
    p = int(name.split("_")[1])
    return (_rand(rng, p, b"ACGTN") * ((1 << 18) // p + 1))[:(1 << 18) + p // 2]


@pytest.mark.parametrize("name", ["homopolymer"] + [f"period_{p}" for p in (2, 3, 21, 22, 64, 171, 2000)]
                         + ["fibonacci", "block_x1000"])
def test_suffix_array_many_rounds(bi, name):
    _check_sa(_many_round_text(name), name)


@pytest.mark.parametrize("n", [1 << 24, (1 << 27) + 1])
def test_suffix_array_at_scale(bi, n):
    """ACGTN with ~1 % of the bytes in tandem arrays; the 2^27 + 1 case needs ~2.5 GB of host memory"""
    rng = np.random.default_rng(n)
    t = np.frombuffer(b"ACGTN", np.uint8)[rng.integers(0, 5, n, dtype=np.uint8)]
    for start in rng.integers(0, n - 5000, max(1, n // 100 // 5000)):
        unit = t[start:start + int(rng.integers(1, 50))].copy()
        t[start:start + 5000] = np.resize(unit, 5000)
    _check_sa(t.tobytes(), "acgtn at scale")


# ---- matching statistics: wide intervals -----------------------------------------------------------------------

@pytest.mark.parametrize("period,div", [(1, 0.0), (2, 0.0), (2, 0.02), (171, 0.0), (171, 0.01), (2000, 0.0),
                                        (2000, 0.02)])
def test_ms_tandem_arrays(bi, period, div):
    """a genome array of ~600 kb (intervals past 64, 4096 and, for periods 1 and 2, 262144 suffixes) and a shorter
    one; the pivot carries ~10 kb of the same unit, with its own divergence"""
    rng = np.random.default_rng(period * 100 + int(div * 100))
    unit = _rand(rng, period)
    arr = lambda n: _mutate(rng, (unit * (n // period + 1))[:n], div)  # noqa: E731
    pivot = [_rand(rng, 3000) + arr(10_000) + _rand(rng, 3000), arr(4097), unit * 3]
    texts = [_rand(rng, 5000) + arr(600_000) + b"\0" + _rand(rng, 5000),
             _rand(rng, 2000) + arr(150_007) + _rand(rng, 10) + b"\0" + arr(65) + b"\0"]
    got = _ms(bi, pivot, texts, f"tandem p={period} div={div}")
    if div == 0:
        assert got[3000:12000, 0].min() >= 1000          # the pivot's array, matched up to its end


def test_ms_homopolymer_genome(bi):
    pivot = [b"A" * 20_000 + b"C" + b"A" * 5000, b"A" * 4097, b"GA" * 100 + b"A" * 65, b"A", b"CAT"]
    got = _ms(bi, pivot, [b"A" * 300_000, b"A" * 300_000 + b"\0C\0"], "homopolymer")
    assert got[0, 0] == 20_000


@pytest.mark.parametrize("genome_run", [1 << 15, 1 << 17])
def test_ms_n_runs(bi, genome_run):
    rng = np.random.default_rng(genome_run)
    pivot = [_rand(rng, 20_000) + b"N" * (1 << 16) + _rand(rng, 20_000)]
    texts = [_rand(rng, 30_000) + b"N" * genome_run + _rand(rng, 30_000) + b"\0" + pivot[0][:15_000] + b"\0"]
    got = _ms(bi, pivot, texts, f"N run 2^16 vs 2^{genome_run.bit_length() - 1}")
    assert got[20_000, 0] == min(1 << 16, genome_run)


# ---- long exact matches, every byte value ---------------------------------------------------------------------

def test_ms_long_exact_matches(bi):
    rng = np.random.default_rng(1)
    whole = _rand(rng, 1_000_000)
    pivot = [whole[:700_000], whole[700_000:999_999], whole[999_999:]]       # the text goes on past record ends
    snp = bytearray(whole)
    snp[50_000::100_000] = bytes(ord("C") if c == ord("A") else ord("A") for c in snp[50_000::100_000])
    texts = [bi.genome_text([whole]), bi.genome_text([bytes(snp)])]
    got = _ms(bi, pivot, texts, "identical genome and SNP every 1e5")
    assert got[:700_000, 0].tolist() == list(range(700_000, 0, -1))


def test_ms_every_byte_value(bi):
    rng = np.random.default_rng(255)
    nz = bytes(range(1, 256))
    pivot = [_rand(rng, 60_000, nz) + b"\xff" * 3000 + _rand(rng, 200, nz), nz, nz[::-1], b"\x01" * 300]
    texts = [b"\0".join([pivot[0][10_000:40_000], _mutate(rng, pivot[0], 0.01, nz), b"\xff" * 2000, nz]) + b"\0",
             _rand(rng, 300_000, nz + b"\0")]
    _ms(bi, pivot, texts, "every byte value")
    _ms(bi, pivot, texts, "every byte value", chunk=1)


# ---- structural sizes -----------------------------------------------------------------------------------------

LENGTHS = [64, 65, 255, 257, 4096, 4097, 256 * 37 - 1, 256 * 37 + 1, 262_144, 262_145, 256 * 1001 - 1, 256 * 1001 + 1]


def test_ms_text_lengths_at_structural_boundaries(bi):
    """raw NUL-separated texts of exact lengths (genome_text only makes even ones), one column each, added in a
    mixed order to one handle"""
    rng = np.random.default_rng(64)
    pivot = [_rand(rng, 1000, b"ACGTN"), _rand(rng, 1999), b"G"]
    seq = b"".join(pivot)
    base = b"\0".join(_mutate(rng, seq, 0.01) for _ in range(4)) + b"\0" + b"A" * 300 + b"\0"
    texts = [(base * (n // len(base) + 1))[:n] for n in LENGTHS]
    order = rng.permutation(len(texts))
    _, rb = M.records_layout(pivot)
    with bi.MatchingStatistics(seq, rb, len(texts)) as ms:
        for c in order:
            ms.add(texts[c], int(c))
        got = ms.fetch()
        print(f"timings structural lengths: {ms.timings()}")
    for c, t in enumerate(texts):
        assert len(t) == LENGTHS[c]
        _same(got[:, c], M.ms(t, seq, rb), f"text of {len(t)} bytes")


@pytest.fixture(scope="module")
def many_records():
    rng = np.random.default_rng(20_000)
    lens = rng.choice([1, 2, 3, 127, 128, 129, 255], 20_000)
    whole = _rand(rng, int(lens.sum()))
    cut = np.concatenate([[0], np.cumsum(lens)])
    pivot = [whole[a:b] for a, b in zip(cut[:-1], cut[1:])]
    order = rng.permutation(len(pivot))
    texts = [_mutate(rng, whole, 0.005), b"\0".join(pivot[i] for i in order[:10_000]) + b"\0"]
    seq, rb = M.records_layout(pivot)
    return pivot, texts, [M.ms(t, seq, rb) for t in texts]


@pytest.mark.parametrize("chunk", [1, 3, 0, 129, 1 << 20])
def test_ms_many_records_every_chunk(bi, many_records, chunk):
    pivot, texts, want = many_records
    _ms(bi, pivot, texts, "20000 records", chunk=chunk, want=want)


# ---- one handle, many genomes ------------------------------------------------------------------------------------

def test_ms_handle_reuse(bi):
    """large, small, large, empty, large into columns out of order; then a column written twice and an empty genome
    over a filled column"""
    rng = np.random.default_rng(7)
    pivot = [_rand(rng, 150_000), _rand(rng, 50_000, b"ACGTN")]
    seq, rb = M.records_layout(pivot)
    big = lambda r: b"\0".join([_mutate(rng, seq, r), _rand(rng, 800_000)]) + b"\0"  # noqa: E731
    large1, small, large2, large3, small2 = big(0.01), pivot[1][:100] + b"\0", big(0.001), big(0.05), seq[5:3005]
    want = {0: small, 1: b"", 2: large3, 3: small2, 4: b""}
    with bi.MatchingStatistics(seq, rb, 5) as ms:
        for text, col in ((large1, 3), (small, 0), (large2, 4), (b"", 1), (large3, 2), (small2, 3), (b"", 4)):
            ms.add(text, col)
        got = ms.fetch()
        print(f"timings handle reuse: {ms.timings()}")
    for col, text in want.items():
        _same(got[:, col], M.ms(text, seq, rb), f"column {col}")
    assert not got[:, [1, 4]].any()


# ---- a DAP matrix past 2^31 entries ---------------------------------------------------------------------------

def _dap_all(conv, batches):
    out = list(batches) + [conv.finish()]
    return [np.concatenate([b[i] for b in out]) for i in range(4)]


def test_ms_matrix_past_2_31_entries(bi):
    """4096 columns x (2^19 + 3) positions (8.6 GB): the rows past entry 2^31 through fetch and memo_ms_push_dap"""
    from memo_amd.dap_to_bed import DapConverter
    rng = np.random.default_rng(31)
    C, npos = 4096, (1 << 19) + 3
    pivot = [_rand(rng, 1 << 18), _rand(rng, (1 << 18) + 2), b"T"]
    seq, rb = M.records_layout(pivot)
    assert rb[-1] == npos and npos * C > 2 ** 31
    texts = {0: bi.genome_text([_mutate(rng, seq, 0.01)]), 1: bi.genome_text([seq[::-1]]),
             4095: bi.genome_text([_mutate(rng, seq, 0.001)])}
    tail = 700                                           # rows npos - 700 .. npos - 1; 2^31 / 4096 = 2^19 is inside
    assert (npos - 3) * C >= 2 ** 31                     # the last fetch and push_ms below start past entry 2^31
    with bi.MatchingStatistics(seq, rb, C) as ms:
        for col, t in texts.items():
            ms.add(t, col)
        print(f"timings 4096 columns: {ms.timings()}")
        head = ms.fetch(0, 300)
        last = ms.fetch(npos - tail, tail)
        for block in (1, 3, 299, 400):                  # 1 and 3: slices that start past 2^31 entries
            _same(ms.fetch(npos - block, block).ravel(), last[tail - block:].ravel(), f"fetch of the last {block}")
        with DapConverter(C, np.array([0, tail]), True, True) as dev, DapConverter(C, np.array([0, tail]), True, True) as host:
            got = _dap_all(dev, [dev.push_ms(ms, npos - tail, 400), dev.push_ms(ms, npos - 300, 297),
                                 dev.push_ms(ms, npos - 3, 3)])
            want = _dap_all(host, [host.push(last[:400]), host.push(last[400:697]), host.push(last[697:])])
    others = np.setdiff1d(np.arange(C), list(texts))
    assert not head[:, others].any() and not last[:, others].any()
    for col, t in texts.items():
        ms_col = M.ms(t, seq, rb)
        _same(head[:, col], ms_col[:300], f"column {col} head")
        _same(last[:, col], ms_col[-tail:], f"column {col} past 2^31 entries")
    for g, w, what in zip(got, want, ("rec", "start", "end", "annot")):
        _same(g, w, f"device DAP rows past 2^31 entries: {what}")
    for g, w in zip(got, dap_oracle.dap_rows(last, np.array([0, tail]), True, True)):
        _same(g, w, "device DAP rows against dap_oracle")


# ---- device DAP against host DAP -------------------------------------------------------------------------------

def test_device_dap_equals_host_dap_and_the_oracle(bi):
    from memo_amd.dap_to_bed import DapConverter
    rng = np.random.default_rng(99)
    pivot = [_rand(rng, int(n)) for n in rng.choice([1, 2, 50, 127, 128, 3000, 40_000], 60)]
    seq, rb = M.records_layout(pivot)
    texts = [bi.genome_text([_mutate(rng, seq, r)]) for r in (0.001, 0.01, 0.05)] + [b"\0".join(pivot[:7]) + b"\0"]
    with bi.MatchingStatistics(seq, rb, len(texts)) as ms:
        for c, t in enumerate(texts):
            ms.add(t, c)
        mat = ms.fetch()
        for c, t in enumerate(texts):
            _same(mat[:, c], M.ms(t, seq, rb), f"column {c}")
        npos = len(seq)
        for order in (False, True):
            want = dap_oracle.dap_rows(mat, rb, True, order)
            for block in (777, 4099, npos):
                starts = range(0, npos, block)
                with DapConverter(len(texts), rb, order, True) as dev, DapConverter(len(texts), rb, order, True) as host:
                    got = _dap_all(dev, [dev.push_ms(ms, s, min(block, npos - s)) for s in starts])
                    ref = _dap_all(host, [host.push(mat[s:s + block]) for s in starts])
                for g, h, w, what in zip(got, ref, want, ("rec", "start", "end", "annot")):
                    _same(g, h, f"push_ms vs push, order={order} block={block}: {what}")
                    _same(g, w, f"push_ms vs dap_oracle, order={order} block={block}: {what}")


# ---- end to end: FASTA -> `memo index` -> `memo query` against the chain of oracles ------------------------------

_IUPAC_COMPLEMENT = bytes.maketrans(b"ACGTRYKMBVDH", b"TGCAYRMKVBHD")   # samtools faidx -i; N, S, W, ... stay


def _text_of(seqs):
    """S_1 $ ... S_s $ rc(S_1) $ ... rc(S_s) $ with $ = NUL, restated for the oracle"""
    return b"".join(s + b"\0" for s in seqs) + b"".join(s.translate(_IUPAC_COMPLEMENT)[::-1] + b"\0" for s in seqs)


def _write_fasta(path, recs, rng):
    with open(path, "wb") as fh:
        for name, seq in recs:
            fh.write(b">" + name + b" some description\n")
            for i in range(0, len(seq), 60):
                line = seq[i:i + 60]
                fh.write((line.lower() if rng.random() < 0.3 else line) + b"\n")


@pytest.fixture(scope="module")
def pangenome(tmp_path_factory, bi):
    """~300 kb of pivot and genomes with tandem arrays, N runs, IUPAC codes and lowercase lines; one genome lacks a
    record, one carries more tandem copies and a longer N run"""
    rng = np.random.default_rng(300)
    work = tmp_path_factory.mktemp("ms_pan")
    unit = _rand(rng, 171)
    iupac = _rand(rng, 400, b"ACGTRYKMBVDHSWN")
    pivot = [(b"chr1", _rand(rng, 60_000) + unit * 60 + _rand(rng, 40_000) + b"N" * 3000 + _rand(rng, 30_000)),
             (b"chr2", _rand(rng, 20_000) + iupac + b"A" * 500 + _rand(rng, 20_000) + b"AC" * 800 + _rand(rng, 5000)),
             (b"chr3", _rand(rng, 700))]
    genomes = []
    for g in range(4):
        recs = [(name, _mutate(rng, seq, 0.002 * (g + 1))) for name, seq in pivot]
        if g == 1:
            recs = recs[:2]                                          # no chr3
        if g == 2:
            s1 = recs[0][1]
            recs[0] = (b"chr1", s1[:60_000] + unit * 90 + s1[60_000 + 171 * 60:-33_000] + b"N" * 5000 + s1[-30_000:])
        genomes.append(recs)
    files = [str(work / "pivot.fa")]
    _write_fasta(files[0], pivot, rng)
    for g, recs in enumerate(genomes):
        files.append(str(work / f"g{g}.fa"))
        _write_fasta(files[-1], recs, rng)
    (work / "list.txt").write_text("".join(f + "\n" for f in files))
    idx = {}
    for prefix, flags in (("cons", []), ("memb", ["-m"])):
        stats = bi.build_index(str(work / "list.txt"), str(work), prefix, bool(flags), log=lambda s: None)
        print(f"timings pangenome ({prefix}): sa {stats['sa_ms']:.1f} ms, lcp {stats['lcp_ms']:.1f} ms, "
              f"walk {stats['walk_ms']:.1f} ms")
        idx[prefix] = str(work / (prefix + ".parquet"))
    seq, rb = M.records_layout([s for _, s in pivot])
    mat = np.stack([M.ms(_text_of([s for _, s in recs]), seq, rb) for recs in genomes], axis=1)
    return dict(work=work, pivot=pivot, rb=rb, mat=mat, idx=idx, n_docs=len(genomes) + 1)


@pytest.mark.parametrize("membership", [False, True], ids=["conservation", "membership"])
@pytest.mark.parametrize("k", [31, 101])
def test_pangenome_index_and_query_equal_the_oracle_chain(pangenome, k, membership):
    """MS oracle -> dap_oracle.dap_rows -> memo_oracle.conservation / membership -> the printed bytes, against the
    files `memo index` and `memo query` write, over whole records"""
    from memo_amd import memo_query as mq
    from oracle import memo_oracle as O
    P = pangenome
    rec, start, end, annot = dap_oracle.dap_rows(P["mat"], P["rb"], True, not membership)
    n = P["n_docs"]
    for r, (name, seq) in enumerate(P["pivot"]):
        L = len(seq)
        sel = rec == r
        rows = O.filter_rows(start[sel], end[sel], annot[sel], 0, L, k)
        if membership:
            want = O.emit_membership(O.membership(*rows, 0, L, k, n, literal=False), n)
        else:
            want = O.emit_conservation(O.conservation(*rows, 0, L, k, n, literal=False))
        out = str(P["work"] / f"{'m' if membership else 'c'}_{r}_{k}.txt")
        mq.main(mq.parse_arguments((["-m"] if membership else []) + [
            "-b", P["idx"]["memb" if membership else "cons"], "-k", str(k), "-n", str(n),
            "-r", f"{name.decode()}:0-{L}", "-o", out]))
        with open(out, "rb") as fh:
            got = fh.read()
        assert got == want, (name, k, membership, len(got), len(want))
