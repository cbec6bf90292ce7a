"""Run-coded matching-statistics columns (memo_ms_create_layout, MEMO_MS_LAYOUT_CODED): the layout `memo index` takes when the
dense DAP matrix int32 [positions][genomes - 1] does not fit on the device.  A coded handle must give, value for value, what a
dense handle and the suffix-automaton oracle give: whole, in ranges, as index rows, through `memo index`, and on a shape whose
matrix is larger than the device's whole memory.  The code itself is checked against a NumPy twin of its rule (exact counts and
bytes), and a column that does not fit against its message, through the A/B library's memo_debug_ms_free_bytes.

Not covered: the device is never filled to make an allocation fail for real (the seam stands in for it), and the free memory
the driver reports is not compared before and after the refused column (the runtime's own pools make that figure move); that
nothing leaks rests on the column's three move-only owners, and is observed through layout_info / column_info only."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import dap_oracle
from oracle import ms_oracle as M
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


@pytest.fixture(scope="module")
def block(bi):
    """positions per coding block, as the library reports it"""
    with bi.MatchingStatistics(b"ACGT", np.array([0, 4]), 1, layout="coded") as ms:
        info = ms.layout_info()
    assert info["layout"] == "coded" and info["block"] >= 64 and info["block"] & (info["block"] - 1) == 0
    return info["block"]


def _rand(rng, n, alpha=b"ACGT"):
    a = np.frombuffer(alpha, np.uint8)
    return a[rng.integers(0, len(a), n)].tobytes()


def _mutate(rng, seq, rate, alpha=b"ACGT"):
    """substitutions at `rate` (lengths stay)"""
    s = np.frombuffer(seq, np.uint8).copy()
    hit = rng.random(len(s)) < rate
    a = np.frombuffer(alpha, np.uint8)
    s[hit] = a[rng.integers(0, len(a), int(hit.sum()))]
    return s.tobytes()


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got.ravel() != want.ravel())
    assert not len(bad), (f"{what}: {len(bad)} entries differ, first {bad[:8].tolist()}: "
                          f"got {got.ravel()[bad[:8]].tolist()}, want {want.ravel()[bad[:8]].tolist()}")


def _twin_flags(ms_col, block):
    """the rule, restated: expect[i] = max(MS[i - 1] - 1, 0), MS[-1] = 0; flagged iff MS[i] != expect[i] or i starts a block"""
    ms_col = np.asarray(ms_col, np.int64)
    expect = np.maximum(np.concatenate([[0], ms_col[:-1]]) - 1, 0)
    flag = ms_col != expect
    flag[::block] = True
    return flag


def _twin_decode(ms_col, block):
    """decode(encode(column)) by the rule: MS[i] = max(value[j] - (i - j), 0), j the last flagged position <= i"""
    flag = _twin_flags(ms_col, block)
    idx = np.arange(len(ms_col))
    j = np.maximum.accumulate(np.where(flag, idx, 0))
    return np.maximum(np.asarray(ms_col, np.int64)[j] - (idx - j), 0)


def _column_bytes(positions, flagged, block):
    """the header's formula: bytes = 4 flagged + 8 (block / 64) nblocks + 8 nblocks"""
    nblocks = -(-positions // block)
    return 4 * flagged + 8 * (block // 64) * nblocks + 8 * nblocks


def _pivot(rng, shape, block):
    """pivot records: one record; many records whose lengths sit at the coding block +- 1, 64 +- 1 and 1; 20,000 records of one
    to three bases.  The first two hold a run of N and one stretch of every byte value 1 .. 255."""
    every = bytes(range(1, 256))
    if shape == "one":
        return [_rand(rng, 2500) + b"N" * 2300 + _rand(rng, 1500) + every + _rand(rng, 900)]
    if shape == "edges":
        lens = [block + 1, 1, block - 1, 63, block, 64, 1, 65, 1, 1, 2 * block + 1, 64, 63, block - 1, 1]
        recs = [_rand(rng, n) for n in lens]
        recs[2] = recs[2][:300] + b"N" * 1200 + recs[2][1500:]
        recs[10] = recs[10][:100] + every + recs[10][355:]
        return recs
    assert shape == "tiny"
    return [_rand(rng, int(n)) for n in rng.integers(1, 4, 20_000)]


def _families(rng, pivot, bi):
    """{name: genome records} around a pivot (list of records)"""
    whole = b"".join(pivot)
    n_at = whole.find(b"NNNN")
    fam = {}
    for rate in (0.001, 0.01, 0.1):
        fam[f"mutated {rate}"] = [_mutate(rng, r, rate) for r in pivot if len(r) > 3] or [_mutate(rng, whole, rate)]
    fam["unrelated"] = [_rand(rng, len(whole) // 2), _rand(rng, len(whole) // 3)]
    unit = whole[40:40 + 37]
    fam["tandem arrays"] = [unit * 60, (whole[200:211] * 150)[:1500] + unit[::-1] * 20]
    fam["homopolymer"] = [b"A" * 3000, b"C"]
    if n_at >= 0:                                                  # the pivot's N run, and a genome without one
        n_end = n_at + len(whole[n_at:]) - len(whole[n_at:].lstrip(b"N"))
        fam["N in the pivot only"] = [whole[:n_at] + _rand(rng, 50) + whole[n_end:]]
        fam["N in both"] = [whole[max(0, n_at - 700):n_end + 700]]
    fam["N in the genome only"] = [whole[:600] + b"N" * 900 + whole[600:1200], b"N" * 400]
    fam["every byte value"] = [bytes(range(1, 256)) * 3, bytes(range(255, 0, -1)), whole[:300]]
    fam["revcomp of the pivot"] = [bi.revcomp(whole[100:3000])]
    return fam


def _check_code(ms, got, block, what):
    """column_info of every column against the NumPy twin of the rule, exactly"""
    total = 0
    for c in range(got.shape[1]):
        info = ms.column_info(c)
        if not info["bytes"]:                                       # never added: no storage, zeros
            assert info["flagged"] == 0 and not got[:, c].any(), (what, c)
            continue
        flags = _twin_flags(got[:, c], block)
        assert info["flagged"] == int(flags.sum()), (what, c, info, int(flags.sum()))
        assert info["bytes"] == _column_bytes(len(got), info["flagged"], block), (what, c, info)
        _same(_twin_decode(got[:, c], block), got[:, c], f"{what}: the rule gives column {c} back")
        total += info["flagged"]
    assert ms.layout_info()["flagged"] == total


# ---- 1. coded == dense == the oracle ------------------------------------------------------------------------------

@pytest.mark.parametrize("chunk", [1, 7, 0])
@pytest.mark.parametrize("shape", ["one", "edges", "tiny"])
def test_coded_equals_dense_equals_the_oracle(bi, block, shape, chunk):
    rng = np.random.default_rng(1000 + 10 * ["one", "edges", "tiny"].index(shape) + chunk)
    pivot = _pivot(rng, shape, block)
    seq, rb = M.records_layout(pivot)
    fam = _families(rng, pivot, bi)
    names = list(fam)
    # columns: the families, an empty genome (add(b"")), a genome of no records, one column added twice, one never added
    C = len(names) + 4
    c_empty, c_norec, c_twice, c_never = len(names), len(names) + 1, len(names) + 2, len(names) + 3
    want = np.zeros((len(seq), C), np.int32)
    for c, name in enumerate(names):
        want[:, c] = M.ms(bi.genome_text(fam[name]), seq, rb)
    want[:, c_twice] = want[:, 1]
    assert want[:, 0].max() > 50 or shape == "tiny"

    def fill(ms, by_records):
        for c, name in enumerate(names):
            if by_records:                       # a forced cap that gives several pieces: the merge path
                recs = fam[name]
                cap = max(len(s) for s in recs) + 1 + (c % 3) * 40
                n_pieces = ms.add_records(recs, c, cap)
                assert n_pieces == bi.plan_pieces([len(s) for s in recs], cap)[0] and n_pieces >= 2, (name, n_pieces)
            else:
                ms.add(bi.genome_text(fam[name]), c)
        ms.add(b"", c_empty)
        assert ms.add_records([], c_norec) == 0
        ms.add(bi.genome_text(fam[names[0]]), c_twice)
        if by_records:
            ms.add_records(fam[names[1]], c_twice, 0)
        else:
            ms.add(bi.genome_text(fam[names[1]]), c_twice)          # the second content wins
    with bi.MatchingStatistics(seq, rb, C, 0, chunk, layout="dense") as dense:
        fill(dense, False)
        assert dense.layout_info()["layout"] == "dense"
        assert dense.column_info(0) == {"flagged": 0, "bytes": 4 * len(seq)}
        d = dense.fetch()
    _same(d, want, f"{shape} chunk {chunk}: dense against the oracle")
    for by_records in (False, True):
        what = f"{shape} chunk {chunk} {'add_records in pieces' if by_records else 'add'}"
        with bi.MatchingStatistics(seq, rb, C, 0, chunk, layout="coded") as coded:
            assert not coded.fetch().any(), "a coded handle with no column added reads as zeros"
            fill(coded, by_records)
            got = coded.fetch()
            info = coded.layout_info()
            assert info["layout"] == "coded" and info["block"] == block
            for c, name in enumerate(names):
                _same(got[:, c], want[:, c], f"{what}: coded column {c} ({name}) against the oracle")
            _same(got, d, f"{what}: coded against dense")
            assert not got[:, [c_empty, c_norec, c_never]].any()
            assert coded.column_info(c_never) == {"flagged": 0, "bytes": 0}
            assert coded.column_info(c_empty)["flagged"] == -(-len(seq) // block)        # the block starts alone
            _check_code(coded, got, block, what)
            held = sum(coded.column_info(c)["bytes"] for c in range(C))
            assert info["device_bytes"] >= held + 4 * len(seq) and info["dense_bytes"] == 4 * len(seq) * C
            print(f"{what}: flagged {info['flagged']} of {len(seq) * C}, {info['device_bytes']} B held (dense {info['dense_bytes']}), "
                  f"encode {info['encode_ms']:.2f} ms decode {info['decode_ms']:.2f} ms")


# ---- 2. ranges ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", [3, 70])
def test_fetch_ranges(bi, block, C):
    """any first and any length: off by one around block edges and 64-position word edges, lengths 0 and 1, the whole pivot;
    70 columns: two column groups of the decode kernel, most columns never added"""
    rng = np.random.default_rng(64 + C)
    pivot = [_rand(rng, block + 37), _rand(rng, 1), _rand(rng, 2 * block - 5), _rand(rng, 700)]
    seq, rb = M.records_layout(pivot)
    npos = len(seq)
    cols = {0: 0.002, 1: 0.05, C - 1: 0.3, C // 2: 0.0}
    with bi.MatchingStatistics(seq, rb, C, layout="coded") as ms:
        for c, rate in cols.items():
            ms.add(bi.genome_text([_mutate(rng, seq, rate)]), c)
        full = ms.fetch()
        for c in cols:
            assert full[:, c].max() > 8
        assert not np.delete(full, list(cols), axis=1).any()
        assert full.shape == (npos, C) and ms.fetch(0, npos).tolist() == full.tolist()
        edges = sorted({e + d for e in list(range(0, npos + 1, block)) + list(range(0, npos + 1, 64))[:12] + [npos - 64, npos]
                        for d in (-1, 0, 1) if 0 <= e + d <= npos})
        ranges = [(a, n) for a in edges for n in (0, 1, 2, 63, 64, 65) if a + n <= npos]
        ranges += [(a, b - a) for a in edges[::7] for b in edges[::5] if a <= b]
        for _ in range(300):
            a = int(rng.integers(0, npos + 1))
            ranges.append((a, int(rng.integers(0, npos - a + 1))))
        ranges += [(npos, 0), (0, 0), (npos - 1, 1), (0, npos)]
        assert len(ranges) > 500
        for a, n in ranges:
            got = ms.fetch(a, n)
            assert got.shape == (n, C)
            _same(got, full[a:a + n], f"fetch({a}, {n}) of {npos} positions, {C} columns")
        from memo_amd._lib import MemoError
        for a, n in ((-1, 2), (npos, 1), (0, npos + 1)):
            with pytest.raises(MemoError, match="outside the pivot"):
                ms.fetch(a, n)


# ---- 3. the code is what the rule says ---------------------------------------------------------------------------

def test_the_code_is_what_the_rule_says(bi, block):
    """flagged positions and bytes of the mutated-copy and unrelated families, counted on the ORACLE's columns with the twin
    of the rule: exact, no tolerance"""
    rng = np.random.default_rng(3)
    for shape in ("one", "edges", "tiny"):
        pivot = _pivot(rng, shape, block)
        seq, rb = M.records_layout(pivot)
        texts = [bi.genome_text([_mutate(rng, seq, rate)]) for rate in (0.001, 0.01, 0.1)] + [bi.genome_text([_rand(rng, len(seq))])]
        with bi.MatchingStatistics(seq, rb, len(texts), layout="coded") as ms:
            for c, t in enumerate(texts):
                ms.add(t, c)
            shares = []
            for c, t in enumerate(texts):
                flags = _twin_flags(M.ms(t, seq, rb), block)
                info = ms.column_info(c)
                assert info["flagged"] == int(flags.sum()), (shape, c)
                assert info["bytes"] == _column_bytes(len(seq), int(flags.sum()), block), (shape, c)
                shares.append(info["flagged"] / len(seq))
            print(f"{shape}: flagged share at 0.1 % / 1 % / 10 % substitutions / unrelated: {['%.4f' % s for s in shares]}")


# ---- 4. rows -----------------------------------------------------------------------------------------------------

def _cat(batches):
    return [np.concatenate([b[i] for b in batches]) for i in range(4)]


def _pushes(conv, ms, sizes, npos):
    """pushes of the given sizes (the last size repeats to the end), then finish()"""
    out, first = [], 0
    sizes = list(sizes)
    while first < npos:
        n = min(sizes.pop(0) if len(sizes) > 1 else sizes[0], npos - first)
        out.append(conv.push_ms(ms, first, n))
        first += n
    return _cat(out + [conv.finish()])


def test_rows_of_a_coded_handle(bi, block):
    """push_ms in pushes of 1 (the first 2,500 positions one by one, then the rest at once), 255, 256, 257 and 10^4 positions:
    a coded handle gives the rows a dense handle gives for the same pushes, conservation and membership order"""
    from memo_amd.dap_to_bed import DapConverter
    rng = np.random.default_rng(44)
    pivot = [_rand(rng, n) for n in (block - 1, 1, 9000, 256, 255, 257, 1, 7000, 2 * block + 3, 2)]
    seq, rb = M.records_layout(pivot)
    npos = len(seq)
    assert npos > 2 * 10 ** 4
    texts = [bi.genome_text([_mutate(rng, seq, r)]) for r in (0.0, 0.003, 0.02, 0.3)] + [b"", bi.genome_text([_rand(rng, 4000)])]
    C = len(texts) + 1                                               # the last column is never added
    with bi.MatchingStatistics(seq, rb, C, layout="dense") as dense, bi.MatchingStatistics(seq, rb, C, layout="coded") as coded:
        for c, t in enumerate(texts):
            dense.add(t, c)
            coded.add(t, c)
        mat = dense.fetch()
        _same(coded.fetch(), mat, "the matrix")
        for order in (True, False):
            want = dap_oracle.dap_rows(mat, rb, True, order)
            for sizes in ([1] * 2500 + [npos], [255], [256], [257], [10 ** 4]):
                what = f"order={order}, pushes of {sizes[0]}"
                with DapConverter(C, rb, order, True) as a, DapConverter(C, rb, order, True) as b:
                    rows_dense, rows_coded = _pushes(a, dense, sizes, npos), _pushes(b, coded, sizes, npos)
                for g, d, w, f in zip(rows_coded, rows_dense, want, ("rec", "start", "end", "annot")):
                    _same(g, d, f"{what}: {f}, coded against dense")
                    _same(g, w, f"{what}: {f}, coded against dap_oracle")


# ---- 5. the command ------------------------------------------------------------------------------------------------

def test_memo_index_with_coded_columns_equals_the_golden_index(bi, tmp_path):
    import pyarrow.parquet as pq
    longest = max(len(s) for p in EXAMPLE for _, s in bi.read_fasta(p))
    lst = tmp_path / "genome_list.txt"
    lst.write_text("".join(p + "\n" for p in EXAMPLE))
    base = {k: v for k, v in os.environ.items() if k not in ("MEMO_INDEX_DAP_LAYOUT", "MEMO_INDEX_PIECE_BYTES")}
    for n, extra in enumerate(({}, {"MEMO_INDEX_PIECE_BYTES": str(longest + 1)})):
        env = dict(base, MEMO_INDEX_DAP_LAYOUT="coded", MEMO_INDEX_STATS=str(tmp_path / f"stats{n}.json"), **extra)
        for flag, prefix, golden in (([], "test", "example_cons.parquet"), (["-m"], "memb", "example_memb.parquet")):
            out = tmp_path / f"w{n}"
            r = subprocess.run([sys.executable, EXE, "index", "-g", str(lst), "-o", str(out), "-p", prefix] + flag,
                               capture_output=True, timeout=300, env=env)
            assert r.returncode == 0, r.stderr
            assert r.stdout.decode().splitlines()[-1] == "DONE"
            got, want = pq.read_table(str(out / (prefix + ".parquet"))), pq.read_table(os.path.join(G.GOLD, golden))
            assert got.schema.names == ["f0", "f1", "f2", "f3"]
            assert [str(t) for t in got.schema.types] == ["string", "int64", "int64", "int64"]
            assert pq.ParquetFile(str(out / (prefix + ".parquet"))).metadata.row_group(0).column(1).compression == "ZSTD"
            for col in ("f0", "f1", "f2", "f3"):
                assert got.column(col).to_pylist() == want.column(col).to_pylist(), (extra, prefix, col)
            import json
            said = json.loads((tmp_path / f"stats{n}.json").read_text())      # the command's own account of what ran
            assert said["dap_layout"] == "coded" and said["rows"] == got.num_rows and not list(out.glob("*.part"))
    # what ran: the layout the variable names; unset, the matrix (it fits)
    quiet = lambda s: None  # noqa: E731
    st = bi.build_index(str(lst), str(tmp_path / "s1"), "x", False, log=quiet,
                        layout=bi.dap_layout_from_env({"MEMO_INDEX_DAP_LAYOUT": "coded"}))
    assert st["dap_layout"] == "coded" and all(g["flagged"] > 0 for g in st["per_genome"]) and st["dap_device_bytes"] > 0
    st1 = bi.build_index(str(lst), str(tmp_path / "s2"), "x", False, log=quiet, piece_bytes=longest + 1, layout="coded")
    assert st1["dap_layout"] == "coded" and st1["pieces"] == [2 * len(bi.read_fasta(p)) for p in EXAMPLE[1:]]
    assert [g["flagged"] for g in st1["per_genome"]] == [g["flagged"] for g in st["per_genome"]]
    st2 = bi.build_index(str(lst), str(tmp_path / "s3"), "x", False, log=quiet, layout=bi.dap_layout_from_env({}))
    assert st2["dap_layout"] == "dense" and all(g["flagged"] == 0 for g in st2["per_genome"])
    assert st2["dap_device_bytes"] == 4 * st2["positions"] * (len(EXAMPLE) - 1)
    assert st["rows"] == st1["rows"] == st2["rows"]
    for d in ("s1", "s2", "s3"):
        assert pq.read_table(str(tmp_path / d / "x.parquet")).equals(pq.read_table(str(tmp_path / "w0" / "test.parquet")))


# ---- 6. a shape the dense layout refuses ---------------------------------------------------------------------------

def test_a_pivot_whose_matrix_is_larger_than_the_device(bi, block):
    """4096 columns over a pivot long enough that the matrix passes the device's TOTAL memory: memo_ms_create refuses, AUTO
    codes.  The homologous slice is 3 * 2^20 positions.  fetch returns every column, 16 KiB per position, so the 4096-column
    handle is fetched on windows (the two ends of the slice, its middle, the pivot's ends, a record end, seeded ones), and
    the whole slice is checked on a second coded handle of the same pivot that holds the same genomes in 3 columns; the two
    handles must agree on every window and on the flagged count of every column (the whole column, exactly)."""
    import ctypes as C_
    import torch
    from memo_amd._lib import MemoError, check, lib
    from memo_amd.dap_to_bed import DapConverter
    _, total = torch.cuda.mem_get_info()
    C = 4096
    npos = (total // (C * 4) + (1 << 16)) & ~0xFFF | 0x41                  # past the device's memory, and no round number
    assert npos * C * 4 > total
    rng = np.random.default_rng(4096)
    letters = np.frombuffer(b"ACGT", np.uint8)
    seq = letters[rng.integers(0, 4, npos, dtype=np.uint8)].tobytes()
    rb = np.array([0, npos // 2 + 11, npos // 2 + 12, npos - 70_001, npos], np.int64)
    h = C_.c_void_p()
    with pytest.raises(MemoError, match="device memory"):
        check(lib().memo_ms_create(seq, rb.ctypes.data, len(rb) - 1, C, 0, 0, C_.byref(h)))
    assert not h.value
    with pytest.raises(MemoError, match="device memory"):
        bi.MatchingStatistics(seq, rb, C, layout="dense")
    L, pad = 3 << 20, 4096
    w0 = int(rb[2]) + 123_457                                            # the homologous slice, inside record 2
    w1 = w0 + L
    assert w1 + pad < rb[3]
    genomes = {0: [_mutate(rng, seq[w0:w1], 0.01)], 1: [_rand(rng, 1 << 20), _rand(rng, 300_000)], 4095: []}
    windows = [(w0, w1), (0, 3000), (npos - 2000, npos), (int(rb[1]) - 1500, int(rb[1]) + 1), (w0 - 5000, w0 + 100)]
    wide = [(w0, w0 + 70_000), (w1 - 70_000, w1 + 300), ((w0 + w1) // 2 - 111, (w0 + w1) // 2 + 40_000)] + windows[1:]
    for _ in range(4):
        a = int(rng.integers(0, npos - 20_000))
        windows.append((a, a + int(rng.integers(1, 6000))))
        wide.append(windows[-1])
    step = 1 << 15
    narrow_of = {0: 0, 1: 1, 4095: 2}
    with bi.MatchingStatistics(seq, rb, C) as ms, bi.MatchingStatistics(seq, rb, 3, layout="coded") as narrow:
        assert ms.layout_info()["layout"] == "coded"
        for c, recs in genomes.items():
            ms.add_records(recs, c)
            narrow.add_records(recs, narrow_of[c])
            assert ms.column_info(c) == narrow.column_info(narrow_of[c])
        info = ms.layout_info()
        print(f"{npos} positions x {C} columns: dense {info['dense_bytes'] / 1e9:.1f} GB refused (device {total / 1e9:.1f} GB), "
              f"{info['device_bytes'] / 1e6:.1f} MB held, flagged {[ms.column_info(c)['flagged'] for c in genomes]}, "
              f"encode {info['encode_ms']:.1f} ms, {ms.timings()}")
        assert info["dense_bytes"] == npos * C * 4 and info["device_bytes"] < info["dense_bytes"] // 1000
        # the oracle once per genome, on the windows' pivot slices [a, min(b + pad, end of the pivot)) laid back to back as
        # records of their own (cut again where a real record ends inside one)
        offs, sl_rb, ends, last_cut = [], [0], [], []
        for a, b in windows:
            end = min(b + pad, npos)
            cuts = [int(c) for c in rb if a < c < end]
            offs.append(sl_rb[-1])
            for c0, c1 in zip([a] + cuts, cuts + [end]):
                sl_rb.append(sl_rb[-1] + c1 - c0)
            ends.append(end)
            last_cut.append(max([a] + cuts))
        cat = b"".join(seq[a:end] for (a, _), end in zip(windows, ends))
        want = {c: M.ms(bi.genome_text(recs), cat, np.array(sl_rb, np.int64)) for c, recs in genomes.items() if recs}
        for (a, b), off, end, cut in zip(windows, offs, ends, last_cut):
            for c, w in want.items():
                # no match of a checked position reaches the end of its slice (unless the pivot or a record of it ends there):
                # every checked value is the MS against the whole pivot
                p = np.arange(cut, b)
                reach = p + w[off + cut - a:off + b - a] if cut < b else np.zeros(1, np.int64)
                assert end in rb or int(reach.max()) < end, (a, b, c, int(reach.max()), end)
            got = narrow.fetch(a, b - a)                             # every window, the whole slice among them: 3 columns
            for c, w in want.items():
                _same(got[:, narrow_of[c]], w[off:off + b - a], f"window [{a}, {b}) column {c}, 3-column handle")
            assert not got[:, 2].any(), (a, b)
        for a, b in wide:                                             # the 4096-column handle against the 3-column one
            for s in range(a, b, step):
                n = min(step, b - s)
                got, ref = ms.fetch(s, n), narrow.fetch(s, n)
                for c, k in narrow_of.items():
                    _same(got[:, c], ref[:, k], f"window [{a}, {b}) column {c} at {s}: 4096 columns against 3")
                assert not got[:, 2:].any(), (a, b, s)
        assert ms.fetch(w0, 5000)[:, 0].max() > 100                     # (the homologous slice does match)
        head = ms.fetch(0, 3000)
        for order in (True, False):
            with DapConverter(C, rb, order, True) as conv:
                got = _cat([conv.push_ms(ms, 0, 1000), conv.push_ms(ms, 1000, 1), conv.push_ms(ms, 1001, 1999), conv.finish()])
            for g, w, f in zip(got, dap_oracle.dap_rows(head, rb, True, order), ("rec", "start", "end", "annot")):
                _same(g, w, f"rows of the first 3000 positions, order={order}: {f}")
        print(f"decode {ms.layout_info()['decode_ms']:.1f} ms in all")


# ---- 7. a column that does not fit ---------------------------------------------------------------------------------

def test_a_column_that_does_not_fit_is_refused_and_leaves_the_handle_good(bi, block):
    from memo_amd import _lib
    from memo_amd._lib import MemoError
    rng = np.random.default_rng(77)
    pivot = [_rand(rng, 30_000), _rand(rng, 20_001)]
    seq, rb = M.records_layout(pivot)
    near, far = bi.genome_text([_mutate(rng, seq, 0.01)]), bi.genome_text([_rand(rng, 40_000)])
    flag_bytes = 8 * (block // 64) * -(-len(seq) // block)
    L = _lib.use_ab()
    try:
        with bi.MatchingStatistics(seq, rb, 3, layout="coded") as ms:
            ms.add(near, 0)
            ms.add(far, 2)
            before, held = ms.fetch(), ms.layout_info()["device_bytes"]
            far_bytes = 4 * ms.column_info(2)["flagged"]
            assert far_bytes > flag_bytes + 1
            # the budget holds the flag words, not the values
            _lib.check(L.memo_debug_ms_free_bytes(flag_bytes + 1))
            with pytest.raises(MemoError, match=rf"coded column 1: its flagged values need {far_bytes} bytes of device memory, "
                                                rf"{flag_bytes + 1} bytes are free"):
                ms.add(far, 1)
            # ... nor even the flag words
            _lib.check(L.memo_debug_ms_free_bytes(100))
            with pytest.raises(MemoError, match=rf"coded column 1: its flag words need {flag_bytes} bytes of device memory, 100 bytes"):
                ms.add_records([far[:500]], 1)
            assert ms.column_info(1) == {"flagged": 0, "bytes": 0} and ms.layout_info()["device_bytes"] == held
            _same(ms.fetch(), before, "after the refused column")
            # a column that held something loses it (its buffers went first), the others stay
            with pytest.raises(MemoError, match="coded column 2"):
                ms.add(near, 2)
            assert ms.column_info(2) == {"flagged": 0, "bytes": 0}
            after = ms.fetch()
            _same(after[:, 0], before[:, 0], "column 0")
            assert not after[:, 1:].any()
            assert ms.layout_info()["device_bytes"] == held - _column_bytes(len(seq), far_bytes // 4, block)
            _lib.check(L.memo_debug_ms_free_bytes(-1))
            ms.add(far, 2)
            ms.add(near, 1)
            got = ms.fetch()
            _same(got[:, 2], before[:, 2], "column 2 added again")
            _same(got[:, 1], before[:, 0], "column 1 at last")
    finally:
        L.memo_debug_ms_free_bytes(-1)
        _lib.use_ab(False)
