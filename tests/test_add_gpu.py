"""`memo add` on the GPU: add_dap_kernel alone through the C ABI against NumPy, memo_ms_rows_dev against memo_ms_fetch on a dense and on
a coded handle, memo_amd.add.rows / add_index against the definition (tests/add_oracle.py) on a seeded pangenome at every slice and batch
length and in both layouts of the matching statistics, and the command line against the committed example indexes.

Every comparison is exact."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import add_oracle
from tests import golden_util as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "memo")
FASTA = [os.path.join(G.GOLD, "example_fa", f"ref_{i}.fa") for i in range(1, 6)]
PAD = 0x5A5A5A5A
EINVAL = -1
OLD_COLS = (1, 2, 63, 64, 65, 100, 128)
NEW_COLS = (1, 2, 3, 63, 64, 65, 129)
WIDEST = ((2046, 1), (1, 2046))


@pytest.fixture(scope="module")
def memo():
    import memo_amd
    from memo_amd import _lib
    memo_amd.build()                     # make: a no-op when libmemo_amd.so is up to date
    assert _lib.lib().memo_device_count() > 0, "no HIP device: the product has no CPU fallback"
    return memo_amd


class Device:
    """device buffers the test lays out itself"""

    def __init__(self):
        from memo_amd._lib import check, lib
        self.check, self.lib, self.held = check, lib(), []

    def alloc(self, nbytes):
        d = C.c_void_p()
        self.check(self.lib.memo_dev_malloc(0, max(nbytes, 16), C.byref(d)))
        self.held.append(d)
        assert d.value % 16 == 0
        return d.value

    def upload(self, d, host):
        host = np.ascontiguousarray(host)
        if host.nbytes:
            self.check(self.lib.memo_dev_upload(0, d, host.ctypes.data, host.nbytes, None))

    def get(self, d, n, dtype):
        out = np.empty(n, dtype)
        if out.nbytes:
            self.check(self.lib.memo_dev_download(0, out.ctypes.data, d, out.nbytes, None))
        return out

    def close(self):
        for d in self.held:
            self.lib.memo_dev_free(0, d)
        self.held = []


@pytest.fixture()
def dev(memo):
    d = Device()
    yield d
    d.close()


def same_rows(got, want, note):
    assert len(got) == 3 and all(c.dtype == np.int64 for c in got), note
    assert [len(c) for c in got] == [len(c) for c in want], (note, [len(c) for c in got], [len(c) for c in want])
    for name, g, w in zip(("start", "end", "annot"), got, want):
        if not np.array_equal(g, w):
            i = int(np.flatnonzero(g != w)[0])
            raise AssertionError(f"{note}: {name} differs in {(g != w).sum()} of {len(w)} rows, first at row {i}: got {g[i]}, want {w[i]}")


# ---------------------------------------------------------------------------------------
# the kernel alone, through the C ABI
# ---------------------------------------------------------------------------------------
def cell_values(rng, cols, positions, remaining):
    """uint32 [cols, positions], all at least 1: values at, one under and one over remaining - i, 2^31 - 1, and anything a uint32 holds"""
    room = remaining - np.arange(positions, dtype=np.int64)[None, :]
    kind = rng.integers(0, 6, (cols, positions))
    v = room + (kind - 1)                                          # kinds 0, 1, 2: one under, at, one over
    v = np.where(kind == 3, 2 ** 31 - 1, v)
    v = np.where(kind == 4, rng.integers(1, 2 ** 32, (cols, positions)), v)
    v = np.where(kind == 5, rng.integers(1, 300, (cols, positions)), v)
    return np.clip(v, 1, 2 ** 32 - 1).astype(np.uint32)


@pytest.mark.parametrize("old,new", [(o, n) for o in OLD_COLS for n in NEW_COLS] + list(WIDEST))
def test_the_kernel_against_numpy(memo, dev, old, new):
    """Every cell outside [first, first + positions) of planes 1 .. N - 1 -- plane 0, the cells left and right of the range, the pad up
    to the pitch -- is 0, and so are the four words on either side of the new rows; every value inside either source is at least 1 (as a
    uint32: the new rows hold negative int32 too) and so is remaining - i: a value read from outside would show as a 0.  The output lies
    between words of PAD that must stay."""
    from memo_amd import add
    T = add.tile()
    assert T == 128
    n, W = old + 1, old + new
    rng = np.random.default_rng(10000 * old + new)
    longest = 2 * T + 1
    pitch = ((3 + longest + 3) & ~3) + 64
    d_cells, d_new, d_out = dev.alloc(4 * n * pitch), dev.alloc(4 * (longest * new + 8)), dev.alloc(4 * (longest * W + 8))
    calls = 0
    for positions in (0, 1, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1):
        for first in (0, 1, 3, pitch - positions):                 # the last one ends exactly at the pitch
            for remaining in (positions, positions + 1000, 2 ** 31 - 1):
                cells = np.zeros((n, pitch), np.uint32)
                cells[1:, first:first + positions] = cell_values(rng, old, positions, remaining)
                fresh = np.zeros(longest * new + 8, np.uint32)
                fresh[4:4 + positions * new] = cell_values(rng, new, positions, remaining).T.reshape(-1)      # [positions][new]
                dev.upload(d_cells, cells)
                dev.upload(d_new, fresh)
                dev.upload(d_out, np.full(longest * W + 8, PAD, np.uint32))
                dev.check(dev.lib.memo_add_dap_dev(d_cells, pitch, n, first, positions, remaining, d_new + 16, new, d_out + 16, 0, None))
                got = dev.get(d_out, longest * W + 8, np.uint32)
                assert (got[:4] == PAD).all() and (got[4 + positions * W:] == PAD).all(), (positions, first, remaining)
                both = np.hstack([cells[1:, first:first + positions].T.astype(np.int64), fresh[4:4 + positions * new].reshape(positions, new).astype(np.int64)])
                want = np.minimum(both, remaining - np.arange(positions, dtype=np.int64)[:, None])
                assert want.shape == (positions, W) and (want.size == 0 or want.min() >= 1)
                got = got[4:4 + positions * W].view(np.int32).reshape(positions, W)
                if not np.array_equal(got, want):
                    i, c = np.argwhere(got != want)[0]
                    raise AssertionError(f"positions {positions}, first {first}, remaining {remaining}: {(got != want).sum()} of {want.size} differ, "
                                         f"first at row {i}, column {c}: got {got[i, c]}, want {want[i, c]}")
                calls += 1
    assert calls == 96


def test_the_kernel_through_the_module(memo):
    from memo_amd import add
    rng = np.random.default_rng(5)
    planes = rng.integers(0, 2 ** 32, (7, 301), dtype=np.uint64).astype(np.uint32)
    fresh = rng.integers(-2 ** 31, 2 ** 31, (299, 70), dtype=np.int64).astype(np.int32)
    got = add.dap(planes, fresh, 2, 299, 400)
    want = np.minimum(np.hstack([planes[1:, 2:].T.astype(np.int64), fresh.view(np.uint32).astype(np.int64)]), 400 - np.arange(299)[:, None])
    assert got.dtype == np.int32 and got.shape == (299, 76) and np.array_equal(got, want)
    assert add.dap(planes, np.zeros((0, 3), np.int32), 5, 0, 0).shape == (0, 9)


def test_the_kernel_refuses_before_it_launches(memo, dev):
    n, new, pitch, positions = 5, 3, 64, 40
    W = n - 1 + new
    cells = np.full((n, pitch), 7, np.uint32)
    d_cells, d_new, d_out = dev.alloc(cells.nbytes + 16), dev.alloc(4 * (positions * new + 8)), dev.alloc(4 * (positions * W + 8))
    dev.upload(d_cells, cells)
    dev.upload(d_new, np.full(positions * new + 8, 9, np.uint32))
    poison = np.full(positions * W + 8, PAD, np.uint32)
    dev.upload(d_out, poison)
    ok = dict(d_cells=d_cells, pitch=pitch, n=n, first=3, positions=positions, remaining=50, d_new=d_new + 16, new=new, d_out=d_out + 16)

    def call(a):
        return dev.lib.memo_add_dap_dev(a["d_cells"], a["pitch"], a["n"], a["first"], a["positions"], a["remaining"], a["d_new"], a["new"], a["d_out"], 0, None)
    for change, message in ((dict(n=1), b"num_docs"), (dict(n=2048), b"num_docs"), (dict(n=0), b"num_docs"),
                            (dict(new=0), b"new_cols"), (dict(new=2048), b"new_cols"), (dict(new=-1), b"new_cols"),
                            (dict(n=2047, new=2), b"the limit is 2047"), (dict(n=1025, new=1024), b"the limit is 2047"),
                            (dict(pitch=62), b"multiple of 4"), (dict(pitch=66), b"multiple of 4"),
                            (dict(first=25), b"do not lie inside"), (dict(first=pitch + 1, positions=0), b"do not lie inside"),
                            (dict(positions=62), b"do not lie inside"), (dict(remaining=39), b"remaining"), (dict(remaining=2 ** 31), b"2^31 - 1"),
                            (dict(d_cells=d_cells + 4), b"16-byte aligned"), (dict(d_cells=d_cells + 8), b"16-byte aligned"),
                            (dict(d_new=d_new + 18), b"d_new must be 4-byte aligned"), (dict(d_new=d_new + 17), b"d_new must be 4-byte aligned"),
                            (dict(d_out=d_out + 18), b"d_dap must be 4-byte aligned"), (dict(d_out=d_out + 17), b"d_dap must be 4-byte aligned"),
                            (dict(first=-1), b"negative"), (dict(positions=-1), b"negative"), (dict(pitch=-4), b"negative"),
                            (dict(remaining=-1, positions=0), b"negative"), (dict(d_out=0), b"NULL"), (dict(d_cells=0), b"NULL"), (dict(d_new=0), b"NULL")):
        rc = call(dict(ok, **change))
        assert rc == EINVAL and message in dev.lib.memo_last_error(), (change, dev.lib.memo_last_error())
        assert np.array_equal(dev.get(d_out, len(poison), np.uint32), poison), change
    # nothing to do launches nothing, whatever the pointers are
    assert call(dict(ok, d_cells=0, d_new=0, d_out=0, positions=0, remaining=0)) == 0
    assert np.array_equal(dev.get(d_out, len(poison), np.uint32), poison)
    dev.check(call(ok))
    got = dev.get(d_out, len(poison), np.uint32)
    assert (got[:4] == PAD).all() and (got[-4:] == PAD).all()
    room = (50 - np.arange(positions))[:, None]
    assert np.array_equal(got[4:-4].reshape(positions, W), np.hstack([np.minimum(7, room).repeat(n - 1, 1), np.minimum(9, room).repeat(new, 1)]))
    # the widest matrix the ABI takes on each side is taken
    assert call(dict(ok, n=2047, new=1, positions=0)) == 0 and call(dict(ok, n=2, new=2046, positions=0)) == 0


# ---------------------------------------------------------------------------------------
# the seeded pangenome
# ---------------------------------------------------------------------------------------
def _mutated(rng, seq, rate, alphabet=b"ACGT"):
    out = bytearray(seq)
    for i in np.flatnonzero(rng.random(len(out)) < rate):
        out[i] = alphabet[int(rng.integers(len(alphabet)))]
    return bytes(out)


class Pangenome:
    """A pivot of three records of 1, 300 and 1500 positions; old genomes, mutated copies, with or without one that lacks two pivot
    characters (made of C and G alone, so that neither A nor T occurs in it or in its reverse complement: the matching statistic is 0
    there and the index holds no row for it); three new genomes: a verbatim copy of the longest record, one that shares nothing with
    the pivot, and a mutated copy with a run of N."""

    def __init__(self, lacking):
        rng = np.random.default_rng(20 + lacking)
        letters = np.frombuffer(b"ACGT", np.uint8)
        self.pivot = [(name, letters[rng.integers(0, 4, length)].tobytes()) for name, length in (("one", 1), ("mid", 300), ("long", 1500))]
        seqs = [s for _, s in self.pivot]
        self.old = [[_mutated(rng, s, rate) for s in seqs[::step]] for rate, step in ((0.02, 1), (0.1, 1), (0.3, -1), (0.05, 1))]
        if lacking:
            self.old.insert(2, [s.replace(b"A", b"C").replace(b"T", b"G") for s in seqs])
        else:
            self.old.append([_mutated(rng, s, 0.2) for s in seqs])
        run = bytearray(_mutated(rng, seqs[2], 0.03))
        run[400:600] = b"N" * 200
        self.new = [[seqs[2]], [b"WS" * 333, b"SSW" * 50], [_mutated(rng, seqs[1], 0.05), bytes(run)]]
        self.n = len(self.old) + 1
        assert self.n == 6
        # every pivot character occurs in every old genome (the pivot's one-letter record included)?
        self.complete = all(all(bytes([c]) in add_oracle.genome_text(g) for c in set(b"".join(seqs))) for g in self.old)
        assert self.complete == (not lacking)
        self.index = add_oracle.built_rows(self.pivot, self.old, order=False)
        self.want = {order: add_oracle.index_rows(self.pivot, self.index, self.n, self.new, order) for order in (False, True)}
        if self.complete:                                              # the file `memo index` writes on the full list, by the oracles
            full = add_oracle.built_rows(self.pivot, self.old + self.new, order=False)
            assert all(np.array_equal(g, w) for g, w in zip(self.want[False][1:], [np.concatenate([full[n][i] for n, _ in self.pivot]) for i in range(3)]))

    def write(self, where):
        """the input index, the pivot and the genomes as files: (index path, list of the pivot and the new genomes, list of all)"""
        import pyarrow as pa
        import pyarrow.parquet as pq
        names = [name for name, _ in self.pivot for _ in self.index[name][0]]
        cols = [np.concatenate([self.index[name][i] for name, _ in self.pivot]) for i in range(3)]
        index = str(where / "old.parquet")
        pq.write_table(pa.table({"f0": pa.array(names, pa.utf8()), "f1": cols[0], "f2": cols[1], "f3": cols[2]}), index)

        def fasta(name, records):
            path = str(where / name)
            with open(path, "wb") as fh:
                for rec, seq in records:
                    fh.write(b">" + rec.encode() + b" described\n" + b"\n".join(seq[i:i + 70] for i in range(0, len(seq), 70)) + b"\n")
            return path
        pivot = fasta("pivot.fa", self.pivot)
        old = [fasta(f"old_{i}.fa", [(f"c{j}", s) for j, s in enumerate(g)]) for i, g in enumerate(self.old)]
        new = [fasta(f"new_{i}.fa", [(f"c{j}", s) for j, s in enumerate(g)]) for i, g in enumerate(self.new)]
        plus, full = str(where / "plus.txt"), str(where / "full.txt")
        open(plus, "w").write("".join(p + "\n" for p in [pivot] + new))
        open(full, "w").write("".join(p + "\n" for p in [pivot] + old + new))
        return index, plus, full


_PANGENOMES = {}


def _pangenome(lacking, factory):
    """built once a module, files and all"""
    if lacking not in _PANGENOMES:
        p = Pangenome(lacking)
        p.files = p.write(factory.mktemp("pan"))
        _PANGENOMES[lacking] = p
    return _PANGENOMES[lacking]


@pytest.fixture(scope="module", params=(1, 0), ids=("lacking", "complete"))
def pan(request, tmp_path_factory):
    return _pangenome(request.param, tmp_path_factory)


@pytest.fixture(scope="module")
def complete_pan(tmp_path_factory):
    return _pangenome(0, tmp_path_factory)


def _table(path):
    """(f0 as a list, f1, f2, f3) of a Parquet index, after the check that it has the schema `memo index` writes"""
    import pyarrow as pa
    import pyarrow.parquet as pq
    t = pq.read_table(path)
    assert t.schema.names == ["f0", "f1", "f2", "f3"] and t.schema.types == [pa.utf8(), pa.int64(), pa.int64(), pa.int64()]
    md = pq.ParquetFile(path).metadata
    for g in range(md.num_row_groups):
        assert md.row_group(g).column(0).compression == "ZSTD" and md.row_group(g).column(1).statistics.has_min_max
    return (t.column("f0").to_pylist(), *(t.column(c).to_numpy() for c in ("f1", "f2", "f3")))


def _same_table(path, want, note):
    got = _table(path)
    assert got[0] == list(want[0]), note
    same_rows(tuple(np.asarray(c, np.int64) for c in got[1:]), want[1:], note)


def _memo(*argv, env=None):
    return subprocess.run([sys.executable, EXE, *argv], capture_output=True, timeout=300, env=dict(os.environ, **(env or {})))


# ---------------------------------------------------------------------------------------
# memo_ms_rows_dev
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ("dense", "coded"))
def test_ms_rows_on_the_device_equal_the_fetched_rows(memo, dev, pan, layout):
    from memo_amd.build_index import MatchingStatistics, pivot_layout
    _names, pivot, rec_begin = pivot_layout(pan.pivot)
    npos = int(rec_begin[-1])
    with MatchingStatistics(pivot, rec_begin, len(pan.new), 0, 0, layout) as ms:
        assert ms.layout_info()["layout"] == layout
        for j, g in enumerate(pan.new):
            ms.add_records(g, j)
        whole = ms.fetch()
        assert np.array_equal(whole, np.vstack([add_oracle.new_ms(seq, pan.new) for _, seq in pan.pivot]))
        for first, positions in ((0, 0), (0, 1), (0, 129), (0, npos), (1, 300), (700, 0), (700, 1), (650, 513), (npos - 1, 1), (npos, 0), (npos - 257, 257)):
            d_rows = C.c_void_p(0xDEAD0)
            dev.check(dev.lib.memo_ms_rows_dev(ms._h, first, positions, C.byref(d_rows)))
            if not positions:
                assert d_rows.value is None, (first, positions)
                continue
            assert d_rows.value and d_rows.value % 4 == 0
            got = dev.get(d_rows.value, positions * ms.columns, np.int32).reshape(positions, ms.columns)
            assert np.array_equal(got, ms.fetch(first, positions)) and np.array_equal(got, whole[first:first + positions]), (first, positions)
        for first, positions in ((-1, 1), (0, npos + 1), (npos, 1), (npos + 1, 0), (5, -1)):
            d_rows = C.c_void_p(0xDEAD0)
            assert dev.lib.memo_ms_rows_dev(ms._h, first, positions, C.byref(d_rows)) == EINVAL and d_rows.value == 0xDEAD0, (first, positions)
            assert b"outside the pivot" in dev.lib.memo_last_error()
        assert dev.lib.memo_ms_rows_dev(ms._h, 0, 1, None) == EINVAL and dev.lib.memo_ms_rows_dev(None, 0, 1, C.byref(d_rows)) == EINVAL


# ---------------------------------------------------------------------------------------
# rows and whole indexes against the definition
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("settings", (dict(), dict(MEMO_ADD_SLICE="7", MEMO_ADD_BATCH="5"), dict(MEMO_ADD_SLICE="64", MEMO_ADD_BATCH="5"),
                                      dict(MEMO_ADD_SLICE="2049", MEMO_ADD_BATCH="5"), dict(MEMO_ADD_SLICE="7", MEMO_ADD_BATCH="1000"),
                                      dict(MEMO_ADD_SLICE="64", MEMO_ADD_BATCH="1000"), dict(MEMO_ADD_SLICE="2049", MEMO_ADD_BATCH="1000")),
                         ids=lambda s: "-".join(s.values()) or "default")
def test_the_grown_index_equals_the_definition_at_every_slice_and_batch_length(memo, pan, tmp_path, monkeypatch, settings):
    from memo_amd import add
    for name, value in settings.items():
        monkeypatch.setenv(name, value)
    index, plus, _full = pan.files
    memb, cons = str(tmp_path / "memb.parquet"), str(tmp_path / "cons.parquet")
    got = add.add_index(index, plus, pan.n, out_path=memb, cons_path=cons, log=lambda line: None)
    assert sorted(os.listdir(tmp_path)) == ["cons.parquet", "memb.parquet"]
    assert got == {"positions": 1801, "new": 3, "rows": [len(pan.want[False][1]), len(pan.want[True][1])]}
    _same_table(memb, pan.want[False], (settings, "-o"))
    _same_table(cons, pan.want[True], (settings, "-c"))


@pytest.mark.parametrize("order", (False, True))
def test_one_record_at_a_slice_and_a_batch_of_one_position(memo, pan, order):
    from memo_amd import add
    name, seq = pan.pivot[1]
    assert len(seq) == 300
    want = add_oracle.rows(*pan.index[name], pan.n, seq, pan.new, order)
    shuffle = np.random.default_rng(3).permutation(len(pan.index[name][0]))
    for kw in (dict(slice_positions=1, batch_positions=1), dict(), dict(slice_positions=129, batch_positions=7)):
        same_rows(add.rows(*pan.index[name], pan.n, seq, pan.new, order=order, **kw), want, (order, kw))
        same_rows(add.rows(*(c[shuffle] for c in pan.index[name]), pan.n, seq, pan.new, order=order, **kw), want, (order, kw, "shuffled"))


@pytest.mark.parametrize("layout", ("dense", "coded"))
def test_cli_under_either_layout_of_the_matching_statistics(memo, pan, tmp_path, layout):
    index, plus, _full = pan.files
    memb, cons = str(tmp_path / "memb.parquet"), str(tmp_path / "cons.parquet")
    r = _memo("add", "-b", index, "-n", str(pan.n), "-g", plus, "-o", memb, "-c", cons,
              env={"MEMO_INDEX_DAP_LAYOUT": layout, "MEMO_ADD_SLICE": "500", "MEMO_ADD_BATCH": "130", "MEMO_INDEX_PIECE_BYTES": "1600", "MEMO_INDEX_WALK_BUDGET": "3"})
    assert (r.returncode, r.stdout) == (0, b"MEMO - add\n"), r.stderr
    _same_table(memb, pan.want[False], (layout, "-o"))
    _same_table(cons, pan.want[True], (layout, "-c"))


def test_the_files_are_what_memo_index_writes_on_the_full_list(memo, complete_pan, tmp_path):
    """where every pivot character occurs in every old genome"""
    pan = complete_pan
    assert pan.complete
    _index, _plus, full = pan.files
    for flags, prefix, order in ((("-m",), "memb", False), ((), "cons", True)):
        r = _memo("index", "-g", full, "-o", str(tmp_path), "-p", prefix, *flags)
        assert r.returncode == 0, r.stderr
        _same_table(str(tmp_path / (prefix + ".parquet")), pan.want[order], prefix)


# ---------------------------------------------------------------------------------------
# the command line on the example
# ---------------------------------------------------------------------------------------
def _list(path, fasta):
    open(path, "w").write("".join(p + "\n" for p in fasta))
    return str(path)


def _golden_table(name):
    f0, s, e, a = _table(os.path.join(G.GOLD, name))
    return f0, s, e, a


def test_cli_grows_the_example_to_both_committed_indexes_and_the_results_are_queried(memo, tmp_path):
    work = tmp_path / "work"
    r = _memo("index", "-g", _list(tmp_path / "four.txt", FASTA[:4]), "-o", str(work), "-p", "four", "-m")
    assert r.returncode == 0, r.stderr
    assert len(_table(str(work / "four.parquet"))[1]) == 34
    memb, cons = str(tmp_path / "memb5.parquet"), str(tmp_path / "cons5.parquet")
    plus = _list(tmp_path / "plus.txt", [FASTA[0], FASTA[4]])
    r = _memo("add", "-b", str(work / "four.parquet"), "-n", "4", "-g", plus, "-o", memb, "-c", cons)
    assert (r.returncode, r.stdout) == (0, b"MEMO - add\n"), r.stderr
    assert sorted(os.listdir(tmp_path)) == ["cons5.parquet", "four.txt", "memb5.parquet", "plus.txt", "work"]      # written beside their names and renamed
    _same_table(memb, _golden_table("example_memb.parquet"), "memb5")
    _same_table(cons, _golden_table("example_cons.parquet"), "cons5")
    assert len(_table(memb)[1]) == 48 and len(_table(cons)[1]) == 56
    for index, name, flags in ((memb, "ex_memb_k3_0_20", ("-m",)), (cons, "ex_cons_k3_0_20", ())):
        case = next(c for c in G.cases(raises=False) if c["name"] == name)
        assert case["k"] == 3
        text = str(tmp_path / (name + ".txt"))
        r = _memo("query", "-b", index, "-r", case["region"], "-k", "3", "-n", str(case["n"]), "-o", text, *flags)
        assert r.returncode == 0 and open(text, "rb").read() == G.out_bytes(case), r.stderr
    # either output alone
    alone = str(tmp_path / "alone.parquet")
    r = _memo("add", "-b", str(work / "four.parquet"), "-n", "4", "-g", plus, "-o", alone)
    assert (r.returncode, r.stdout) == (0, b"MEMO - add\n"), r.stderr
    _same_table(alone, _golden_table("example_memb.parquet"), "-o alone")
    r = _memo("add", "-b", str(work / "four.parquet"), "-n", "4", "-g", plus, "-c", alone, env={"MEMO_ADD_SLICE": "7", "MEMO_ADD_BATCH": "3"})
    assert (r.returncode, r.stdout) == (0, b"MEMO - add\n"), r.stderr
    _same_table(alone, _golden_table("example_cons.parquet"), "-c alone")
    assert sorted(os.listdir(tmp_path)) == ["alone.parquet", "cons5.parquet", "ex_cons_k3_0_20.txt", "ex_memb_k3_0_20.txt", "four.txt", "memb5.parquet",
                                            "plus.txt", "work"]


def test_cli_chain_of_two_three_five_genomes(memo, tmp_path):
    r = _memo("index", "-g", _list(tmp_path / "two.txt", FASTA[:2]), "-o", str(tmp_path), "-p", "two", "-m")
    assert r.returncode == 0, r.stderr
    three, memb, cons = (str(tmp_path / name) for name in ("three.parquet", "memb5.parquet", "cons5.parquet"))
    r = _memo("add", "-b", str(tmp_path / "two.parquet"), "-n", "2", "-g", _list(tmp_path / "third.txt", [FASTA[0], FASTA[2]]), "-o", three)
    assert r.returncode == 0, r.stderr
    r = _memo("add", "-b", three, "-n", "3", "-g", _list(tmp_path / "rest.txt", [FASTA[0], FASTA[3], FASTA[4]]), "-o", memb, "-c", cons)
    assert r.returncode == 0, r.stderr
    _same_table(memb, _golden_table("example_memb.parquet"), "2 -> 3 -> 5, -o")
    _same_table(cons, _golden_table("example_cons.parquet"), "2 -> 3 -> 5, -c")


def test_cli_refuses_and_leaves_no_file_behind(memo, tmp_path):
    memb = os.path.join(G.GOLD, "example_memb.parquet")
    out, cons = str(tmp_path / "never.parquet"), str(tmp_path / "never_cons.parquet")
    plus = _list(tmp_path / "plus.txt", [FASTA[0], FASTA[4]])
    other = tmp_path / "other.fa"
    other.write_bytes(b">ref_1\nACGACTCGACGACTCACGACACTGC\n")
    short = _list(tmp_path / "short.txt", [str(other), FASTA[4]])
    before = sorted(os.listdir(tmp_path))
    for argv, env, message in ((("-b", memb, "-n", "4", "-g", plus), None, b"has annot 4 outside [1, 3]"),
                               (("-b", os.path.join(G.GOLD, "rnd_negoverlap.parquet"), "-n", "12", "-g", plus), None, b"ends before it starts"),
                               (("-b", memb, "-n", "5", "-g", short), None, b"has 25 positions"),
                               (("-b", memb, "-n", "5", "-g", plus), {"WORLD_SIZE": "2"}, b"sharded launch"),
                               # refused by the device call, after the host had nothing to refuse: a cap no genome record fits under
                               (("-b", memb, "-n", "5", "-g", plus), {"MEMO_INDEX_PIECE_BYTES": "5"}, b"ref_5.fa: record 'ref_5'")):
        r = _memo("add", *argv, "-o", out, "-c", cons, env=env)
        assert r.returncode == 1 and r.stdout == b"MEMO - add\n" and r.stderr.startswith(b"memo add: ") and message in r.stderr, (argv, r.stderr)
        assert sorted(os.listdir(tmp_path)) == before, argv
