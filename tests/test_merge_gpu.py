"""`memo merge` on the GPU: merge_dap_kernel alone through the C ABI and through memo_amd.merge.dap against NumPy and against
convert_dap_kernel, memo_amd.merge.rows / merge_index against the definition (tests/merge_oracle.py) on a seeded pangenome indexed in two
groups by `bin/memo index -m`, at every slice and batch length, and the command line on the committed example.

Three references that do not share code: the definition (NumPy), the canonical rows of the inputs filtered and renumbered (neither planes
nor matrix), and the files `bin/memo index` writes on the combined list.  Every comparison is exact."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import golden_util as G
from tests import merge_oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "memo")
FASTA = [os.path.join(G.GOLD, "example_fa", f"ref_{i}.fa") for i in range(1, 6)]
MEMB = os.path.join(G.GOLD, "example_memb.parquet")
PAD = 0x5A5A5A5A
EINVAL = -1
COLS = (1, 2, 63, 64, 65, 128, 129, 2047)


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
# the kernel alone
# ---------------------------------------------------------------------------------------
def cell_values(rng, count, positions, remaining):
    """uint32 [count, positions], all at least 1: values at, one under and one over remaining - i, 2^31 - 1, and anything a uint32 holds"""
    room = remaining - np.arange(positions, dtype=np.int64)[None, :]
    kind = rng.integers(0, 6, (count, positions))
    v = room + (kind - 1)                                          # kinds 0, 1, 2: one under, at, one over
    v = np.where(kind == 3, 2 ** 31 - 1, v)
    v = np.where(kind == 4, rng.integers(1, 2 ** 32, (count, positions)), v)
    v = np.where(kind == 5, rng.integers(1, 300, (count, positions)), v)
    return np.clip(v, 1, 2 ** 32 - 1).astype(np.uint32)


def column_maps(rng, cols, planes):
    """{name: int64 [cols]} over `planes` = 2 cols + 1 planes.  Plane 0 holds zeros and no map names it."""
    assert planes == 2 * cols + 1
    identity = np.arange(1, cols + 1, dtype=np.int64)
    maps = {"identity": identity, "reversed": identity[::-1].copy(), "permutation": rng.permutation(identity),
            "strided": np.arange(1, 2 * cols, 2, dtype=np.int64), "upper": identity + cols}
    twice = rng.permutation(np.arange(1, planes, dtype=np.int64))[:cols]
    if cols >= 2:
        twice[cols // 2] = twice[0]
        if cols >= 66:
            twice[65] = twice[0]                                   # the same plane from two tiles of columns
    maps["twice"] = twice
    for name, entries in (("outside", (-1, planes)), ("far outside", (-2 ** 31, 2 ** 31 - 1))):
        bad = rng.permutation(np.arange(1, planes, dtype=np.int64))[:cols]
        if cols == 1:
            maps[name + " below"], maps[name + " above"] = np.asarray([entries[0]]), np.asarray([entries[1]])
            continue
        bad[cols // 2], bad[-1] = entries                          # their neighbours stay
        maps[name] = bad
    return maps


def expected(cells, entries, first, positions, remaining):
    """int64 [positions, cols] of the definition: an entry outside the planes is a column of zeros"""
    inside = (entries >= 0) & (entries < len(cells))
    taken = cells[np.where(inside, entries, 0), first:first + positions].T.astype(np.int64)
    want = np.minimum(taken, remaining - np.arange(positions, dtype=np.int64)[:, None])
    want[:, ~inside] = 0
    return want, inside


@pytest.mark.parametrize("cols", COLS)
def test_the_kernel_against_numpy(memo, dev, cols):
    """Plane 0, the cells left and right of [first, first + positions) and the pad up to the pitch are 0, every value inside is at
    least 1 and so is remaining - i: a value read from outside would show as a 0.  The output lies between words of PAD that must stay.
    One layout of the cells serves every map.  At 2047 columns the corners of the grid of lengths run, not all of it: the tile's paths
    are the same as at 129 columns, where all of it runs."""
    from memo_amd import merge
    T = merge.tile()
    assert T == 128
    planes = 2 * cols + 1
    rng = np.random.default_rng(77000 + cols)
    maps = column_maps(rng, cols, planes)
    longest = 2 * T + 1
    pitch = ((3 + longest + 3) & ~3) + 64
    d_cells, d_map, d_out = dev.alloc(4 * planes * pitch), dev.alloc(4 * (cols + 8)), dev.alloc(4 * (longest * cols + 8))
    whole = cols < 2047
    calls = 0
    for positions in (0, 1, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1) if whole else (0, 1, T, 2 * T + 1):
        for first in (0, 1, 3, pitch - positions) if whole else (3, pitch - positions):       # the last one ends exactly at the pitch
            for remaining in (positions, positions + 1000, 2 ** 31 - 1):
                cells = np.zeros((planes, pitch), np.uint32)
                cells[1:, first:first + positions] = cell_values(rng, planes - 1, positions, remaining)
                dev.upload(d_cells, cells)
                for name, entries in maps.items():
                    dev.upload(d_map, np.concatenate([[0] * 4, entries, [0] * 4]).astype(np.int32))
                    dev.upload(d_out, np.full(longest * cols + 8, PAD, np.uint32))
                    dev.check(dev.lib.memo_merge_dap_dev(d_cells, pitch, planes, d_map + 16, cols, first, positions, remaining, d_out + 16, 0, None))
                    got = dev.get(d_out, longest * cols + 8, np.uint32)
                    note = (name, positions, first, remaining)
                    assert (got[:4] == PAD).all() and (got[4 + positions * cols:] == PAD).all(), note
                    want, inside = expected(cells, entries, first, positions, remaining)
                    assert want.shape == (positions, cols) and (want.size == 0 or want[:, inside].min(initial=1) >= 1), note
                    got = got[4:4 + positions * cols].view(np.int32).reshape(positions, cols)
                    if not np.array_equal(got, want):
                        i, c = np.argwhere(got != want)[0]
                        raise AssertionError(f"{note}: {(got != want).sum()} of {want.size} differ, first at row {i}, column {c} "
                                             f"(plane {entries[c]}): got {got[i, c]}, want {want[i, c]}")
                    calls += 1
    assert calls == (96 if whole else 24) * len(maps) and len(maps) >= 8


@pytest.mark.parametrize("cols", COLS)
def test_the_identity_map_is_memo_convert(memo, cols):
    """planes = cols + 1: the map 1 .. cols gives what convert_dap_kernel gives on the same planes, through both modules"""
    from memo_amd import convert, merge
    rng = np.random.default_rng(500 + cols)
    planes = rng.integers(0, 2 ** 32, (cols + 1, 391), dtype=np.uint64).astype(np.uint32)
    for first, positions, remaining in ((0, 391, 391), (2, 300, 2 ** 31 - 1), (130, 257, 300), (5, 0, 0)):
        got = merge.dap(planes, np.arange(1, cols + 1), first, positions, remaining)
        assert got.dtype == np.int32 and got.shape == (positions, cols)
        assert np.array_equal(got, convert.dap(planes, first, positions, remaining)), (first, positions, remaining)
        want = np.minimum(planes[1:, first:first + positions].T.astype(np.int64), remaining - np.arange(positions)[:, None])
        assert np.array_equal(got, want)
    # the pivot's plane is a plane like any other here, and a larger pitch changes nothing
    got = merge.dap(planes, [0, cols, 0], 1, 390, 1000, pitch=400)
    assert np.array_equal(got, np.minimum(planes[[0, cols, 0], 1:].T.astype(np.int64), 1000 - np.arange(390)[:, None]))


def test_the_kernel_refuses_before_it_launches(memo, dev):
    planes, cols, pitch, positions = 6, 4, 64, 40
    cells = np.full((planes, pitch), 7, np.uint32)
    d_cells, d_map, d_out = dev.alloc(cells.nbytes + 16), dev.alloc(4 * (cols + 8)), dev.alloc(4 * (positions * cols + 8))
    dev.upload(d_cells, cells)
    dev.upload(d_map, np.asarray([0] * 4 + [5, 1, 6, 1] + [0] * 4, np.int32))
    poison = np.full(positions * cols + 8, PAD, np.uint32)
    dev.upload(d_out, poison)
    ok = dict(d_cells=d_cells, pitch=pitch, planes=planes, d_map=d_map + 16, cols=cols, first=3, positions=positions, remaining=50, d_out=d_out + 16)

    def call(a):
        return dev.lib.memo_merge_dap_dev(a["d_cells"], a["pitch"], a["planes"], a["d_map"], a["cols"], a["first"], a["positions"], a["remaining"],
                                          a["d_out"], 0, None)
    for change, message in ((dict(planes=0), b"planes must be"), (dict(planes=-1), b"planes must be"), (dict(planes=65537), b"planes must be"),
                            (dict(cols=0), b"cols must be"), (dict(cols=2048), b"cols must be"), (dict(cols=-1), b"cols must be"),
                            (dict(pitch=62), b"multiple of 4"), (dict(pitch=66), b"multiple of 4"),
                            (dict(first=25), b"do not lie inside"), (dict(first=pitch + 1, positions=0), b"do not lie inside"),
                            (dict(positions=62), b"do not lie inside"), (dict(remaining=39), b"remaining"), (dict(remaining=2 ** 31), b"2^31 - 1"),
                            (dict(d_cells=d_cells + 4), b"16-byte aligned"), (dict(d_cells=d_cells + 8), b"16-byte aligned"),
                            (dict(d_map=d_map + 18), b"d_plane_of must be 4-byte aligned"), (dict(d_map=d_map + 17), b"d_plane_of must be 4-byte aligned"),
                            (dict(d_out=d_out + 18), b"d_dap must be 4-byte aligned"), (dict(d_out=d_out + 17), b"d_dap must be 4-byte aligned"),
                            (dict(first=-1), b"negative"), (dict(positions=-1), b"negative"), (dict(pitch=-4), b"negative"),
                            (dict(remaining=-1, positions=0), b"negative"), (dict(d_out=0), b"NULL"), (dict(d_cells=0), b"NULL"), (dict(d_map=0), b"NULL")):
        rc = call(dict(ok, **change))
        assert rc == EINVAL and message in dev.lib.memo_last_error(), (change, dev.lib.memo_last_error())
        assert np.array_equal(dev.get(d_out, len(poison), np.uint32), poison), change
    # nothing to do launches nothing, whatever the pointers are
    assert call(dict(ok, d_cells=0, d_map=0, d_out=0, positions=0, remaining=0)) == 0
    assert np.array_equal(dev.get(d_out, len(poison), np.uint32), poison)
    dev.check(call(ok))
    got = dev.get(d_out, len(poison), np.uint32)
    assert (got[:4] == PAD).all() and (got[-4:] == PAD).all()
    room = np.minimum(7, 50 - np.arange(positions))[:, None]
    assert np.array_equal(got[4:-4].reshape(positions, cols), np.hstack([room, room, 0 * room, room]))          # entry 6 names no plane
    # the widest stack and the widest matrix the ABI takes are taken
    assert call(dict(ok, planes=65536, positions=0)) == 0 and call(dict(ok, cols=2047, positions=0)) == 0 and call(dict(ok, planes=1, positions=0)) == 0


# ---------------------------------------------------------------------------------------
# the seeded pangenome, indexed in two groups
# ---------------------------------------------------------------------------------------
def _mutated(rng, seq, rate, alphabet=b"ACGT"):
    out = bytearray(seq)
    for i in np.flatnonzero(rng.random(len(out)) < rate):
        out[i] = alphabet[int(rng.integers(len(alphabet)))]
    return bytes(out)


def _memo(*argv, env=None):
    return subprocess.run([sys.executable, EXE, *argv], capture_output=True, timeout=300, env=dict(os.environ, **(env or {})))


def _table(path):
    """(f0 as a list, f1, f2, f3) of a Parquet index, after the check that it has the schema `memo index` writes"""
    import pyarrow as pa
    import pyarrow.parquet as pq
    t = pq.read_table(path)
    assert t.schema.names == ["f0", "f1", "f2", "f3"] and t.schema.types == [pa.utf8(), pa.int64(), pa.int64(), pa.int64()]
    md = pq.ParquetFile(path).metadata
    for g in range(md.num_row_groups):
        assert md.row_group(g).column(0).compression == "ZSTD" and md.row_group(g).column(1).statistics.has_min_max
    return (t.column("f0").to_pylist(), *(np.ascontiguousarray(t.column(c).to_numpy(), np.int64) for c in ("f1", "f2", "f3")))


def _same_table(path, want, note):
    got = _table(path)
    assert got[0] == list(want[0]), note
    same_rows(tuple(got[1:]), tuple(want[1:]), note)


def _list(path, fasta):
    open(path, "w").write("".join(p + "\n" for p in fasta))
    return str(path)


def _fasta(path, records):
    with open(path, "wb") as fh:
        for rec, seq in records:
            fh.write(b">" + rec.encode() + b" described\n" + b"\n".join(seq[i:i + 70] for i in range(0, len(seq), 70)) + b"\n")
    return str(path)


class Pangenome:
    """A pivot of three records of 1, 300 and 1500 positions and six genomes: mutated copies (one with its records in the other order),
    a verbatim copy of the longest record, one that shares nothing with the pivot but single letters (runs of A, C, G and T: every
    pivot character occurs in it, so its index says what its matching statistics are), and a mutated copy with a run of N.  With
    `lacking`, the last mutated copy is made of C and G alone instead: neither A nor T occurs in it or in its reverse complement, the
    matching statistic is 0 there, the index holds no row for it, and the column is what the index answers with.
    Group A is genomes 1, 2, 3 of the combined list, group B genomes 4, 5, 6, each indexed with the pivot by `bin/memo index -m`."""

    def __init__(self, lacking, where):
        rng = np.random.default_rng(40 + lacking)
        letters = np.frombuffer(b"ACGT", np.uint8)
        self.pivot = [(name, letters[rng.integers(0, 4, length)].tobytes()) for name, length in (("one", 1), ("mid", 300), ("long", 1500))]
        seqs = [s for _, s in self.pivot]
        run = bytearray(_mutated(rng, seqs[2], 0.03))
        run[400:600] = b"N" * 200
        last = [s.replace(b"A", b"C").replace(b"T", b"G") for s in seqs] if lacking else [_mutated(rng, s, 0.3) for s in seqs[::-1]]
        self.genomes = [[_mutated(rng, s, 0.02) for s in seqs], [seqs[2]], [b"A" * 40 + b"C" * 40 + b"G" * 40 + b"T" * 40],
                        [_mutated(rng, s, 0.1) for s in seqs], [_mutated(rng, seqs[1], 0.05), bytes(run)], last]
        self.complete = not lacking
        self.lengths = {name: len(s) for name, s in self.pivot}
        pivot = _fasta(where / "pivot.fa", self.pivot)
        files = [_fasta(where / f"g{i + 1}.fa", [(f"c{j}", s) for j, s in enumerate(g)]) for i, g in enumerate(self.genomes)]
        self.lists = [_list(where / "a.txt", [pivot] + files[:3]), _list(where / "b.txt", [pivot] + files[3:])]
        self.full = _list(where / "full.txt", [pivot] + files)
        self.where = where
        self.index, self.rows, self.canonical = [], [], []
        from memo_amd import convert
        for prefix, listed in zip("ab", self.lists):
            r = _memo("index", "-g", listed, "-o", str(where), "-p", prefix, "-m")
            assert r.returncode == 0, r.stderr
            path = str(where / (prefix + ".parquet"))
            self.index.append(path)
            self.rows.append(merge_oracle.by_record(*_table(path)))
            assert list(self.rows[-1]) == ["one", "mid", "long"]
            assert {name: int(c[0].max()) for name, c in self.rows[-1].items()} == self.lengths
            canon = str(where / (prefix + "_canonical.parquet"))          # its `memo convert -m` form
            convert.convert_index(path, canon, 4, order=False, log=lambda line: None)
            self.canonical.append(merge_oracle.by_record(*_table(canon)))
        self._want = {}

    def want(self, selections, order):
        """(names, s, e, a) of the definition for the inputs [(group, selection), ...]"""
        key = (tuple((g, None if sel is None else tuple(sel)) for g, sel in selections), order)
        if key not in self._want:
            self._want[key] = merge_oracle.index_rows([(self.rows[g], 4, sel) for g, sel in selections], order)
        return self._want[key]

    def renumbered(self, selections):
        """the same -o rows from the canonical forms alone"""
        names, parts = [], []
        for name in self.lengths:
            part = merge_oracle.renumbered([(self.canonical[g][name], 4, sel) for g, sel in selections])
            names += [name] * len(part[0])
            parts.append(part)
        return (names, *(np.concatenate([p[i] for p in parts]) for i in range(3)))


_PANGENOMES = {}


def _pangenome(lacking, factory):
    """built once a module, files and all"""
    if lacking not in _PANGENOMES:
        _PANGENOMES[lacking] = Pangenome(lacking, factory.mktemp("pan"))
    return _PANGENOMES[lacking]


@pytest.fixture(scope="module", params=(1, 0), ids=("lacking", "complete"))
def pan(request, memo, tmp_path_factory):
    return _pangenome(request.param, tmp_path_factory)


@pytest.fixture(scope="module")
def complete_pan(memo, tmp_path_factory):
    return _pangenome(0, tmp_path_factory)


BOTH = ((0, None), (1, None))


def _merged(pan, tmp_path, selections, note):
    """merge_index of the groups and selections into both outputs, held against the definition and against the renumbered rows"""
    from memo_amd import merge
    memb, cons = str(tmp_path / "memb.parquet"), str(tmp_path / "cons.parquet")
    got = merge.merge_index([(pan.index[g], 4, sel) for g, sel in selections], out_path=memb, cons_path=cons, log=lambda line: None)
    assert sorted(os.listdir(tmp_path)) == ["cons.parquet", "memb.parquet"]
    want = {order: pan.want(selections, order) for order in (False, True)}
    width = sum(3 if sel is None else len(sel) for _, sel in selections)
    assert got == {"positions": 1801, "genomes": width + 1, "rows": [len(want[False][1]), len(want[True][1])]}, note
    _same_table(memb, want[False], (note, "-o"))
    _same_table(cons, want[True], (note, "-c"))
    _same_table(memb, pan.renumbered(selections), (note, "-o, renumbered"))
    os.unlink(memb), os.unlink(cons)


@pytest.mark.parametrize("settings", (dict(), dict(MEMO_MERGE_SLICE="7", MEMO_MERGE_BATCH="5"), dict(MEMO_MERGE_SLICE="64", MEMO_MERGE_BATCH="5"),
                                      dict(MEMO_MERGE_SLICE="2049", MEMO_MERGE_BATCH="5"), dict(MEMO_MERGE_SLICE="7", MEMO_MERGE_BATCH="1000"),
                                      dict(MEMO_MERGE_SLICE="64", MEMO_MERGE_BATCH="1000"), dict(MEMO_MERGE_SLICE="2049", MEMO_MERGE_BATCH="1000")),
                         ids=lambda s: "-".join(s.values()) or "default")
def test_two_indexes_merged_equal_the_definition_at_every_slice_and_batch_length(memo, pan, tmp_path, monkeypatch, settings):
    for name, value in settings.items():
        monkeypatch.setenv(name, value)
    _merged(pan, tmp_path, BOTH, settings)


@pytest.mark.parametrize("settings", (dict(), dict(MEMO_MERGE_SLICE="130", MEMO_MERGE_BATCH="129")), ids=lambda s: "-".join(s.values()) or "default")
def test_chosen_genomes_of_one_and_of_two_indexes(memo, pan, tmp_path, monkeypatch, settings):
    for name, value in settings.items():
        monkeypatch.setenv(name, value)
    for selections in (((0, [3, 1]),), ((1, [2]),), ((1, [3, 2, 1]),), ((1, [3]), (0, [2, 3])), ((0, [2]), (1, [3, 1]))):
        _merged(pan, tmp_path, selections, (settings, selections))


@pytest.mark.parametrize("order", (False, True))
def test_one_record_at_a_slice_and_a_batch_of_one_position(memo, pan, order):
    from memo_amd import merge
    name = "mid"
    assert pan.lengths[name] == 300
    for selections in (BOTH, ((1, [3, 1]), (0, [2]))):
        sources = [(*pan.rows[g][name], 4, sel) for g, sel in selections]
        want = merge_oracle.rows(sources, 300, order)
        shuffle = [np.random.default_rng(3 + g).permutation(len(pan.rows[g][name][0])) for g, _ in selections]
        shuffled = [(*(c[at] for c in src[:3]), *src[3:]) for src, at in zip(sources, shuffle)]
        for kw in (dict(slice_positions=1, batch_positions=1), dict(), dict(slice_positions=129, batch_positions=7)):
            same_rows(merge.rows(sources, order=order, **kw), want, (order, selections, kw))
            same_rows(merge.rows(shuffled, 300, order=order, **kw), want, (order, selections, kw, "shuffled"))
    # a selection as the command writes it, and a record longer than its largest row start
    same_rows(merge.rows([(*pan.rows[0][name], 4, "3,1-2")], order=order), merge_oracle.rows([(*pan.rows[0][name], 4, [3, 1, 2])], 300, order), "a string")
    sources = [(*pan.rows[g][name], 4, None) for g in (0, 1)]
    same_rows(merge.rows(sources, 310, order=order, slice_positions=64), merge_oracle.rows(sources, 310, order), "length 310")


def test_the_files_are_what_memo_index_writes_on_the_combined_list(memo, complete_pan, tmp_path):
    """where every pivot character occurs in every genome: the third reference, from the genomes themselves"""
    from memo_amd import merge
    pan = complete_pan
    assert pan.complete
    memb, cons = str(tmp_path / "memb.parquet"), str(tmp_path / "cons.parquet")
    merge.merge_index([(path, 4, None) for path in pan.index], out_path=memb, cons_path=cons, log=lambda line: None)
    for flags, prefix, path in ((("-m",), "full_memb", memb), ((), "full_cons", cons)):
        r = _memo("index", "-g", pan.full, "-o", str(tmp_path), "-p", prefix, *flags)
        assert r.returncode == 0, r.stderr
        _same_table(path, _table(str(tmp_path / (prefix + ".parquet"))), prefix)


# ---------------------------------------------------------------------------------------
# the command line on the example
# ---------------------------------------------------------------------------------------
def test_cli_selections_of_the_example(memo, tmp_path):
    s, e, a = G.index_columns("example_memb.parquet", "ref_1")
    for text, chosen, members, conserved in (("1-3", [1, 2, 3], 34, 38), ("3,1", [3, 1], 26, 27), ("2", [2], 8, 8), ("4,3,2,1", [4, 3, 2, 1], 48, 56)):
        memb, cons = str(tmp_path / "memb.parquet"), str(tmp_path / "cons.parquet")
        r = _memo("merge", "-b", MEMB, "-n", "5", "-s", text, "-o", memb, "-c", cons)
        assert (r.returncode, r.stdout) == (0, b"MEMO - merge\n"), r.stderr
        assert sorted(os.listdir(tmp_path)) == ["cons.parquet", "memb.parquet"]                     # written beside their names and renamed
        for path, order, count in ((memb, False, members), (cons, True, conserved)):
            want = merge_oracle.rows([(s, e, a, 5, chosen)], 26, order)
            assert len(want[0]) == count
            _same_table(path, (["ref_1"] * count, *want), (text, order))
        _same_table(memb, (["ref_1"] * members, *merge_oracle.renumbered([((s, e, a), 5, chosen)])), (text, "renumbered"))
    # conservation does not depend on the order of the genomes
    _same_table(cons, _table(os.path.join(G.GOLD, "example_cons.parquet")), "-s 4,3,2,1 -c")


def test_cli_reversed_twice_is_the_index_and_either_output_alone(memo, tmp_path):
    back, again, cons, fai = (str(tmp_path / name) for name in ("back.parquet", "again.parquet", "cons.parquet", "ref_1.fa.fai"))
    open(fai, "w").write("ref_1\t26\t7\t26\t27\n")
    r = _memo("merge", "-b", MEMB, "-n", "5", "-s", "4,3,2,1", "-o", back, env={"MEMO_MERGE_SLICE": "7", "MEMO_MERGE_BATCH": "3"})
    assert (r.returncode, r.stdout) == (0, b"MEMO - merge\n"), r.stderr
    assert _table(back)[3].tolist() != _table(MEMB)[3].tolist()
    r = _memo("merge", "-b", back, "-n", "5", "-s", "4,3,2,1", "-o", again)
    assert (r.returncode, r.stdout) == (0, b"MEMO - merge\n"), r.stderr
    _same_table(again, _table(MEMB), "reversed twice")
    r = _memo("merge", "-b", back, "-n", "5", "-c", cons, "-f", fai)
    assert (r.returncode, r.stdout) == (0, b"MEMO - merge\n"), r.stderr
    _same_table(cons, _table(os.path.join(G.GOLD, "example_cons.parquet")), "-c alone")
    assert sorted(os.listdir(tmp_path)) == ["again.parquet", "back.parquet", "cons.parquet", "ref_1.fa.fai"]


def test_cli_the_example_split_and_merged_is_both_committed_indexes_and_they_are_queried(memo, tmp_path):
    work = tmp_path / "work"
    lists = [_list(tmp_path / "a.txt", [FASTA[0], FASTA[1], FASTA[2]]), _list(tmp_path / "b.txt", [FASTA[0], FASTA[3], FASTA[4]])]
    for prefix, listed in zip("ab", lists):
        r = _memo("index", "-g", listed, "-o", str(work), "-p", prefix, "-m")
        assert r.returncode == 0, r.stderr
        assert int(_table(str(work / (prefix + ".parquet")))[1].max()) == 26                       # every sub-index closes the record at start 26
    memb, cons, listed = (str(tmp_path / name) for name in ("memb5.parquet", "cons5.parquet", "five.txt"))
    r = _memo("merge", "-b", str(work / "a.parquet"), "-n", "3", "-g", lists[0], "-b", str(work / "b.parquet"), "-n", "3", "-g", lists[1],
              "-o", memb, "-c", cons, "-G", listed)
    assert (r.returncode, r.stdout) == (0, b"MEMO - merge\n"), r.stderr
    assert sorted(os.listdir(tmp_path)) == ["a.txt", "b.txt", "cons5.parquet", "five.txt", "memb5.parquet", "work"]
    _same_table(memb, _table(MEMB), "memb5")
    _same_table(cons, _table(os.path.join(G.GOLD, "example_cons.parquet")), "cons5")
    assert len(_table(memb)[1]) == 48 and len(_table(cons)[1]) == 56
    assert open(listed).read() == "".join(p + "\n" for p in FASTA)
    for index, name, flags in ((memb, "ex_memb_k3_0_20", ("-m",)), (cons, "ex_cons_k3_0_20", ())):
        case = next(c for c in G.cases(raises=False) if c["name"] == name)
        assert case["k"] == 3
        text = str(tmp_path / (name + ".txt"))
        r = _memo("query", "-b", index, "-r", case["region"], "-k", "3", "-n", str(case["n"]), "-o", text, *flags)
        assert r.returncode == 0 and open(text, "rb").read() == G.out_bytes(case), r.stderr
    # a choice on each input, and its list
    r = _memo("merge", "-b", str(work / "b.parquet"), "-n", "3", "-s", "2", "-g", lists[1], "-b", str(work / "a.parquet"), "-n", "3", "-s", "2,1", "-g", lists[0],
              "-c", cons, "-G", listed)
    assert (r.returncode, r.stdout) == (0, b"MEMO - merge\n"), r.stderr
    s, e, a = G.index_columns("example_memb.parquet", "ref_1")
    want = merge_oracle.rows([(s, e, a, 5, [4, 2, 1])], 26, True)
    _same_table(cons, (["ref_1"] * len(want[0]), *want), "-s on each input")
    assert open(listed).read() == "".join(FASTA[i] + "\n" for i in (0, 4, 2, 1))


def test_cli_refuses_and_leaves_no_file_behind(memo, tmp_path):
    out, cons, listed = str(tmp_path / "never.parquet"), str(tmp_path / "never_cons.parquet"), str(tmp_path / "never.txt")
    five = _list(tmp_path / "five.txt", FASTA)
    before = sorted(os.listdir(tmp_path))
    for argv, env, message in ((("-b", MEMB, "-n", "4"), None, b"has annot 4 outside [1, 3]"),
                               (("-b", MEMB, "-n", "5", "-b", os.path.join(G.GOLD, "rnd_negoverlap.parquet"), "-n", "12"), None, b"ends before it starts"),
                               (("-b", MEMB, "-n", "5", "-s", "1,5"), None, b"names annot 5, outside [1, 4]"),
                               (("-b", MEMB, "-n", "5", "-b", MEMB, "-n", "5"), None, b"is given as two inputs"),
                               (("-b", MEMB, "-n", "5", "-g", five, "-b", os.path.join(G.GOLD, "example_cons.parquet"), "-n", "5", "-G", listed), None, b"-G needs"),
                               (("-b", MEMB, "-n", "5"), {"WORLD_SIZE": "2"}, b"sharded launch"),
                               # refused by the device call, after the host had nothing to refuse: no such device
                               (("-b", MEMB, "-n", "5", "-g", five, "-G", listed), {"MEMO_DEVICE": "99"}, b"device 99")):
        r = _memo("merge", *argv, "-o", out, "-c", cons, env=env)
        assert r.returncode == 1 and r.stdout == b"MEMO - merge\n" and r.stderr.startswith(b"memo merge: ") and message in r.stderr, (argv, r.stderr)
        assert sorted(os.listdir(tmp_path)) == before, argv
