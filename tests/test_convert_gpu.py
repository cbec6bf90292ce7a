"""`memo convert` on the GPU: convert_dap_kernel alone through the C ABI against NumPy, memo_amd.convert.rows against the definition
(tests/convert_oracle.py) at every slice and batch length, the promise checked with the shipped sweeps on the device, and the command
line against the committed indexes.

Every comparison is exact."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import convert_oracle
from tests import golden_util as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "memo")
PAD = 0x5A5A5A5A
EINVAL = -1
# the golden membership records whose rows all have end >= start: (index, record, N)
RECORDS = (("example_memb.parquet", "ref_1", 5), ("rnd_n4.parquet", "chrA", 4), ("rnd_n4.parquet", "chrB", 4), ("rnd_n8.parquet", "chr1", 8),
           ("rnd_n40.parquet", "chr1", 40), ("rnd_n40.parquet", "chr2", 40), ("rnd_n70_sparse.parquet", "chr1", 70),
           ("rnd_n130.parquet", "chr1", 130))
KS = (2, 3, 4, 8, 31, 32, 33, 64, 65, 101, 257)


@pytest.fixture(scope="module")
def memo():
    import memo_amd
    from memo_amd import _lib
    memo_amd.build()                     # make: a no-op when libmemo_amd.so is up to date
    assert _lib.lib().memo_device_count() > 0, "no HIP device: the product has no CPU fallback"
    return memo_amd


@pytest.fixture(scope="module")
def wanted():
    """the definition's rows of every record, in both orders, computed once: {(index, record, order): (start, end, annot)}"""
    out = {}
    for index, rec, n in RECORDS:
        s, e, a = G.index_columns(index, rec)
        for order in (True, False):
            out[(index, rec, order)] = convert_oracle.rows(s, e, a, n, order=order)
    return out


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


@pytest.mark.parametrize("cols", (1, 2, 31, 32, 33, 63, 64, 65, 100, 129, 2047))
def test_the_kernel_against_numpy(memo, dev, cols):
    """Every cell outside [first, first + positions) of planes 1 .. N - 1 -- plane 0, the cells left and right of the range, the pad up
    to the pitch -- is 0, and every cell inside is at least 1 and so is remaining - i: a value read from outside would show as a 0."""
    from memo_amd import convert
    T = convert.tile()
    assert T >= 32 and T % 4 == 0
    n = cols + 1
    rng = np.random.default_rng(cols)
    longest = 2 * T + 1
    pitch = ((3 + longest + 3) & ~3) + 64
    d_cells, d_out = dev.alloc(4 * n * pitch), dev.alloc(4 * (longest * cols + 8))
    calls = 0
    for positions in (0, 1, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1):
        for first in (0, 1, 3, pitch - positions):                 # the last one ends exactly at the pitch
            for remaining in (positions, positions + 1000, 2 ** 31 - 1):
                cells = np.zeros((n, pitch), np.uint32)
                cells[1:, first:first + positions] = cell_values(rng, cols, positions, remaining)
                dev.upload(d_cells, cells)
                dev.upload(d_out, np.full(longest * cols + 8, PAD, np.uint32))
                dev.check(dev.lib.memo_convert_dap_dev(d_cells, pitch, n, first, positions, remaining, d_out + 16, 0, None))
                got = dev.get(d_out, longest * cols + 8, np.uint32)
                assert (got[:4] == PAD).all() and (got[4 + positions * cols:] == PAD).all(), (positions, first, remaining)
                want = np.minimum(cells[1:, first:first + positions].T.astype(np.int64), remaining - np.arange(positions, dtype=np.int64)[:, None])
                assert want.size == 0 or want.min() >= 1
                got = got[4:4 + positions * cols].view(np.int32).reshape(positions, cols)
                if not np.array_equal(got, want):
                    i, c = np.argwhere(got != want)[0]
                    raise AssertionError(f"positions {positions}, first {first}, remaining {remaining}: {(got != want).sum()} of {want.size} differ, "
                                         f"first at row {i}, column {c}: got {got[i, c]}, want {want[i, c]}")
                calls += 1
    assert calls == 96


def test_the_kernel_through_the_module(memo):
    from memo_amd import convert
    rng = np.random.default_rng(5)
    planes = rng.integers(0, 2 ** 32, (7, 301), dtype=np.uint64).astype(np.uint32)
    got = convert.dap(planes, 2, 299, 400)
    assert got.dtype == np.int32 and np.array_equal(got, np.minimum(planes[1:, 2:].T.astype(np.int64), 400 - np.arange(299)[:, None]))
    assert convert.dap(planes, 5, 0, 0).shape == (0, 6)


def test_the_kernel_refuses_before_it_launches(memo, dev):
    n, pitch, positions = 5, 64, 40
    cells = np.full((n, pitch), 7, np.uint32)
    d_cells, d_out = dev.alloc(cells.nbytes + 16), dev.alloc(4 * (positions * (n - 1) + 8))
    dev.upload(d_cells, cells)
    poison = np.full(positions * (n - 1) + 8, PAD, np.uint32)
    dev.upload(d_out, poison)
    ok = dict(d_cells=d_cells, pitch=pitch, n=n, first=3, positions=positions, remaining=50, d_out=d_out + 16)
    for change, message in ((dict(n=1), b"num_docs"), (dict(n=2049), b"num_docs"), (dict(n=0), b"num_docs"),
                            (dict(pitch=62), b"multiple of 4"), (dict(pitch=66), b"multiple of 4"),
                            (dict(first=25), b"do not lie inside"), (dict(first=pitch + 1, positions=0), b"do not lie inside"),
                            (dict(positions=62), b"do not lie inside"), (dict(remaining=39), b"remaining"), (dict(remaining=2 ** 31), b"2^31 - 1"),
                            (dict(d_cells=d_cells + 4), b"16-byte aligned"), (dict(d_cells=d_cells + 8), b"16-byte aligned"),
                            (dict(d_out=d_out + 18), b"4-byte aligned"), (dict(d_out=d_out + 17), b"4-byte aligned"),
                            (dict(first=-1), b"negative"), (dict(positions=-1), b"negative"), (dict(pitch=-4), b"negative"),
                            (dict(remaining=-1, positions=0), b"negative"), (dict(d_out=0), b"NULL"), (dict(d_cells=0), b"NULL")):
        a = dict(ok, **change)
        rc = dev.lib.memo_convert_dap_dev(a["d_cells"], a["pitch"], a["n"], a["first"], a["positions"], a["remaining"], a["d_out"], 0, None)
        assert rc == EINVAL and message in dev.lib.memo_last_error(), (change, dev.lib.memo_last_error())
        assert np.array_equal(dev.get(d_out, len(poison), np.uint32), poison), change
    # nothing to do launches nothing, whatever the pointers are
    assert dev.lib.memo_convert_dap_dev(0, pitch, n, 3, 0, 0, 0, 0, None) == 0
    assert np.array_equal(dev.get(d_out, len(poison), np.uint32), poison)
    a = ok
    dev.check(dev.lib.memo_convert_dap_dev(a["d_cells"], a["pitch"], a["n"], a["first"], a["positions"], a["remaining"], a["d_out"], 0, None))
    got = dev.get(d_out, len(poison), np.uint32)
    assert (got[:4] == PAD).all() and (got[-4:] == PAD).all()
    assert np.array_equal(got[4:-4].reshape(positions, n - 1), np.minimum(7, 50 - np.arange(positions))[:, None].repeat(n - 1, 1))


# ---------------------------------------------------------------------------------------
# one record's rows against the definition
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", (True, False))
@pytest.mark.parametrize("index,rec,n", RECORDS)
def test_rows_equal_the_definition_at_every_slice_and_batch_length(memo, wanted, index, rec, n, order):
    """The default sizes; every slice length at one batch length and every batch length at one slice length; the rows shuffled.  A slice
    or a batch of ONE position costs a record of P positions P rounds of launches: on the records above 3000 positions the slices of
    one run in the conservation order only and the batches of one in the membership order only (the orders differ in the row builder's
    sort, not in how a slice or a batch is cut); the shorter records cross them with both orders."""
    from memo_amd import convert, lengths
    s, e, a = G.index_columns(index, rec)
    short = int(s.max()) <= 3000
    settings = [dict()] + [dict(slice_positions=v, batch_positions=5) for v in (7, 64, lengths.tile() + 1)] + [dict(slice_positions=64, batch_positions=1000)]
    if short or order:
        settings.append(dict(slice_positions=1, batch_positions=5))
    if short or not order:
        settings.append(dict(slice_positions=64, batch_positions=1))
    want = wanted[(index, rec, order)]
    for kw in settings:
        same_rows(convert.rows(s, e, a, n, order=order, **kw), want, (index, rec, order, kw))
    shuffle = np.random.default_rng(3).permutation(len(s))
    for kw in (dict(), dict(slice_positions=7, batch_positions=5)):
        same_rows(convert.rows(s[shuffle], e[shuffle], a[shuffle], n, order=order, **kw), want, (index, rec, order, kw, "shuffled"))


def test_rows_of_odd_records(memo):
    from memo_amd import convert
    assert all(len(c) == 0 and c.dtype == np.int64 for c in convert.rows([], [], [], 3))             # no rows, no length: no positions
    assert all(len(c) == 0 for c in convert.rows([0, 0], [4, 9], [1, 2], 3))                         # rows at start 0 only
    s, e, a = np.array([4, 9, 9]), np.array([6, 9, 11]), np.array([1, 1, 2])
    for order in (True, False):
        for length in (None, 9, 12):
            for kw in (dict(), dict(slice_positions=1, batch_positions=1), dict(slice_positions=4, batch_positions=3)):
                same_rows(convert.rows(s, e, a, 3, order=order, length=length, **kw), convert_oracle.rows(s, e, a, 3, order=order, length=length),
                          (order, length, kw))
    got = convert.rows([], [], [], 3, length=6)                                                      # a record nothing is known about
    same_rows(got, convert_oracle.rows(np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64), 3, length=6), "empty, length 6")
    assert len(got[0])


# ---------------------------------------------------------------------------------------
# the promise, with the shipped sweeps
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("index,rec,n", RECORDS)
def test_the_shipped_sweeps_agree(memo, index, rec, n):
    """conservation of the converted rows = the number of membership bits of the source rows; membership of the -m rows = those bits;
    the -m rows convert to themselves"""
    from memo_amd import convert
    from memo_amd.index import DeviceIndex, bits_to_matrix
    s, e, a = G.index_columns(index, rec)
    L = int(s.max())
    cons = convert.rows(s, e, a, n, order=True)
    memb = convert.rows(s, e, a, n, order=False)
    same_rows(convert.rows(*memb, n, order=False, length=L), memb, (index, rec, "the -m rows again"))
    held = [DeviceIndex.from_host(*cols) for cols in ((s, e, a), cons, memb)]
    try:
        source, ix_cons, ix_memb = held
        for qs, qe in ((0, L), (L // 3, L - L // 4)):
            for k in KS:
                bits = bits_to_matrix(source.membership(qs, qe, k, n), n)
                assert np.array_equal(ix_cons.conservation(qs, qe, k, n), bits.sum(axis=1)), (index, rec, qs, qe, k)
                assert np.array_equal(bits_to_matrix(ix_memb.membership(qs, qe, k, n), n), bits), (index, rec, qs, qe, k)
    finally:
        for ix in held:
            ix.close()


# ---------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------
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
    return (t.column("f0").to_pylist(), *(t.column(c).to_numpy() for c in ("f1", "f2", "f3")))


def _same_table(path, want_path):
    got, want = _table(path), _table(want_path)
    assert got[0] == want[0] and all(np.array_equal(g, w) for g, w in zip(got[1:], want[1:])), (path, want_path)


def test_cli_converts_the_example_both_ways_and_the_result_is_queried(memo, tmp_path):
    memb, cons = os.path.join(G.GOLD, "example_memb.parquet"), os.path.join(G.GOLD, "example_cons.parquet")
    out = str(tmp_path / "out.parquet")
    r = _memo("convert", "-b", memb, "-n", "5", "-o", out)
    assert (r.returncode, r.stdout) == (0, b"MEMO - convert\n"), r.stderr
    _same_table(out, cons)
    assert os.listdir(tmp_path) == ["out.parquet"]                                  # written beside its name and renamed
    case = next(c for c in G.cases(raises=False, membership=False) if c["name"] == "ex_cons_k4_3_30")
    text = str(tmp_path / "query.txt")
    r = _memo("query", "-b", out, "-r", case["region"], "-k", str(case["k"]), "-n", str(case["n"]), "-o", text)
    assert r.returncode == 0 and open(text, "rb").read() == G.out_bytes(case), r.stderr
    r = _memo("convert", "-b", memb, "-n", "5", "-o", out, "-m", env={"MEMO_CONVERT_SLICE": "7", "MEMO_CONVERT_BATCH": "3"})
    assert (r.returncode, r.stdout) == (0, b"MEMO - convert\n"), r.stderr
    _same_table(out, memb)


@pytest.mark.parametrize("index,n", (("rnd_n4.parquet", 4), ("rnd_n40.parquet", 40)))
def test_cli_converts_two_records_in_order(memo, wanted, tmp_path, index, n):
    out = str(tmp_path / "two.parquet")
    r = _memo("convert", "-b", os.path.join(G.GOLD, index), "-n", str(n), "-o", out, env={"MEMO_CONVERT_SLICE": "64", "MEMO_CONVERT_BATCH": "50"})
    assert r.returncode == 0, r.stderr
    f0, s, e, a = _table(out)
    records = [rec for i, rec, _ in RECORDS if i == index]
    assert len(records) == 2 and list(dict.fromkeys(f0)) == records
    f0 = np.asarray(f0, dtype=object)
    at = 0
    for rec in records:
        want = wanted[(index, rec, True)]
        rows = slice(at, at + len(want[0]))
        assert (f0[rows] == rec).all()
        same_rows((s[rows], e[rows], a[rows]), want, (index, rec))
        at += len(want[0])
    assert at == len(s)


def test_cli_takes_record_lengths_from_a_fai(memo, tmp_path):
    memb = os.path.join(G.GOLD, "example_memb.parquet")
    fai = str(tmp_path / "pivot.fa.fai")
    open(fai, "w").write("other\t11\t5\t60\t61\nref_1\t30\t40\t60\t61\n")
    out = str(tmp_path / "longer.parquet")
    r = _memo("convert", "-b", memb, "-n", "5", "-o", out, "-f", fai)
    assert r.returncode == 0, r.stderr
    f0, s, e, a = _table(out)
    assert set(f0) == {"ref_1"} and int(s.max()) == 30
    same_rows((s, e, a), convert_oracle.rows(*G.index_columns("example_memb.parquet", "ref_1"), 5, order=True, length=30), "length 30")


def test_cli_refuses_and_converts_nothing(memo, tmp_path):
    import pyarrow as pa
    import pyarrow.parquet as pq
    out = str(tmp_path / "never.parquet")
    r = _memo("convert", "-b", os.path.join(G.GOLD, "rnd_negoverlap.parquet"), "-n", "12", "-o", out)
    assert r.returncode == 1 and r.stderr.startswith(b"memo convert: ") and b"ends before it starts" in r.stderr
    assert os.listdir(tmp_path) == []
    empty = str(tmp_path / "empty.parquet")
    pq.write_table(pa.table({"f0": pa.array([], pa.utf8()), "f1": pa.array([], pa.int64()), "f2": pa.array([], pa.int64()),
                             "f3": pa.array([], pa.int64())}), empty)
    for flags in ((), ("-m",)):
        r = _memo("convert", "-b", empty, "-n", "3", "-o", out, *flags)
        assert r.returncode == 0, r.stderr
        f0, s, e, a = _table(out)
        assert f0 == [] and len(s) == len(e) == len(a) == 0
    assert sorted(os.listdir(tmp_path)) == ["empty.parquet", "never.parquet"]
