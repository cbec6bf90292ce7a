"""Index-row construction on the device (memo_amd/csrc/memo_dap.hip: memo_dap_push / push_dev / finish) against
oracle/dap_oracle.dap_rows (whole-array NumPy, int64), bit for bit, where that code goes wrong:

  * widths around every 64-column chunk of count/write and every power of two of the --order bitonic network,
    past 2048 columns (more than one pair per thread per step), with dense ties and MS-like decays;
  * push shapes around the 256-row scan segments, single rows, pieces that end on a record end or one row
    before it, the block build_index uses, through push and through push_ms;
  * 10^5 tiny records (locate_kernel, records that open and close in one row, the finish() record scan);
  * one column of a DAP past 2^31 positions with a last record of 2^30 - 1, against closed-form rows;
  * values up to 2^31 - 1, whose MEM ends pass 2^31, through DapConverter and the dap_to_bed.py text path;
  * a seeded fuzz from tests/fuzz_dap_gpu.py's distribution with a fixed case count.

The one CPU test proves the closed form used for the 2^31 positions against dap_oracle on small instances."""
import io
import time

import numpy as np
import pytest

from oracle import dap_oracle as O

gpu = pytest.mark.gpu
MAX_RECORD = (1 << 30) - 1
FIELDS = ("rec", "start", "end", "annot")


@pytest.fixture(scope="module")
def D():
    from memo_amd import _lib, dap_to_bed
    _lib.lib()
    return dap_to_bed


def _same(got, want, what):
    for g, w, f in zip(got, want, FIELDS):
        g, w = np.asarray(g, np.int64), np.asarray(w, np.int64)
        assert g.shape == w.shape, f"{what}: {f}: {g.shape[0]} rows, want {w.shape[0]}"
        bad = np.flatnonzero(g != w)
        assert not len(bad), (f"{what}: {f} differs in {len(bad)} rows, first {bad[:6].tolist()}: "
                              f"got {g[bad[:6]].tolist()}, want {w[bad[:6]].tolist()}")


def _cat(batches):
    return [np.concatenate([b[i] for b in batches]) for i in range(4)]


def _convert(D, lcp, rec_begin, order, overlap, cuts=()):
    """rows of pushes of lcp[cuts[i]:cuts[i+1]] and finish(), concatenated"""
    bounds = [0, *sorted(set(int(c) for c in cuts if 0 < c < len(lcp))), len(lcp)]
    with D.DapConverter(lcp.shape[1], rec_begin, order, overlap) as conv:
        return _cat([conv.push(lcp[a:b]) for a, b in zip(bounds, bounds[1:])] + [conv.finish()])


def _rec_begin(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def _decays(rng, prev, n, hi, keep=0.7):
    """n MS-like rows after `prev`: each value is the one above minus 1 (floor 0) or, at 1 - keep, a fresh draw"""
    out = np.empty((n, len(prev)), np.int64)
    fresh, kept = rng.integers(0, hi, out.shape), rng.random(out.shape) < keep
    for i in range(n):
        prev = out[i] = np.where(kept[i], np.maximum(prev - 1, 0), fresh[i])
    return out


# ---- 1. widths ------------------------------------------------------------------------------------------------

WIDTHS = [1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096]


@gpu
@pytest.mark.parametrize("C", WIDTHS)
def test_widths_every_mode(D, C):
    """dense ties (values 0..2) then MS-like decays; a record of length 1; the DAP stops inside the last record"""
    rng = np.random.default_rng(C)
    rb = _rec_begin([900, 1, 613, 257, 1200])
    npos = 2400
    head = rng.integers(0, 3, (1100, C))
    lcp = np.vstack([head, _decays(rng, head[-1], npos - 1100, 40)]).astype(np.int32)
    ordered = -np.sort(-lcp.astype(np.int64), axis=1)
    for order in (False, True):
        for overlap in (False, True):
            want = O.dap_rows(ordered if order else lcp, rb, overlap, False)
            _same(_convert(D, lcp, rb, order, overlap, (1000, 1771)), want, f"C={C} order={order} overlap={overlap}")


# ---- 2. push shapes -------------------------------------------------------------------------------------------

def _push_splits(rb, npos, C):
    ends = rb[1:-1][rb[1:-1] < npos]
    return {
        "rows of 1": range(1, npos),
        "rows of 255": range(255, npos, 255),
        "rows of 256": range(256, npos, 256),
        "rows of 257": range(257, npos, 257),
        "record ends": ends,
        "one before record ends": ends - 1,
        "build_index block": range(max(1024, (64 << 20) // C), npos, max(1024, (64 << 20) // C)),
        "one push": (),
    }


@gpu
@pytest.mark.parametrize("C", [5, 70])
def test_push_shapes(D, C):
    rng = np.random.default_rng(100 + C)
    rb = _rec_begin([256, 1, 1, 255, 257, 512, 1, 700, 2])
    npos = int(rb[-1]) - 1                                   # stops inside the last record
    lcp = np.vstack([rng.integers(0, 4, (600, C)), _decays(rng, np.zeros(C, np.int64), npos - 600, 300)]).astype(np.int32)
    for order in (False, True):
        for overlap in (False, True):
            want = O.dap_rows(lcp, rb, overlap, order)
            for name, cuts in _push_splits(rb, npos, C).items():
                _same(_convert(D, lcp, rb, order, overlap, cuts), want, f"C={C} order={order} overlap={overlap}: {name}")


@gpu
def test_push_ms_shapes(D):
    """the same splits through memo_ms_push_dap on a small MatchingStatistics handle"""
    from memo_amd import build_index as bi
    rng = np.random.default_rng(7)
    lens = [256, 1, 1, 255, 257, 512, 1, 700, 2]
    pivot = [bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)]) for n in lens]
    seq, rb = b"".join(pivot), _rec_begin(lens)
    texts = [bi.genome_text([bytes(np.where(rng.random(len(seq)) < r, ord("A"), np.frombuffer(seq, np.uint8)).astype(np.uint8))])
             for r in (0.0, 0.02, 0.3)]
    npos = len(seq)
    with bi.MatchingStatistics(seq, rb, len(texts)) as ms:
        for c, t in enumerate(texts):
            ms.add(t, c)
        mat = ms.fetch()
        assert mat[:, 0].max() > 100 and mat[:, 2].max() < mat[:, 0].max()
        for order in (False, True):
            for overlap in (False, True):
                want = O.dap_rows(mat, rb, overlap, order)
                for name, cuts in _push_splits(rb, npos, len(texts)).items():
                    bounds = [0, *sorted(set(int(c) for c in cuts if 0 < c < npos)), npos]
                    with D.DapConverter(len(texts), rb, order, overlap) as conv:
                        got = _cat([conv.push_ms(ms, a, b - a) for a, b in zip(bounds, bounds[1:])] + [conv.finish()])
                    _same(got, want, f"push_ms order={order} overlap={overlap}: {name}")


def _ms_like(rng, npos, C, reset=0.02, hi=5000):
    """decays by one with rare jumps (few MEM starts): value = max(h - (p - last jump), 0), vectorised"""
    jump = rng.random((npos, C)) < reset
    jump[0] = True
    p = np.arange(npos)[:, None]
    last = np.maximum.accumulate(np.where(jump, p, 0), axis=0)
    h = rng.integers(0, hi, (npos, C))
    return np.maximum(np.take_along_axis(h, last, 0) - (p - last), 0).astype(np.int32)


@gpu
def test_build_index_block_at_4096_columns(D):
    """4096 columns: build_index's block is 16384 rows; blocks, odd pieces and one push give identical rows"""
    C = 4096
    block = max(1024, (64 << 20) // C)
    rb = _rec_begin([block - 1, 1, block + 1, 299])
    npos = int(rb[-1])
    lcp = _ms_like(np.random.default_rng(4096), npos, C)
    for order in (True, False):                              # conservation / membership index
        one = _convert(D, lcp, rb, order, True)
        assert len(one[0]) > 100_000
        for cuts in (range(block, npos, block), range(4099, npos, 4099), (block - 1, block, 2 * block)):
            _same(_convert(D, lcp, rb, order, True, cuts), one, f"order={order} cuts {cuts}")
    tail = lcp[-600:]                                         # and the rows of the last two records against the oracle
    rb_tail = np.array([0, 301, 600], np.int64)
    _same(_convert(D, tail, rb_tail, True, True, (256,)), O.dap_rows(tail, rb_tail, True, True), "tail vs oracle")


# ---- 3. many records ------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("C", [2, 33])
@pytest.mark.parametrize("layout", ["1e5 records of 1-3", "lengths 1 and 1e4"])
def test_many_records(D, C, layout):
    rng = np.random.default_rng(C)
    if layout.startswith("1e5"):
        lens = rng.integers(1, 4, 100_000)
        lens[-1] = 3
    else:
        lens = np.where(rng.random(250) < 0.9, 1, 10_000)
        lens[-2:] = (1, 10_000)
    rb = _rec_begin(lens)
    npos = int(rb[-1]) - 2                                   # stops inside the last record: finish() scans them all
    lcp = rng.integers(0, 4, (npos, C)).astype(np.int32)
    lcp[rng.random(npos) < 0.3] = 0
    cuts = rng.integers(1, npos, 5)
    for order, overlap in ((True, True), (False, False)):
        want = O.dap_rows(lcp, rb, overlap, order)
        _same(_convert(D, lcp, rb, order, overlap, cuts), want, f"{layout} C={C} order={order} overlap={overlap}")


# ---- 4. long coordinates: closed-form rows of a sawtooth DAP ---------------------------------------------------

def sawtooth(rel, period, base):
    """DAP value at position rel of its record: strictly decreasing runs base + period - 1 .. base"""
    return base + (period - 1) - rel % period


def sawtooth_rows(lens, period, base, overlap):
    """(rec, start, end, annot) of one sawtooth column over whole records, in print order, without the oracle.
    A MEM starts exactly at each run start kP (the value jumps up there, and falls inside a run) and ends at
    kP + base + P - 1.  --mem prints every MEM and the chr-end row (L, 2L).  --overlap prints the run at kP,
    k >= 1, against the one before: end min(kP + base - 1, kP + base + P - 1) = kP + base - 1 when base >= 1; and
    at the chr end min(s + base + P - 1, 2L) for the last run start s, when that is >= L."""
    out = []
    for r, L in enumerate(int(x) for x in lens):
        starts = np.arange(0, L, period, dtype=np.int64)
        if not overlap:
            ends = starts + base + period - 1
            start, end = np.append(starts, L), np.append(ends, 2 * L)
        else:
            starts = starts[1:] if base >= 1 else starts[:0]
            ends = starts + base - 1
            e = min(((L - 1) // period) * period + base + period - 1, 2 * L)
            start, end = (np.append(starts, L), np.append(ends, e)) if e >= L else (starts, ends)
        out.append((np.full(len(start), r, np.int64), start, end, np.ones(len(start), np.int64)))
    return _cat(out)


@pytest.mark.parametrize("base", [0, 1, 5, 1 << 30, (1 << 31) - 7])
def test_sawtooth_closed_form_equals_the_oracle(base):
    """CPU: the closed form of the long-coordinate test against dap_oracle on a scaled-down instance"""
    period = 7
    lens = [1, 6, 7, 8, 13, 14, 15, 50, 3, 1]
    rb = _rec_begin(lens)
    rel = np.arange(rb[-1]) - rb[np.searchsorted(rb, np.arange(rb[-1]), side="right") - 1]
    lcp = sawtooth(rel, period, base)[:, None]
    assert lcp.max() < 2 ** 31
    for overlap in (False, True):
        for order in (False, True):
            _same(sawtooth_rows(lens, period, base, overlap), O.dap_rows(lcp, rb, overlap, order),
                  f"base={base} overlap={overlap} order={order}")


@gpu
def test_positions_past_2_31(D):
    """one column, records totalling 2^31 + 1233567 positions, the last exactly MAX_RECORD = 2^30 - 1 long, pushed
    in build_index blocks (2^26 rows at one column); every row against the closed form.  Global positions pass 2^31
    in the last record, 2 L reaches 2^31 - 2, values reach 2^31 - 2, and MEM ends pass 2^31 in both modes."""
    period = 4093
    base = (1 << 31) - period - 1
    lens = np.array([MAX_RECORD - 1000, 1, 1, 1_234_567, MAX_RECORD], np.int64)
    rb = _rec_begin(lens)
    total = int(rb[-1])
    assert total > 2 ** 31 and lens.max() == MAX_RECORD and base + period - 1 < 2 ** 31
    block = max(1024, (64 << 20) // 1)
    buf = np.empty(block, np.int32)
    for order, overlap in ((True, True), (False, False)):
        t0 = time.perf_counter()
        batches = []
        with D.DapConverter(1, rb, order, overlap) as conv:
            for g0 in range(0, total, block):
                g1 = min(g0 + block, total)
                for r in range(len(lens)):
                    a, b = max(g0, rb[r]), min(g1, rb[r + 1])
                    if a < b:
                        rel = np.arange(a - rb[r], b - rb[r], dtype=np.int32)
                        buf[a - g0:b - g0] = sawtooth(rel, period, base)
                batches.append(conv.push(buf[:g1 - g0, None]))
            batches.append(conv.finish())
        got = _cat(batches)
        assert got[2].max() > 2 ** 31 and (got[2] < 0).sum() == 0
        _same(got, sawtooth_rows(lens, period, base, overlap), f"order={order} overlap={overlap}")
        print(f"2^31 positions, overlap={overlap}: {len(got[0])} rows in {time.perf_counter() - t0:.1f} s")


# ---- 5. value extremes ----------------------------------------------------------------------------------------

EXTREMES = [0, (1 << 30) - 1, (1 << 31) - 2, (1 << 31) - 1]


def _extreme_cases():
    """(name, rec lengths, lcp int64): the 10-position example of a MEM end past 2^31, then every extreme at every
    position of records of lengths 10, 1, 3 and 12 (rel 0, 1 and the last two), cyclically and at random"""
    ten = np.zeros((10, 1), np.int64)
    ten[1], ten[2] = 2 ** 31 - 1, 5
    lens = [10, 1, 3, 12]
    n = sum(lens)
    cyc = np.array(EXTREMES)[(np.arange(n)[:, None] + np.arange(4)[None, :]) % 4]
    cases = [("ten", [10], ten), ("cyclic", lens, cyc), ("cyclic reversed", lens, cyc[::-1].copy())]
    rng = np.random.default_rng(31)
    cases += [(f"random {i}", lens, np.array(EXTREMES)[rng.integers(0, 4, (n, 5))]) for i in range(4)]
    return cases


def test_ten_position_example_in_the_oracle():
    """CPU: what the reference prints for the issue's example (Python ints: no wrap)"""
    lcp = _extreme_cases()[0][2]
    rb = _rec_begin([10])
    rows = list(zip(*O.dap_rows(lcp, rb, False, False)))
    assert (0, 1, 2 ** 31, 1) in rows
    assert list(zip(*O.dap_rows(lcp, rb, True, False)))[0] == (0, 4, 4, 1)


@gpu
@pytest.mark.parametrize("case", _extreme_cases(), ids=lambda c: c[0])
def test_value_extremes(D, case, tmp_path):
    name, lens, lcp = case
    rb = _rec_begin(lens)
    names = [f"chr{i}" for i in range(len(lens))]
    fai, dap = tmp_path / "p.fa.fai", tmp_path / "p.dap"
    fai.write_text("".join(f"{nm}\t{L}\t0\t60\t61\n" for nm, L in zip(names, lens)))
    dap.write_text("".join(" ".join(map(str, [i, *row])) + "\n" for i, row in enumerate(lcp.tolist())))
    for order in (False, True):
        for overlap in (False, True):
            what = f"{name} order={order} overlap={overlap}"
            want = O.dap_rows(lcp, rb, overlap, order)
            _same(_convert(D, lcp, rb, order, overlap), want, what + " int64 push")
            _same(_convert(D, lcp.astype(np.int32), rb, order, overlap, (1, 11)), want, what + " int32 push")
            argv = ["--mem", "--fai", str(fai), "--dap", str(dap)] + (["--overlap"] * overlap) + (["--order"] * order)
            args = D.parse_arguments(argv)
            D.check_args(args)
            buf = io.BytesIO()
            D.main(args, buf)
            assert buf.getvalue().decode() == O.bed_text(names, *want), what + " text path"


@gpu
@pytest.mark.parametrize("dtype", [np.int8, np.int16, np.int32, np.int64, np.uint8, np.uint16, np.uint32, np.uint64])
def test_values_out_of_range_raise(D, dtype, tmp_path):
    rb = _rec_begin([4])
    bad = []
    if np.issubdtype(dtype, np.signedinteger):
        bad.append(-1)
    if np.iinfo(dtype).max >= 2 ** 31:
        bad.append(2 ** 31)
    if np.iinfo(dtype).max >= 2 ** 32:
        bad.append(2 ** 63 - 1 if dtype == np.int64 else 2 ** 64 - 1)
    for v in bad:
        lcp = np.array([[0], [3], [v], [1]], dtype)
        with D.DapConverter(1, rb, False, True) as conv:
            with pytest.raises(ValueError):
                conv.push(lcp)
    if np.iinfo(dtype).max < 2 ** 31:
        ok = np.array([[0], [np.iinfo(dtype).max], [1], [0]], dtype)
        want = O.dap_rows(ok, rb, False, True)
        _same(_convert(D, ok, rb, True, False), want, f"{np.dtype(dtype).name} max")
    for v in (-1, 2 ** 31):                                   # and the text path
        fai, dap = tmp_path / "p.fa.fai", tmp_path / "p.dap"
        fai.write_text("chr1\t4\t0\t60\t61\n")
        dap.write_text(f"0 0\n1 3\n2 {v}\n3 1\n")
        args = D.parse_arguments(["--mem", "--overlap", "--fai", str(fai), "--dap", str(dap)])
        with pytest.raises(ValueError):
            D.main(args, io.BytesIO())


# ---- 6. seeded fuzz -------------------------------------------------------------------------------------------

@gpu
def test_seeded_fuzz(D):
    """tests/fuzz_dap_gpu.py's distribution, fixed seed and case count"""
    rng = np.random.default_rng(20261015)
    t0 = time.perf_counter()
    for case in range(200):
        C_ = int(rng.choice([1, 2, 3, 31, 32, 33, 64, 65, 99, 128, 129, 499, 700]))
        nrec = int(rng.integers(1, 6))
        lens = rng.integers(1, int(rng.choice([3, 50, 2000])), nrec)
        rb = _rec_begin(lens)
        total = int(rb[-1])
        npos = total if rng.random() < 0.7 else int(rng.integers(1, total + 1))
        hi = int(rng.choice([2, 10, 60, 5000]))
        lcp = rng.integers(0, hi, (npos, C_)).astype(np.int32)
        if rng.random() < 0.5:
            for i in range(1, npos):
                keep = rng.random(C_) < 0.8
                lcp[i] = np.where(keep, np.maximum(lcp[i - 1] - 1, 0), lcp[i])
        order, overlap = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
        pieces = int(rng.choice([1, 2, 5, 17]))
        cuts = np.cumsum([len(p) for p in np.array_split(lcp, pieces)])[:-1]
        _same(_convert(D, lcp, rb, order, overlap, cuts), O.dap_rows(lcp, rb, overlap, order),
              f"case {case}: C={C_} lens={lens.tolist()} npos={npos} order={order} overlap={overlap} pieces={pieces}")
    print(f"dap fuzz: 200 cases in {time.perf_counter() - t0:.1f} s")
