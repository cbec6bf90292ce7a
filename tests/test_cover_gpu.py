"""`memo cover` on the GPU: the kernels of memo_amd/csrc/memo_cover.hip against NumPy on the host -- the weights against the definition,
the scores and the take against min, max and sums of whole planes, on cells of the full cell range --, the window route against the
worked tables (tests/cover_tables.py) and against `memo panel` at one k, the command line against the README's bytes.  Every comparison
is exact."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import cover_tables as T
from tests import golden_util as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "memo")
CAP_MAX = 2 ** 31 - 1
EXAMPLE_INDEX, RND40_INDEX = os.path.join(G.GOLD, "example_memb.parquet"), os.path.join(G.GOLD, "rnd_n40.parquet")
DTYPE = {2: np.uint16, 4: np.uint32}
SENTINEL = {2: 0xA5C3, 4: 0xA5C3F00F}
# (kmin, kmax) with the largest span each cell width holds
SPANS = {2: (5, 65539), 4: (5, CAP_MAX)}


@pytest.fixture(scope="module")
def memo():
    import memo_amd
    from memo_amd import _lib
    memo_amd.build()                     # make: a no-op when libmemo_amd.so is up to date
    assert _lib.lib().memo_device_count() > 0, "no HIP device: the product has no CPU fallback"
    return memo_amd


def want_weights(lengths, kmin, kmax):
    v = np.minimum(lengths.astype(np.int64), kmax)
    return np.maximum(v - (kmin - 1), 0)


def weights_call(d_lengths, Ls, pitch_src, num_docs, kmin, kmax, genomes, d_weights, pitch, cell_bytes, cell0, n_list=None):
    from memo_amd._lib import check, lib
    ids = np.ascontiguousarray(genomes, np.uint16)
    check(lib().memo_cover_weights_dev(d_lengths, Ls, pitch_src, num_docs, kmin, kmax, ids.ctypes.data, len(ids) if n_list is None else n_list, d_weights, pitch,
                                       cell_bytes, cell0, 0, None))


# ---------------------------------------------------------------------------------------
# memo_cover_weights_dev against the definition
# ---------------------------------------------------------------------------------------
def test_the_pass(memo):
    from memo_amd import cover
    assert (cover.pass_cells(2), cover.pass_cells(4), cover.pass_cells(1), cover.pass_cells(8)) == (2048, 1024, 0, 0)


@pytest.mark.parametrize("cell_bytes", (2, 4))
def test_weights_equal_the_definition_at_every_length_and_offset(memo, cell_bytes):
    """cells [cell0, cell0 + Ls) of plane i are w[list[i]], narrowed; every other cell of a sentinel-filled buffer with a pitch wider
    than needed, and the plane behind the last, stay the sentinel.  The lengths sit at kmin - 1, kmin, kmax and above kmax as well as
    between, and what lies behind Ls in their pitch is garbage that reaches no plane."""
    from memo_amd import cover
    from memo_amd._device import DevBuffer
    kmin, kmax = SPANS[cell_bytes]
    per, N, dtype = cover.pass_cells(cell_bytes), 6, DTYPE[cell_bytes]
    sizes = (1, 7, 8, 9, per - 1, per, per + 1, 3 * per + 5)
    rng = np.random.default_rng([1, cell_bytes])
    edges = np.array([0, 1, kmin - 1, kmin, kmin + 1, kmax - 1, kmax, kmax + 1, 2 ** 32 - 1], np.uint64)
    full = np.where(rng.random((N, sizes[-1])) < 0.5, rng.choice(edges, (N, sizes[-1])), rng.integers(0, min(2 * kmax, 2 ** 32), (N, sizes[-1]), dtype=np.uint64)).astype(np.uint32)
    lists = ([0, 1, 2, 3, 4, 5], [4, 2], [5, 0, 3, 1], [2, 2, 5, 2])                 # everyone, a subset, reordered, repeats
    for Ls in sizes:
        pitch_src = (Ls + 3) // 4 * 4 + 4
        src = np.full((N, pitch_src), 0xFFFFFFFF, np.uint32)
        src[:, :Ls] = full[:, :Ls]
        want = want_weights(full[:, :Ls], kmin, kmax)
        assert int(want.max()) <= kmax - kmin + 1
        with DevBuffer.of(src, 0) as lengths:
            for at, cell0 in enumerate((0, 8, 40)):
                genomes = lists[(at + Ls) % len(lists)]
                pitch = (cell0 + Ls + 15) // 16 * 16 + 16
                filled = np.full((len(genomes) + 1, pitch), SENTINEL[cell_bytes], dtype)
                with DevBuffer.of(filled, 0) as planes:
                    weights_call(lengths.d, Ls, pitch_src, N, kmin, kmax, genomes, planes.d, pitch, cell_bytes, cell0)
                    got = planes.to_host(filled.shape, dtype)
                assert np.array_equal(got[:len(genomes), cell0:cell0 + Ls].astype(np.int64), want[genomes]), (cell_bytes, Ls, cell0)
                got[:len(genomes), cell0:cell0 + Ls] = SENTINEL[cell_bytes]
                assert (got == SENTINEL[cell_bytes]).all(), (cell_bytes, Ls, cell0)


def test_weights_of_slices_laid_end_to_end(memo):
    """three slices of one window, written out of order into one buffer, are the window's weights; kmin = kmax gives bits"""
    from memo_amd._device import DevBuffer
    N, L = 9, 2 * 2048 + 8 * 7 + 5
    lens = np.random.default_rng(2).integers(0, 40, (N, L), dtype=np.uint32)
    cuts = [0, 8 * 5, 2048 + 8, L]
    for cell_bytes, (kmin, kmax) in ((2, (1, 31)), (2, (12, 12)), (4, (1, 100000))):
        genomes = [7, 1, 8, 3]
        pitch = (L + 7) // 8 * 8
        with DevBuffer.of(np.full((len(genomes), pitch), SENTINEL[cell_bytes], DTYPE[cell_bytes]), 0) as planes:
            for a, b in reversed(list(zip(cuts, cuts[1:]))):
                part = np.zeros((N, (b - a + 3) // 4 * 4), np.uint32)
                part[:, :b - a] = lens[:, a:b]
                with DevBuffer.of(part, 0) as lengths:
                    weights_call(lengths.d, b - a, part.shape[1], N, kmin, kmax, genomes, planes.d, pitch, cell_bytes, a)
            got = planes.to_host((len(genomes), pitch), DTYPE[cell_bytes])
        assert np.array_equal(got[:, :L].astype(np.int64), want_weights(lens, kmin, kmax)[genomes]) and (got[:, L:] == SENTINEL[cell_bytes]).all()


# ---------------------------------------------------------------------------------------
# memo_cover_begin_dev, memo_cover_score_dev and memo_cover_take_dev against NumPy
# ---------------------------------------------------------------------------------------
class Vectors:
    """random planes of N genomes over `cells` cells (a multiple of a quad) and two random vectors, on the host and on the device,
    all of the FULL range of the cell type: the formulas hold literally, not only for weights up to a span.  The cells between
    `cells` and the pitch hold ones, which nothing may count."""

    def __init__(self, N, cells, cell_bytes, seed, extra=16, fill=None):
        from memo_amd._device import DevBuffer
        rng = np.random.default_rng([seed, N, cells, cell_bytes])
        self.N, self.cells, self.cell_bytes, self.dtype = N, cells, cell_bytes, DTYPE[cell_bytes]
        assert cells % (16 // cell_bytes) == 0
        top = 2 ** (8 * cell_bytes)
        self.pitch = cells + extra
        self.planes = np.full((N, self.pitch), top - 1, self.dtype)
        if fill is None:
            self.planes[:, :cells] = rng.integers(0, top, (N, cells), dtype=np.uint64)
            self.core = rng.integers(0, top, cells, dtype=np.uint64).astype(self.dtype)
            self.covered = rng.integers(0, top, cells, dtype=np.uint64).astype(self.dtype)
        else:
            self.planes[:, :cells] = fill
            self.core, self.covered = np.full(cells, fill, self.dtype), np.zeros(cells, self.dtype)
        self.d_planes, self.d_core, self.d_covered = (DevBuffer.of(a, 0) for a in (self.planes, self.core, self.covered))

    def score(self, planes, out=None, **over):
        from memo_amd._lib import check, lib
        ids = np.ascontiguousarray(planes, np.uint16)
        out = np.zeros((len(ids), 2), np.uint64) if out is None else out
        a = dict(base=self.d_planes.d, pitch=self.pitch, N=self.N, cell_bytes=self.cell_bytes, cells=self.cells, core=self.d_core.d, covered=self.d_covered.d, n=len(ids))
        a.update(over)
        check(lib().memo_cover_score_dev(a["base"], a["pitch"], a["N"], a["cell_bytes"], a["cells"], a["core"], a["covered"], ids.ctypes.data, a["n"],
                                         out.ctypes.data, 0, None))
        return out

    def take(self, plane, out=None, **over):
        from memo_amd._lib import check, lib
        out = np.zeros(2, np.uint64) if out is None else out
        a = dict(base=self.d_planes.d, pitch=self.pitch, N=self.N, cell_bytes=self.cell_bytes, cells=self.cells, core=self.d_core.d, covered=self.d_covered.d)
        a.update(over)
        check(lib().memo_cover_take_dev(a["base"], a["pitch"], a["N"], a["cell_bytes"], a["cells"], plane, a["core"], a["covered"], out.ctypes.data, 0, None))
        return out

    def want_scores(self, planes):
        core, covered = self.core.astype(np.int64), self.covered.astype(np.int64)
        rows = self.planes[np.asarray(planes, np.int64), :self.cells].astype(np.int64)
        return [[int(np.maximum(w - covered, 0).sum()), int(np.minimum(w, core).sum())] for w in rows]

    def device_vectors(self):
        return self.d_core.to_host(self.core.shape, self.dtype), self.d_covered.to_host(self.covered.shape, self.dtype)

    def close(self):
        for b in (self.d_planes, self.d_core, self.d_covered):
            b.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def cell_counts(cell_bytes):
    from memo_amd import cover
    per, quad = cover.pass_cells(cell_bytes), 16 // cell_bytes
    return (quad, per - quad, per, per + quad, 3 * per)


LISTS = ([11], [3, 1, 4, 15, 9, 2, 6], [5, 3, 18, 9, 7, 1, 12, 0], [19, 8, 7, 6, 5, 4, 3, 2, 1], list(range(17)), [4, 9, 4, 4, 0, 9, 19, 4, 9, 4])


@pytest.mark.parametrize("cell_bytes", (2, 4))
def test_scores_equal_numpy(memo, cell_bytes):
    """lists of 1, 7, 8, 9 and 17 planes and one with repeats (a block of the kernel is 8), at one quad, a quad below and above a
    workgroup's pass, and several workgroups along the cells; the vectors stay as they were"""
    for cells in cell_counts(cell_bytes):
        with Vectors(20, cells, cell_bytes, seed=4) as v:
            for planes in LISTS:
                got = v.score(planes)
                assert got.dtype == np.uint64 and got.tolist() == v.want_scores(planes), (cell_bytes, cells, planes)
            core, covered = v.device_vectors()
            assert np.array_equal(core, v.core) and np.array_equal(covered, v.covered)
            assert v.score([]).shape == (0, 2)


@pytest.mark.parametrize("cell_bytes", (2, 4))
def test_scores_of_many_planes_and_sums_past_32_bits(memo, cell_bytes):
    from memo_amd import cover
    quad, per = 16 // cell_bytes, cover.pass_cells(cell_bytes)
    with Vectors(2048, quad, cell_bytes, seed=5, extra=0) as v:
        everyone = np.random.default_rng(6).permutation(2048)
        assert v.score(everyone).tolist() == v.want_scores(everyone)               # 256 blocks of candidates of one quad, the pitch with nothing to spare
    # every cell the span, at the largest span the cell holds, over one pass: with 4-byte cells a lane's sum passes 2^32
    span = 65535 if cell_bytes == 2 else CAP_MAX
    with Vectors(3, per, cell_bytes, seed=7, fill=span) as v:
        assert v.score([0, 1, 2, 1]).tolist() == [[per * span, per * span]] * 4
        assert v.take(2).tolist() == [per * span, per * span]
        assert v.score([0]).tolist() == [[0, per * span]]                          # everything is covered now
    if cell_bytes == 2:
        # ... and with 2-byte cells where a workgroup takes 130 passes (2048 candidates leave 8 workgroups along the cells): a wave's sum
        # and a workgroup's pass 2^32, which the 32-bit lane sums may not carry into the reduce
        cells = 8 * 130 * per
        with Vectors(1, cells, 2, seed=8, fill=span) as v:
            assert v.score([0] * 2048).tolist() == [[cells * span, cells * span]] * 2048
            assert v.take(0).tolist() == [cells * span, cells * span]


@pytest.mark.parametrize("cell_bytes", (2, 4))
def test_take_equals_numpy_step_by_step(memo, cell_bytes):
    for cells in cell_counts(cell_bytes):
        with Vectors(6, cells, cell_bytes, seed=8) as v:
            core, covered = v.core.copy(), v.covered.copy()
            for g in (3, 0, 5, 3):
                core, covered = np.minimum(core, v.planes[g, :cells]), np.maximum(covered, v.planes[g, :cells])
                got = v.take(g)
                assert got.tolist() == [int(core.astype(np.int64).sum()), int(covered.astype(np.int64).sum())], (cell_bytes, cells, g)
                now = v.device_vectors()
                assert np.array_equal(now[0], core) and np.array_equal(now[1], covered), (cell_bytes, cells, g)
                v.core, v.covered = core, covered                                   # ... and the scores against the vectors as they are now
                assert v.score([1, 2, 4]).tolist() == v.want_scores([1, 2, 4])
            assert np.array_equal(v.d_planes.to_host(v.planes.shape, v.dtype), v.planes)


@pytest.mark.parametrize("cell_bytes", (2, 4))
def test_begin_writes_the_vectors_and_the_pads_alone(memo, cell_bytes):
    from memo_amd._device import DevBuffer
    from memo_amd._lib import check, lib
    dtype, quad, S = DTYPE[cell_bytes], 16 // cell_bytes, SENTINEL[cell_bytes]
    span = 65535 if cell_bytes == 2 else CAP_MAX
    for N, L in ((5, 1), (5, quad - 1), (5, quad), (70, quad + 1), (3, 127), (3, 128), (2048, 161), (9, 5 * 2048 + 3)):
        cells = (L + quad - 1) // quad * quad
        pitch = cells + quad
        filled = np.full((N + 1, pitch), S, dtype)
        with DevBuffer.of(filled, 0) as planes, DevBuffer.of(np.full(cells + quad, S, dtype), 0) as core, DevBuffer.of(np.full(cells + quad, S, dtype), 0) as covered:
            check(lib().memo_cover_begin_dev(planes.d, pitch, N, cell_bytes, L, span, core.d, covered.d, 0, None))
            got = planes.to_host(filled.shape, dtype)
            assert (got[:N, L:cells] == 0).all() and (got[:N, :L] == S).all() and (got[:N, cells:] == S).all() and (got[N] == S).all(), (N, L)
            a, o = core.to_host(cells + quad, dtype), covered.to_host(cells + quad, dtype)
            assert (a[:L] == span).all() and (a[L:cells] == 0).all() and (a[cells:] == S).all(), (N, L)
            assert (o[:cells] == 0).all() and (o[cells:] == S).all(), (N, L)


@pytest.mark.parametrize("cell_bytes", (2, 4))
def test_score_take_and_begin_refusals_leave_everything_unchanged(memo, cell_bytes):
    from memo_amd._lib import MEMO_EINVAL, MemoError, check, lib
    N, quad = 20, 16 // cell_bytes
    with Vectors(N, 3 * quad, cell_bytes, seed=9, extra=2 * quad) as v:
        assert all(b.d.value % 16 == 0 for b in (v.d_planes, v.d_core, v.d_covered))
        good = [3, 1, 4]
        cases = (("planes not 16-byte aligned", good, dict(base=v.d_planes.at(cell_bytes))),
                 ("planes NULL", good, dict(base=None)),
                 ("a pitch that is no multiple of a quad", good, dict(pitch=v.pitch - 1)),
                 ("a pitch of 0", good, dict(pitch=0)),
                 ("cells that are no multiple of a quad", good, dict(cells=3 * quad - 1)),
                 ("cells past the pitch", good, dict(cells=v.pitch + quad)),
                 ("cells below 0", good, dict(cells=-quad)),
                 ("cell_bytes 1", good, dict(cell_bytes=1)),
                 ("cell_bytes 8", good, dict(cell_bytes=8)),
                 ("cell_bytes 0", good, dict(cell_bytes=0)),
                 ("core not 16-byte aligned", good, dict(core=v.d_core.at(4))),
                 ("covered not 16-byte aligned", good, dict(covered=v.d_covered.at(8))),
                 ("covered NULL", good, dict(covered=None)),
                 ("N = 0", good, dict(N=0)),
                 ("N above the bound", good, dict(N=2049)),
                 ("an entry = N", [3, N, 4], dict()),
                 ("n_list below 0", good, dict(n=-1)),
                 ("n_list above the bound", good, dict(n=65536)))

        def unchanged(what):
            core, covered = v.device_vectors()
            assert np.array_equal(core, v.core) and np.array_equal(covered, v.covered), what
            assert np.array_equal(v.d_planes.to_host(v.planes.shape, v.dtype), v.planes), what
        for what, planes, over in cases:
            out = np.full((3, 2), 7, np.uint64)
            with pytest.raises(MemoError) as err:
                v.score(planes, out, **over)
            assert err.value.code == MEMO_EINVAL and (out == 7).all(), what
        for what, planes, over in cases[:15] + (("plane = N", N, dict()), ("plane below 0", -1, dict())):
            out = np.full(2, 7, np.uint64)
            with pytest.raises(MemoError) as err:
                v.take(planes[0] if isinstance(planes, list) else planes, out, **over)
            assert err.value.code == MEMO_EINVAL and (out == 7).all(), what
            unchanged(what)
        span = 65535 if cell_bytes == 2 else CAP_MAX
        a = dict(base=v.d_planes.d, pitch=v.pitch, N=N, cell_bytes=cell_bytes, L=3 * quad - 1, span=span, core=v.d_core.d, covered=v.d_covered.d)
        begins = [(what, over) for what, _, over in cases[:15] if "cells" not in over]
        begins += [("L below 0", dict(L=-1)), ("a window wider than the pitch", dict(L=v.pitch + 1)), ("a span of 0", dict(span=0)), ("a span past 2^31 - 1", dict(span=2 ** 31))]
        if cell_bytes == 2:
            begins.append(("a span that does not fit the cell", dict(span=65536)))
        for what, over in begins:
            b = dict(a, **over)
            with pytest.raises(MemoError) as err:
                check(lib().memo_cover_begin_dev(b["base"], b["pitch"], b["N"], b["cell_bytes"], b["L"], b["span"], b["core"], b["covered"], 0, None))
            assert err.value.code == MEMO_EINVAL, what
            unchanged(what)
        assert v.score(good).tolist() == v.want_scores(good)                       # and the same call with nothing to refuse


@pytest.mark.parametrize("cell_bytes", (2, 4))
def test_weights_refusals_leave_the_planes_unchanged(memo, cell_bytes):
    from memo_amd._device import DevBuffer
    from memo_amd._lib import MEMO_EINVAL, MemoError
    N, Ls, pitch_src, pitch = 7, 21, 24, 48
    kmin, kmax = SPANS[cell_bytes]
    dtype, S = DTYPE[cell_bytes], SENTINEL[cell_bytes]
    src = np.random.default_rng(10).integers(0, 2 ** 32, (N, pitch_src), dtype=np.uint64).astype(np.uint32)
    good = [3, 6, 0]
    filled = np.full((len(good), pitch), S, dtype)
    with DevBuffer.of(src, 0) as lengths, DevBuffer.of(filled, 0) as planes:
        a = dict(lengths=lengths.d, Ls=Ls, pitch_src=pitch_src, N=N, kmin=kmin, kmax=kmax, genomes=good, planes=planes.d, pitch=pitch, cell_bytes=cell_bytes, cell0=8, n=None)
        cases = [("lengths not 16-byte aligned", dict(lengths=lengths.at(4))), ("lengths NULL", dict(lengths=None)), ("planes NULL", dict(planes=None)),
                 ("planes not 16-byte aligned", dict(planes=planes.at(cell_bytes))), ("a pitch that is no multiple of a quad", dict(pitch=pitch - 1)),
                 ("a pitch_src that is no multiple of 4", dict(pitch_src=22)), ("a pitch_src below Ls", dict(pitch_src=20)),
                 ("cells that leave the pitch", dict(cell0=32)), ("a cell0 that is no multiple of 8", dict(cell0=4)), ("cell0 below 0", dict(cell0=-8)),
                 ("Ls below 0", dict(Ls=-1)), ("cell_bytes 3", dict(cell_bytes=3)), ("the other cell's span in 2 bytes", dict(cell_bytes=2, kmin=1, kmax=65536)),
                 ("kmin = 0", dict(kmin=0)), ("kmin above kmax", dict(kmin=9, kmax=8)), ("kmax past 2^31 - 1", dict(kmax=2 ** 31)),
                 ("an entry = num_docs", dict(genomes=[3, N, 0])), ("n_list below 0", dict(n=-1)), ("n_list above the bound", dict(n=65536)),
                 ("num_docs = 0", dict(N=0)), ("num_docs above the bound", dict(N=2049))]
        for what, over in cases:
            b = dict(a, **over)
            with pytest.raises(MemoError) as err:
                weights_call(b["lengths"], b["Ls"], b["pitch_src"], b["N"], b["kmin"], b["kmax"], b["genomes"], b["planes"], b["pitch"], b["cell_bytes"], b["cell0"], b["n"])
            assert err.value.code == MEMO_EINVAL, what
            assert (planes.to_host(filled.shape, dtype) == S).all(), what
        for over in (dict(Ls=0, cell0=pitch), dict(genomes=[])):                  # nothing to write launches nothing, at the very end of the pitch too
            b = dict(a, **over)
            weights_call(b["lengths"], b["Ls"], b["pitch_src"], b["N"], b["kmin"], b["kmax"], b["genomes"], b["planes"], b["pitch"], b["cell_bytes"], b["cell0"])
            assert (planes.to_host(filled.shape, dtype) == S).all()
        weights_call(lengths.d, Ls, pitch_src, N, kmin, kmax, good, planes.d, pitch, cell_bytes, 8)          # and the same call with nothing to refuse
        got = planes.to_host(filled.shape, dtype)
        assert np.array_equal(got[:, 8:8 + Ls].astype(np.int64), want_weights(src[good, :Ls], kmin, kmax))


# ---------------------------------------------------------------------------------------
# end to end: the window route against the tables and against `memo panel`
# ---------------------------------------------------------------------------------------
def region_rows(result, L, span):
    order, core, covered = result[:3]
    assert result[3:] == (L, span)
    assert order.dtype == np.uint16 and core.dtype == np.uint64 and covered.dtype == np.uint64 and order.shape == core.shape == covered.shape
    return list(zip(order.tolist(), core.tolist(), covered.tolist()))


def span_of(kw):
    return kw.get("kmax", CAP_MAX) - kw.get("kmin", 1) + 1


@pytest.mark.parametrize("at", range(len(T.EXAMPLE)))
def test_region_cover_on_the_example(memo, at):
    from memo_amd import cover
    kw, total, want = T.EXAMPLE[at]
    span = span_of(kw)
    assert total == 20 * span
    assert region_rows(cover.region_cover(EXAMPLE_INDEX, "ref_1:0-20", 5, **kw), 20, span) == want
    assert region_rows(cover.region_cover(EXAMPLE_INDEX, "ref_1:0-20", 5, lazy=False, **kw), 20, span) == want
    for step in (8, 64, 2104):
        assert region_rows(cover.region_cover(EXAMPLE_INDEX, "ref_1:0-20", 5, slice_positions=step, **kw), 20, span) == want, step


@pytest.mark.parametrize("at", range(len(T.RND40)))
def test_region_cover_on_rnd_n40(memo, at, monkeypatch):
    from memo_amd import cover, panel
    kw, begins, first, last = T.RND40[at]
    span = span_of(kw)
    rows = region_rows(cover.region_cover(RND40_INDEX, "chr1:0-2100", 40, **kw), 2100, span)
    assert len(rows) == 39 and [r[0] for r in rows[:12]] == begins and rows[:len(first)] == first and rows[-1] == last
    assert cover.planes_scored() <= 40 * 39 // 2
    monkeypatch.setattr(panel, "LAZY_BYTES", 0)          # planes this short go in one call a step: here a step's first call takes 8
    assert region_rows(cover.region_cover(RND40_INDEX, "chr1:0-2100", 40, **kw), 2100, span) == rows
    lazy_scored = cover.planes_scored()
    assert lazy_scored < 40 * 39 // 2
    eager = cover.region_cover(RND40_INDEX, "chr1:0-2100", 40, lazy=False, **kw)
    assert region_rows(eager, 2100, span) == rows and lazy_scored <= cover.planes_scored() == 40 * 39 // 2
    for step in (8, 64, 2104):
        assert region_rows(cover.region_cover(RND40_INDEX, "chr1:0-2100", 40, slice_positions=step, **kw), 2100, span) == rows, step


@pytest.mark.parametrize("at", range(len(T.RND40_STOPS)))
def test_region_cover_stops(memo, at):
    from memo_amd import cover
    kw, want = T.RND40_STOPS[at]
    rows = region_rows(cover.region_cover(RND40_INDEX, "chr1:0-2100", 40, **kw), 2100, 64)
    assert len(rows) == want and 2100 * 64 == 134400
    assert rows == region_rows(cover.region_cover(RND40_INDEX, "chr1:0-2100", 40, slice_positions=64, lazy=False, **kw), 2100, 64)


def test_one_k_is_memo_panel(memo):
    """product against product: -l k -K k is `memo panel -k k`, number for number"""
    from memo_amd import cover, panel
    for index, region, n in ((EXAMPLE_INDEX, "ref_1:0-20", 5), (RND40_INDEX, "chr1:0-2100", 40), (RND40_INDEX, "chr1:33-1058", 40)):
        for k in (3, 4, 31):
            for kw in (dict(), dict(objective="core", seeds="2", max_genomes=4)):
                order, core, covered, L = panel.region_panel(index, region, k, n, **kw)
                got = cover.region_cover(index, region, n, kmin=k, kmax=k, **kw)
                assert got[3:] == (L, 1) and all(np.array_equal(a, b) for a, b in zip(got[:3], (order, core, covered))), (region, k, kw)


def test_the_named_genomes_alone_get_a_plane(memo):
    """seeds and candidates off the ends of the genome range, windows off the slice edges, against the oracle on the golden's lengths"""
    from memo_amd import cover
    from tests import cover_oracle as C
    from tests import lengths_oracle
    from tests.test_cover_cpu import oracle_kw
    cols = G.index_columns("rnd_n40.parquet", "chr1")
    for (qs, qe), kw in (((7, 2090), dict(kmax=64, seeds="39,17", candidates="1-30", max_genomes=12)),
                         ((33, 1058), dict(kmin=12, kmax=70000, objective="core", candidates="39,1,20-25", fraction="0.999")),
                         ((100, 101), dict()),
                         ((0, 2100), dict(kmax=31, seeds="7", fraction="0"))):
        kmin, kmax = kw.get("kmin", 1), kw.get("kmax", CAP_MAX)
        W = C.weights(lengths_oracle.planes(*cols, qs, qe, kmax, 40), kmin, kmax)
        want = C.rows(C.greedy(W, kmax - kmin + 1, **oracle_kw(kw)))
        for step in (None, 96):
            got = cover.region_cover(RND40_INDEX, f"chr1:{qs}-{qe}", 40, slice_positions=step, **kw)
            assert region_rows(got, qe - qs, kmax - kmin + 1) == want, ((qs, qe), kw, step)


def test_slices_begin_at_multiples_of_8(memo):
    from memo_amd import cover
    for bad in (12, 4, 0, 2100):
        with pytest.raises(ValueError, match="multiple of 8"):
            cover.region_cover(EXAMPLE_INDEX, "ref_1:0-20", 5, slice_positions=bad)
    with cover.Weights(20, [1, 2], 1, 8) as weights:
        with pytest.raises(ValueError, match="multiple of 8"):
            weights.pack(None, 8, 8, 5, 12)
    with pytest.raises(ValueError):
        cover.region_cover(EXAMPLE_INDEX, "ref_1:20-0", 5)


# ---------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------
def _memo(*argv):
    return subprocess.run([sys.executable, EXE, *argv], capture_output=True, timeout=300, env=dict(os.environ))


def test_cli_writes_the_readme_bytes_and_an_empty_file_for_an_empty_window(memo, tmp_path):
    out = str(tmp_path / "c.tsv")
    common = ("-b", EXAMPLE_INDEX, "-n", "5", "-o", out)
    r = _memo("cover", *common, "-K", "8", "-r", "ref_1:0-20")
    assert (r.returncode, r.stdout) == (0, b"MEMO - cover\n"), r.stderr
    assert open(out).read() == T.README_EXAMPLE
    genomes = tmp_path / "genomes.txt"
    genomes.write_text("ref/pivot.fa\nasm/g1.fa.gz\ng2.fasta\n\ng3.fa\ng4.fna\n")
    r = _memo("cover", *common, "-r", "ref_1:0-20", "-s", "1,2,4", "-g", str(genomes), "-m", "2")
    assert r.returncode == 0, r.stderr
    assert open(out).read() == "genomes\tcore\tcovered\tadded\n1\t42949672940\t0\tpivot\n2\t82\t82\tg2\n3\t61\t85\tg4\n"
    r = _memo("cover", *common, "-l", "3", "-K", "8", "-r", "ref_1:0-20", "-i", "4,1", "-f", "0")
    assert r.returncode == 0 and open(out).read() == "genomes\tcore\tcovered\tadded\n1\t120\t0\t0\n2\t24\t24\t4\n3\t9\t27\t1\n"
    r = _memo("cover", *common, "-r", "ref_1:7-7")
    assert r.returncode == 0 and open(out, "rb").read() == b""
    assert sorted(os.listdir(tmp_path)) == ["c.tsv", "genomes.txt"]                              # written beside its name and renamed
