"""`memo panel` on the GPU: the kernels of memo_amd/csrc/memo_panel.hip against NumPy on the host -- the planes against np.packbits,
the scores and the take against popcounts of whole words --, the window route against the worked tables (tests/panel_tables.py) and
the oracle (tests/panel_oracle.py), the command line against the README's bytes.  Every comparison is exact."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import golden_util as G
from tests import panel_oracle as P
from tests import panel_tables as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "memo")
SENTINEL = 0xA5C3F00F
EXAMPLE_INDEX, RND40_INDEX = os.path.join(G.GOLD, "example_memb.parquet"), os.path.join(G.GOLD, "rnd_n40.parquet")


@pytest.fixture(scope="module")
def memo():
    import memo_amd
    from memo_amd import _lib
    memo_amd.build()                     # make: a no-op when libmemo_amd.so is up to date
    assert _lib.lib().memo_device_count() > 0, "no HIP device: the product has no CPU fallback"
    return memo_amd


# ---------------------------------------------------------------------------------------
# rows, planes, popcounts on the host
# ---------------------------------------------------------------------------------------
def pack_rows(B, garbage=None):
    """B uint8 [L, N] as membership rows uint32 [L, W]: bit g & 31 of word g >> 5.  garbage: the bits at or above N of the last word"""
    B = np.asarray(B, np.uint8)
    L, N = B.shape
    W = (N + 31) // 32
    full = np.zeros((L, 32 * W), np.uint8)
    full[:, :N] = B
    if garbage is not None:
        full[:, N:] = garbage
    return np.ascontiguousarray(np.packbits(full, axis=1, bitorder="little")).view(np.uint32).reshape(L, W)


def pack_planes(B):
    """B uint8 [L, N] as planes uint32 [N, ceil(L / 32)]: bit p & 31 of word p >> 5 of plane g, zeros at and past L"""
    B = np.asarray(B, np.uint8)
    L, N = B.shape
    nw = (L + 31) // 32
    full = np.zeros((N, 32 * nw), np.uint8)
    full[:, :L] = B.T
    return np.ascontiguousarray(np.packbits(full, axis=1, bitorder="little")).view(np.uint32).reshape(N, nw)


def popcount(words):
    return int(np.unpackbits(np.ascontiguousarray(words, np.uint32).view(np.uint8)).sum())


def random_bits(L, N, density, seed=0):
    return (np.random.default_rng([seed, L, N]).random((L, N)) < density).astype(np.uint8)


def planes_call(d_bits, L, N, d_planes, pitch, word0):
    from memo_amd._lib import check, lib
    check(lib().memo_panel_planes_dev(d_bits, L, N, d_planes, pitch, word0, 0, None))


# ---------------------------------------------------------------------------------------
# memo_panel_planes_dev against np.packbits
# ---------------------------------------------------------------------------------------
def test_the_tile_and_the_pass(memo):
    from memo_amd import panel
    assert panel.tile() == 1024 and panel.pass_words() == 1024


@pytest.mark.parametrize("num_docs", (2, 5, 32, 33, 64, 65, 200))
def test_planes_equal_packbits_at_every_length_and_offset(memo, num_docs):
    """the slice's words of every plane are np.packbits of the column, the tail of the last word zeros; every other word of a
    sentinel-filled buffer with a pitch wider than needed, and the plane behind the last, stay the sentinel.  The rows lie between
    words of all ones and carry ones at and above num_docs: neither reaches a plane."""
    from memo_amd import panel
    from memo_amd._device import DevBuffer
    N, tile = num_docs, panel.tile()
    W = (N + 31) // 32
    lengths = (1, 31, 32, 33, 127, 128, 129, tile - 1, tile, tile + 1, 3 * tile + 5)
    B = random_bits(lengths[-1], N, 0.5, seed=1)
    dirty = pack_rows(B, garbage=1)
    assert N % 32 == 0 or not np.array_equal(dirty, pack_rows(B))
    ones = np.full(16, 0xFFFFFFFF, np.uint32)
    for L in lengths:
        nw = (L + 31) // 32
        want = pack_planes(B[:L])
        host = np.concatenate([ones, dirty[:L].reshape(-1), np.full(64 * W + 16, 0xFFFFFFFF, np.uint32)])
        with DevBuffer.of(host, 0) as rows:
            for word0 in (0, 1, 5):
                pitch = (word0 + nw + 3) // 4 * 4 + 8
                filled = np.full((N + 1, pitch), SENTINEL, np.uint32)
                with DevBuffer.of(filled, 0) as planes:
                    planes_call(rows.at(64), L, N, planes.d, pitch, word0)
                    got = planes.to_host(filled.shape, np.uint32)
                assert np.array_equal(got[:N, word0:word0 + nw], want), (N, L, word0)
                got[:N, word0:word0 + nw] = SENTINEL
                assert (got == SENTINEL).all(), (N, L, word0)
                if L % 32:
                    assert int(want[:, -1].max()) < 1 << (L % 32)


def test_planes_of_slices_laid_end_to_end(memo):
    """three slices of one window, packed out of order into one buffer, are the window's planes"""
    from memo_amd import panel
    from memo_amd._device import DevBuffer
    N, L = 70, 2 * panel.tile() + 32 * 7 + 13
    B = random_bits(L, N, 0.3, seed=2)
    want = pack_planes(B)
    pitch = (want.shape[1] + 3) // 4 * 4
    cuts = [0, 32 * 5, panel.tile() + 32, L]
    with DevBuffer.of(np.full((N, pitch), SENTINEL, np.uint32), 0) as planes:
        for a, b in reversed(list(zip(cuts, cuts[1:]))):
            with DevBuffer.of(pack_rows(B[a:b]), 0) as rows:
                planes_call(rows.d, b - a, N, planes.d, pitch, a // 32)
        got = planes.to_host((N, pitch), np.uint32)
    assert np.array_equal(got[:, :want.shape[1]], want) and (got[:, want.shape[1]:] == SENTINEL).all()


def test_planes_refusals_leave_the_planes_unchanged(memo):
    from memo_amd._device import DevBuffer
    from memo_amd._lib import MEMO_EINVAL, MemoError
    N, L, pitch = 40, 100, 8
    rows = pack_rows(random_bits(L, N, 0.5, seed=3))
    filled = np.full((N, pitch), SENTINEL, np.uint32)
    with DevBuffer.of(rows, 0) as d_rows, DevBuffer.of(filled, 0) as planes:
        assert d_rows.d.value % 16 == 0 and planes.d.value % 16 == 0
        for what, args in (("rows not 16-byte aligned", (d_rows.at(4), L, N, planes.d, pitch, 0)),
                           ("planes not 16-byte aligned", (d_rows.d, L, N, planes.at(4), pitch, 0)),
                           ("planes NULL", (d_rows.d, L, N, None, pitch, 0)),
                           ("a pitch that is no multiple of 4", (d_rows.d, L, N, planes.d, 6, 0)),
                           ("a pitch of 0", (d_rows.d, L, N, planes.d, 0, 0)),
                           ("word0 below 0", (d_rows.d, L, N, planes.d, pitch, -1)),
                           ("words that leave the pitch", (d_rows.d, L, N, planes.d, pitch, 5)),
                           ("L below 0", (d_rows.d, -1, N, planes.d, pitch, 0)),
                           ("N = 0", (d_rows.d, L, 0, planes.d, pitch, 0)),
                           ("N above the bound", (d_rows.d, L, 2049, planes.d, pitch, 0))):
            with pytest.raises(MemoError) as err:
                planes_call(*args)
            assert err.value.code == MEMO_EINVAL, what
            assert (planes.to_host(filled.shape, np.uint32) == SENTINEL).all(), what
        planes_call(d_rows.d, 0, N, planes.d, pitch, 8)                       # L = 0 launches nothing, at the very end of the pitch too
        assert (planes.to_host(filled.shape, np.uint32) == SENTINEL).all()
        planes_call(d_rows.d, L, N, planes.d, pitch, 4)                       # and the same call with nothing to refuse
        assert not (planes.to_host(filled.shape, np.uint32) == SENTINEL).all()


# ---------------------------------------------------------------------------------------
# memo_panel_begin_dev, memo_panel_score_dev and memo_panel_take_dev against NumPy
# ---------------------------------------------------------------------------------------
class Masks:
    """random planes of N genomes over nw words and two random masks, on the host and on the device: the pad words up to the next
    multiple of 4 hold zeros, the words between there and the pitch ones, which nothing may count"""

    def __init__(self, N, nw, seed, extra=8):
        from memo_amd._device import DevBuffer
        rng = np.random.default_rng([seed, N, nw])
        self.N, self.nw, self.words = N, nw, (nw + 3) // 4 * 4
        self.pitch = self.words + extra
        self.planes = np.full((N, self.pitch), 0xFFFFFFFF, np.uint32)
        self.planes[:, :self.words] = 0
        self.planes[:, :nw] = rng.integers(0, 2 ** 32, (N, nw), dtype=np.uint32)
        self.core, self.covered = np.zeros(self.words, np.uint32), np.zeros(self.words, np.uint32)
        self.core[:nw] = rng.integers(0, 2 ** 32, nw, dtype=np.uint32) | rng.integers(0, 2 ** 32, nw, dtype=np.uint32)
        self.covered[:nw] = rng.integers(0, 2 ** 32, nw, dtype=np.uint32) & rng.integers(0, 2 ** 32, nw, dtype=np.uint32)
        self.d_planes, self.d_core, self.d_covered = (DevBuffer.of(a, 0) for a in (self.planes, self.core, self.covered))

    def score(self, genomes, out=None, **over):
        from memo_amd._lib import check, lib
        ids = np.ascontiguousarray(genomes, np.uint16)
        out = np.zeros((len(ids), 2), np.uint64) if out is None else out
        a = dict(planes=self.d_planes.d, pitch=self.pitch, N=self.N, words=self.words, core=self.d_core.d, covered=self.d_covered.d, n=len(ids))
        a.update(over)
        check(lib().memo_panel_score_dev(a["planes"], a["pitch"], a["N"], a["words"], a["core"], a["covered"], ids.ctypes.data, a["n"], out.ctypes.data, 0, None))
        return out

    def take(self, genome, out=None, **over):
        from memo_amd._lib import check, lib
        out = np.zeros(2, np.uint64) if out is None else out
        a = dict(planes=self.d_planes.d, pitch=self.pitch, N=self.N, words=self.words, core=self.d_core.d, covered=self.d_covered.d)
        a.update(over)
        check(lib().memo_panel_take_dev(a["planes"], a["pitch"], a["N"], a["words"], genome, a["core"], a["covered"], out.ctypes.data, 0, None))
        return out

    def want_scores(self, genomes):
        p = self.planes[np.asarray(genomes, np.int64), :self.words]
        return [[popcount(row & ~self.covered), popcount(row & self.core)] for row in p]

    def device_masks(self):
        return self.d_core.to_host(self.core.shape, np.uint32), self.d_covered.to_host(self.covered.shape, np.uint32)

    def close(self):
        for b in (self.d_planes, self.d_core, self.d_covered):
            b.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def word_counts():
    from memo_amd import panel
    per = panel.pass_words()
    return (1, 3, 4, 5, per - 1, per, per + 1, 3 * per + 7)


LISTS = ([11], [3, 1, 4, 15, 9, 2, 6], [5, 3, 18, 9, 7, 1, 12, 0], [19, 8, 7, 6, 5, 4, 3, 2, 1], list(range(17)), [4, 9, 4, 4, 0, 9, 19, 4, 9, 4])


def test_scores_equal_popcounts(memo):
    """lists of 1, 7, 8, 9 and 17 genomes and one with repeats (a block of the kernel is 8), at 1, 3, 4 and 5 words, one word below
    and above a workgroup's pass, and several workgroups along the words; the masks stay as they were"""
    N = 20
    for nw in word_counts():
        with Masks(N, nw, seed=4) as m:
            for genomes in LISTS:
                got = m.score(genomes)
                assert got.dtype == np.uint64 and got.tolist() == m.want_scores(genomes), (nw, genomes)
            core, covered = m.device_masks()
            assert np.array_equal(core, m.core) and np.array_equal(covered, m.covered)
            assert m.score([]).shape == (0, 2)


def test_scores_of_many_genomes_and_extreme_masks(memo):
    from memo_amd import panel
    N, nw = 2048, panel.pass_words() + 9
    with Masks(N, nw, seed=5, extra=0) as m:
        everyone = np.random.default_rng(6).permutation(N)
        assert m.score(everyone).tolist() == m.want_scores(everyone)               # 256 blocks of candidates, the pitch with nothing to spare
    with Masks(3, 700, seed=7) as m:
        from memo_amd._lib import check, lib
        for core, covered in ((0xFFFFFFFF, 0), (0, 0xFFFFFFFF)):
            m.core[:m.nw], m.covered[:m.nw] = core, covered
            for buf, host in ((m.d_core, m.core), (m.d_covered, m.covered)):
                check(lib().memo_dev_upload(0, buf.d, host.ctypes.data, host.nbytes, None))
            own = [popcount(m.planes[g, :m.words]) for g in range(3)]
            assert m.score([0, 1, 2]).tolist() == [[n if core else 0, n if core else 0] for n in own]


def test_take_equals_numpy_step_by_step(memo):
    N = 6
    for nw in word_counts():
        with Masks(N, nw, seed=8) as m:
            core, covered = m.core.copy(), m.covered.copy()
            for g in (3, 0, 5, 3):
                core &= m.planes[g, :m.words]
                covered |= m.planes[g, :m.words]
                got = m.take(g)
                assert got.tolist() == [popcount(core), popcount(covered)], (nw, g)
                now = m.device_masks()
                assert np.array_equal(now[0], core) and np.array_equal(now[1], covered), (nw, g)
                m.core, m.covered = core, covered                                   # ... and the scores against the masks as they are now
                assert m.score([1, 2, 4]).tolist() == m.want_scores([1, 2, 4])
            assert np.array_equal(m.d_planes.to_host(m.planes.shape, np.uint32), m.planes)


def test_begin_writes_the_masks_and_the_pads_alone(memo):
    from memo_amd._device import DevBuffer
    from memo_amd._lib import check, lib
    for N, L in ((5, 1), (5, 31), (5, 32), (70, 33), (70, 127), (3, 128), (3, 129), (2048, 161), (9, 32 * 1024 + 5)):
        nw = (L + 31) // 32
        words = (nw + 3) // 4 * 4
        pitch = words + 4
        filled = np.full((N + 1, pitch), SENTINEL, np.uint32)
        with DevBuffer.of(filled, 0) as planes, DevBuffer.of(np.full(words + 4, SENTINEL, np.uint32), 0) as core, \
                DevBuffer.of(np.full(words + 4, SENTINEL, np.uint32), 0) as covered:
            check(lib().memo_panel_begin_dev(planes.d, pitch, N, L, core.d, covered.d, 0, None))
            got = planes.to_host(filled.shape, np.uint32)
            assert (got[:N, nw:words] == 0).all() and (got[:N, :nw] == SENTINEL).all() and (got[:N, words:] == SENTINEL).all() and (got[N] == SENTINEL).all(), (N, L)
            a, o = core.to_host(words + 4, np.uint32), covered.to_host(words + 4, np.uint32)
            want = pack_planes(np.ones((L, 1), np.uint8))[0]
            assert np.array_equal(a[:nw], want) and (a[nw:words] == 0).all() and (a[words:] == SENTINEL).all(), (N, L)
            assert (o[:words] == 0).all() and (o[words:] == SENTINEL).all(), (N, L)


def test_score_and_take_refusals_leave_everything_unchanged(memo):
    from memo_amd._lib import MEMO_EINVAL, MemoError
    N = 20
    with Masks(N, 9, seed=9) as m:
        assert all(b.d.value % 16 == 0 for b in (m.d_planes, m.d_core, m.d_covered)) and m.words == 12 and m.pitch == 20
        good = [3, 1, 4]
        cases = (("planes not 16-byte aligned", good, dict(planes=m.d_planes.at(4))),
                 ("planes NULL", good, dict(planes=None)),
                 ("a pitch that is no multiple of 4", good, dict(pitch=18)),
                 ("words that are no multiple of 4", good, dict(words=10)),
                 ("words past the pitch", good, dict(words=24)),
                 ("words below 0", good, dict(words=-4)),
                 ("core not 16-byte aligned", good, dict(core=m.d_core.at(4))),
                 ("covered not 16-byte aligned", good, dict(covered=m.d_covered.at(8))),
                 ("covered NULL", good, dict(covered=None)),
                 ("N = 0", good, dict(N=0)),
                 ("N above the bound", good, dict(N=2049)),
                 ("an entry = N", [3, N, 4], dict()),
                 ("n_list below 0", good, dict(n=-1)),
                 ("n_list above the bound", good, dict(n=65536)))
        for what, genomes, over in cases:
            out = np.full((3, 2), 7, np.uint64)
            with pytest.raises(MemoError) as err:
                m.score(genomes, out, **over)
            assert err.value.code == MEMO_EINVAL and (out == 7).all(), what
        for what, genomes, over in cases[:11] + (("genome = N", N, dict()), ("genome below 0", -1, dict())):
            out = np.full(2, 7, np.uint64)
            with pytest.raises(MemoError) as err:
                m.take(genomes[0] if isinstance(genomes, list) else genomes, out, **over)
            assert err.value.code == MEMO_EINVAL and (out == 7).all(), what
            core, covered = m.device_masks()
            assert np.array_equal(core, m.core) and np.array_equal(covered, m.covered), what
        assert np.array_equal(m.d_planes.to_host(m.planes.shape, np.uint32), m.planes)
        assert m.score(good).tolist() == m.want_scores(good)                       # and the same call with nothing to refuse


# ---------------------------------------------------------------------------------------
# end to end: the window route against the tables and the oracle
# ---------------------------------------------------------------------------------------
def region_rows(result):
    order, core, covered, L = result
    assert order.dtype == np.uint16 and core.dtype == np.uint64 and covered.dtype == np.uint64 and order.shape == core.shape == covered.shape
    return list(zip(order.tolist(), core.tolist(), covered.tolist()))


@pytest.mark.parametrize("at", range(len(T.EXAMPLE)))
def test_region_panel_on_the_example(memo, at):
    from memo_amd import panel
    k, kw, want = T.EXAMPLE[at]
    got = panel.region_panel(EXAMPLE_INDEX, "ref_1:0-20", k, 5, **kw)
    assert region_rows(got) == want and got[3] == 20


@pytest.mark.parametrize("at", range(len(T.RND40)))
def test_region_panel_on_rnd_n40(memo, at, monkeypatch):
    from memo_amd import collect, panel
    k, kw, begins, first, last = T.RND40[at]
    got = panel.region_panel(RND40_INDEX, "chr1:0-2100", k, 40, **kw)
    rows = region_rows(got)
    assert len(rows) == 39 and [r[0] for r in rows[:12]] == begins and rows[:len(first)] == first and rows[-1] == last
    assert panel.planes_scored() <= 40 * 39 // 2
    monkeypatch.setattr(panel, "LAZY_BYTES", 0)          # planes this short go in one call a step: here a step's first call takes 8
    assert region_rows(panel.region_panel(RND40_INDEX, "chr1:0-2100", k, 40, **kw)) == rows
    lazy_scored = panel.planes_scored()
    assert lazy_scored < 40 * 39 // 2
    eager = panel.region_panel(RND40_INDEX, "chr1:0-2100", k, 40, lazy=False, **kw)
    assert region_rows(eager) == rows and lazy_scored <= panel.planes_scored() == 40 * 39 // 2
    # feeding the order back to `memo collect` reproduces the two columns
    core, covered = collect.region_curves(RND40_INDEX, "chr1:0-2100", k, 40, got[0][None, :])
    assert np.array_equal(core[0], got[1]) and np.array_equal(covered[0], got[2])
    for step in (32, 64, 2112):
        assert region_rows(panel.region_panel(RND40_INDEX, "chr1:0-2100", k, 40, slice_positions=step, **kw)) == rows, step


@pytest.mark.parametrize("at", range(len(T.RND40_STOPS)))
def test_region_panel_stops(memo, at):
    from memo_amd import panel
    (qs, qe), k, kw, want = T.RND40_STOPS[at]
    rows = region_rows(panel.region_panel(RND40_INDEX, f"chr1:{qs}-{qe}", k, 40, **kw))
    assert (len(rows) == want) if isinstance(want, int) else (rows == want)
    assert rows == region_rows(panel.region_panel(RND40_INDEX, f"chr1:{qs}-{qe}", k, 40, slice_positions=64, lazy=False, **kw))


def test_region_panel_equals_the_oracle_on_windows_off_the_word_edges(memo):
    """windows that begin and end inside words, seeds, candidates and caps together, against the oracle on the goldens' bits"""
    from memo_amd import panel
    from tests.test_panel_cpu import golden_bits, oracle_kw
    for (qs, qe), k, kw in (((7, 2090), 31, dict(seeds="5,17", candidates="1-30", max_genomes=12)),
                            ((33, 1058), 12, dict(objective="core", candidates="39,1,20-25", fraction="0.999")),
                            ((100, 101), 8, dict()),
                            ((0, 2100), 31, dict(seeds="7", fraction="0"))):
        B = golden_bits("rnd_n40.parquet", "chr1", qs, qe, k, 40)
        want = P.rows(P.greedy(B, **oracle_kw(kw)))
        for step in (1 << 24, 96):
            assert region_rows(panel.region_panel(RND40_INDEX, f"chr1:{qs}-{qe}", k, 40, slice_positions=step, **kw)) == want, ((qs, qe), k, kw, step)


def test_region_panel_raises_what_memo_query_raises(memo):
    from memo_amd import panel
    with pytest.raises(ValueError):
        panel.region_panel(EXAMPLE_INDEX, "ref_1:20-0", 3, 5)
    with pytest.raises(IndexError):                      # the sweep's own: an annot outside the result columns
        panel.region_panel(EXAMPLE_INDEX, "ref_1:0-20", 3, 2)


# ---------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------
def _memo(*argv):
    return subprocess.run([sys.executable, EXE, *argv], capture_output=True, timeout=300, env=dict(os.environ))


def test_cli_writes_the_readme_bytes_and_an_empty_file_for_an_empty_window(memo, tmp_path):
    out = str(tmp_path / "p.tsv")
    common = ("-b", EXAMPLE_INDEX, "-n", "5", "-o", out)
    r = _memo("panel", *common, "-k", "3", "-r", "ref_1:0-20")
    assert (r.returncode, r.stdout) == (0, b"MEMO - panel\n"), r.stderr
    assert open(out).read() == T.README_EXAMPLE
    genomes = tmp_path / "genomes.txt"
    genomes.write_text("ref/pivot.fa\nasm/g1.fa.gz\ng2.fasta\n\ng3.fa\ng4.fna\n")
    r = _memo("panel", *common, "-k", "4", "-r", "ref_1:0-20", "-s", "1,2,4", "-g", str(genomes), "-O", "core", "-m", "2")
    assert r.returncode == 0, r.stderr
    assert open(out).read() == "genomes\tcore\tcovered\tadded\n1\t20\t0\tpivot\n2\t12\t12\tg2\n3\t5\t13\tg4\n"
    r = _memo("panel", *common, "-k", "3", "-r", "ref_1:0-20", "-i", "1", "-f", "0.5")
    assert r.returncode == 0 and open(out).read() == "genomes\tcore\tcovered\tadded\n1\t20\t0\t0\n2\t10\t10\t1\n"
    r = _memo("panel", *common, "-k", "3", "-r", "ref_1:7-7")
    assert r.returncode == 0 and open(out, "rb").read() == b""
    assert sorted(os.listdir(tmp_path)) == ["genomes.txt", "p.tsv"]                              # written beside its name and renamed
    never = str(tmp_path / "never.tsv")
    r = _memo("panel", "-b", EXAMPLE_INDEX, "-k", "3", "-n", "2", "-r", "ref_1:0-20", "-o", never)
    assert r.returncode == 1 and b"IndexError" in r.stderr and not os.path.exists(never)
