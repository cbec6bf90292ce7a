"""`memo spectrum` on the GPU: the kernels of memo_amd/csrc/memo_spectrum.hip against the definition in NumPy (tests/spectrum_oracle.py)
on value patterns laid side by side at every shape at which the code takes another path, through the C ABI on padded planes and into
one scratch in several calls, from rows in chunks and slices, against the shipped conservation and membership sweeps on the device,
and the command line against the oracle's text.

Every comparison is exact.  Rows with end < start are compared with the formula only."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import golden_util as G
from tests import spectrum_oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "memo")
PAD = 0xABABABAB
PAD64 = 0xABABABABABABABAB
NS = (1, 2, 5, 33, 64, 65, 100, 257, 2048)
KMAXS = (1, 2, 31, 255, 256, 1024)
LDS_BYTES, HIST_BYTES, THREADS = 128 * 1024, 72 * 1024, 256      # memo_spectrum.hip: kLdsBytes, kHistBytes, kThreads


@pytest.fixture(scope="module")
def memo():
    import memo_amd
    from memo_amd import _lib
    memo_amd.build()                     # make: a no-op when libmemo_amd.so is up to date
    assert _lib.lib().memo_device_count() > 0, "no HIP device: the product has no CPU fallback"
    return memo_amd


# the size rule of memo_spectrum.hip, restated: the tile, the staging, and whether the private table fits beside it
def hist_words(kmax):
    return ((kmax >> 1) + 1) | 1


def rule_tile(kmax, membership):
    if not membership:
        return THREADS
    return next((P for P in (256, 128, 64) if P * hist_words(kmax) * 4 <= HIST_BYTES), 32)


def rule_private(n, kmax, membership):
    staging = rule_tile(kmax, membership) * hist_words(kmax) + THREADS if membership else 0
    return (staging + (n + 1) * (kmax + 1)) * 4 <= LDS_BYTES


class Device:
    """device buffers the test lays out itself"""

    def __init__(self):
        from memo_amd._lib import check, lib
        self.check, self.lib, self.held = check, lib(), []

    def put(self, host):
        host = np.ascontiguousarray(host)
        d = C.c_void_p()
        self.check(self.lib.memo_dev_malloc(0, max(host.nbytes, 16), C.byref(d)))
        self.held.append(d)
        if host.nbytes:
            self.check(self.lib.memo_dev_upload(0, d, host.ctypes.data, host.nbytes, None))
        assert d.value % 16 == 0
        return d.value

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


PATTERNS = 9


def pattern_values(rng, n, L, kmax, shift=0):
    """uint32 [n, L]: column p holds pattern (p + shift) % PATTERNS"""
    v = np.empty((n, L), np.uint32)
    for p in range(L):
        kind = (p + shift) % PATTERNS
        x = int(rng.integers(0, kmax + 1))
        if kind == 0:
            col = np.full(n, kmax)                                   # all at KMAX: the hot cells
        elif kind == 1:
            col = np.zeros(n)                                        # all 0
        elif kind == 2:
            col = np.full(n, (kmax - p // PATTERNS) % (kmax + 1))    # falling by one from one such column to the next
        elif kind == 3:
            col = (np.arange(n) + p) % (kmax + 1)                    # every genome a different value: min(N, KMAX + 1) steps
        elif kind == 4:
            col = rng.choice(np.array([x, int(rng.integers(0, kmax + 1))]), n)      # two values only
        elif kind == 5:                                              # ties across the T boundary: the ranks T - 1, T, T + 1 share a value
            col = np.sort(rng.integers(0, kmax + 1, n))
            t = int(rng.integers(0, n))
            col[max(t - 1, 0):t + 2] = col[t]
        elif kind == 6:
            col = rng.integers(0, kmax + 1, n)                       # random
        elif kind == 7:
            col = rng.integers(0, 2 ** 32, n) >> rng.integers(0, 32, n)      # every bit width: mostly above KMAX, taken as KMAX
        else:
            col = np.full(n, x)                                      # all equal
        v[:, p] = rng.permutation(col).astype(np.uint32)
    return v


def differ(got, want, note):
    assert got.dtype == np.uint64 and got.shape == want.shape, (note, got.shape, want.shape)
    if not np.array_equal(got, want):
        k, v = np.argwhere(got != want)[0]
        raise AssertionError(f"{note}: {(got != want).sum()} of {want.size} counts differ, first at k = {k + 1}, v = {v}: got {got[k, v]}, want {want[k, v]}")


def abi_table(dev, pieces, n, kmax, mode, extra=64):
    """begin, one add per piece (uint32 [n, L_i], each on planes of pitch L_i rounded up to 4, + extra, between poisoned words), finish,
    through the C ABI, scratch and result between poisoned words that must stay as they were"""
    lib = dev.lib
    cells = (n + 1) * (kmax + 1)
    assert lib.memo_spectrum_scratch_bytes(n, kmax) == 8 * cells
    d_scratch = dev.put(np.full(cells + 4, PAD64, np.uint64)) + 16
    d_exact = dev.put(np.full(kmax * (n + 1) + 4, PAD64, np.uint64)) + 16
    dev.check(lib.memo_spectrum_begin_dev(d_scratch, n, kmax, 0, None))
    for piece in pieces:
        L = piece.shape[1]
        pitch = ((L + 3) & ~3) + extra
        whole = np.full((n, pitch), PAD, np.uint32)
        whole[:, :L] = piece
        d_cells = dev.put(np.concatenate([np.full(4, PAD, np.uint32), whole.reshape(-1), np.full(4, PAD, np.uint32)])) + 16
        dev.check(lib.memo_spectrum_add_dev(d_cells, L, pitch, n, kmax, mode, d_scratch, 0, None))
    dev.check(lib.memo_spectrum_finish_dev(d_scratch, n, kmax, d_exact, 0, None))
    scratch = dev.get(d_scratch - 16, cells + 4, np.uint64)
    got = dev.get(d_exact - 16, kmax * (n + 1) + 4, np.uint64)
    dev.close()
    assert (scratch[[0, 1, -2, -1]] == PAD64).all() and (got[[0, 1, -2, -1]] == PAD64).all(), "words around the scratch or the result were written"
    assert (scratch[2:-2].reshape(kmax + 1, n + 1).sum(axis=0, dtype=np.uint64) == 0).all()      # every run that opens closes
    return got[2:-2].reshape(kmax, n + 1).copy()


# ---------------------------------------------------------------------------------------
# the kernel alone
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
def test_value_patterns_at_every_shape(memo, dev, n):
    from memo_amd import spectrum
    calls = 0
    for kmax in KMAXS:
        for membership in (False, True):
            P = spectrum.tile(n, kmax, membership)
            assert P == rule_tile(kmax, membership)
            rng = np.random.default_rng([n, kmax, membership])
            longest = 2 * P + 1
            values = pattern_values(rng, n, longest, kmax, shift=kmax)
            cons = spectrum_oracle.cons(values, kmax, membership)          # once: the table of a prefix is a count over its rows
            for L in (0, 1, 2, P - 1, P, P + 1, longest):
                want = spectrum_oracle.count(cons[:L], n)
                assert (want.sum(axis=1) == L).all()
                differ(spectrum.table(values[:, :L], kmax, membership), want, (n, kmax, membership, L))
                calls += 1
            # pitch L + 64 between poisoned words, and the same columns in three adds into one scratch
            differ(abi_table(dev, [values[:, :P + 1]], n, kmax, int(membership)), spectrum_oracle.count(cons[:P + 1], n), (n, kmax, membership, "padded"))
            cuts = [values[:, :1], values[:, 1:P + 2], values[:, P + 2:]]
            differ(abi_table(dev, cuts, n, kmax, int(membership), extra=0), spectrum_oracle.count(cons, n), (n, kmax, membership, "three adds"))
    assert calls == len(KMAXS) * 2 * 7


def test_both_accumulation_paths_run():
    """the documented size rule: the workgroup-private table is taken where its (N + 1)(KMAX + 1) words fit 128 KiB beside the
    staging.  Of the shapes of test_value_patterns_at_every_shape, some lie on each side in each mode, the nearest to the bound too."""
    shapes = [(n, kmax, m) for n in NS for kmax in KMAXS for m in (False, True)]
    for m in (False, True):
        side = {rule_private(n, kmax, m) for n, kmax, mm in shapes if mm == m}
        assert side == {True, False}
    assert rule_private(2048, 1, True) and rule_private(2048, 2, True) and not rule_private(2048, 31, False)
    # by hand: KMAX = 255 with -m stages 128 rows of 129 words and 256 partial sums, 67 072 bytes; 34 x 256 words of table fit beside
    # them (101 888 bytes), 65 x 256 do not (133 632)
    assert rule_private(33, 255, True) and not rule_private(64, 255, True)
    assert rule_private(5, 1024, True) and not rule_private(33, 1024, False) and rule_private(100, 256, False) and not rule_private(257, 256, False)
    assert [rule_tile(k, True) for k in KMAXS] == [256, 256, 256, 128, 128, 32]


def test_the_library_says_which_path_it_took(memo):
    """memo_debug_spectrum_times of the A/B library: the path of the last add is the size rule's, and the atomics it counts are few"""
    from memo_amd import _lib, spectrum
    L_ = _lib.use_ab(True)
    try:
        path, atomics, ms = C.c_int32(-7), C.c_uint64(0), (C.c_float * 2)()
        assert L_.memo_debug_spectrum_times(3, None, None, None) == 0
        for n, kmax, membership in ((5, 31, False), (5, 31, True), (2048, 31, False), (257, 255, True), (100, 1024, True), (5, 1024, True)):
            P = spectrum.tile(n, kmax, membership)
            planes = np.full((n, 2 * P + 1), kmax, np.uint32)                 # a conserved stretch: one run per position
            got = spectrum.table(planes, kmax, membership)
            assert (got[:, n] == 2 * P + 1).all() and got[:, :n].sum() == 0
            assert L_.memo_debug_spectrum_times(3, ms, C.byref(path), C.byref(atomics)) == 0
            assert path.value == int(rule_private(n, kmax, membership)), (n, kmax, membership)
            # two cells take every update, in three tiles: a workgroup's flush is one atomic a cell, and so is a wave's merged update
            assert 2 <= atomics.value <= 2 * 3 * (1 if path.value else THREADS // 64), (n, kmax, membership, atomics.value)
            assert ms[0] > 0 and ms[1] > 0
    finally:
        L_.memo_debug_spectrum_times(0, None, None, None)
        _lib.use_ab(False)


def test_a_fresh_begin_forgets_and_refusals_change_nothing(dev):
    from memo_amd._lib import MEMO_EINVAL
    lib, n, kmax, L, pitch = dev.lib, 3, 6, 16, 20
    rng = np.random.default_rng(5)
    first, second = rng.integers(0, 9, (n, L)).astype(np.uint32), rng.integers(0, 9, (n, L)).astype(np.uint32)

    def planes(v):
        whole = np.full((n, pitch), PAD, np.uint32)
        whole[:, :L] = v
        return dev.put(whole)
    cells = (n + 1) * (kmax + 1)
    d_scratch, d_exact = dev.put(np.full(cells, PAD64, np.uint64)), dev.put(np.full(kmax * (n + 1), PAD64, np.uint64))
    d_first, d_second = planes(first), planes(second)
    for mode in (0, 1):
        dev.check(lib.memo_spectrum_begin_dev(d_scratch, n, kmax, 0, None))
        dev.check(lib.memo_spectrum_add_dev(d_first, L, pitch, n, kmax, mode, d_scratch, 0, None))
        dev.check(lib.memo_spectrum_begin_dev(d_scratch, n, kmax, 0, None))                      # forgets the first
        dev.check(lib.memo_spectrum_add_dev(d_second, L, pitch, n, kmax, mode, d_scratch, 0, None))
        dev.check(lib.memo_spectrum_finish_dev(d_scratch, n, kmax, d_exact, 0, None))
        differ(dev.get(d_exact, kmax * (n + 1), np.uint64).reshape(kmax, n + 1), spectrum_oracle.table(second, kmax, bool(mode)), ("fresh begin", mode))
        dev.check(lib.memo_spectrum_add_dev(d_first, L, pitch, n, kmax, mode, d_scratch, 0, None))  # finish leaves the scratch: more adds may follow
        dev.check(lib.memo_spectrum_finish_dev(d_scratch, n, kmax, d_exact, 0, None))
        differ(dev.get(d_exact, kmax * (n + 1), np.uint64).reshape(kmax, n + 1), spectrum_oracle.table(np.concatenate([second, first], axis=1), kmax, bool(mode)),
               ("an add after finish", mode))
    scratch_was, exact_was = dev.get(d_scratch, cells, np.uint64), dev.get(d_exact, kmax * (n + 1), np.uint64)
    begin = [d_scratch, n, kmax, 0, None]
    add = [d_first, L, pitch, n, kmax, 1, d_scratch, 0, None]          # cells, L, pitch, N, KMAX, mode, scratch
    fin = [d_scratch, n, kmax, d_exact, 0, None]

    def refused(call, args, at, value, *words):
        args = list(args)
        args[at] = value
        rc = call(*args)
        msg = lib.memo_last_error().decode()
        assert rc == MEMO_EINVAL and all(w in msg for w in words), (at, value, rc, msg)
    for call, args, at_n, at_k, at_s in ((lib.memo_spectrum_begin_dev, begin, 1, 2, 0), (lib.memo_spectrum_add_dev, add, 3, 4, 6), (lib.memo_spectrum_finish_dev, fin, 1, 2, 0)):
        for bad in (0, -1, 2049):
            refused(call, args, at_n, bad, "num_docs")
        for bad in (0, -1, 1025):
            refused(call, args, at_k, bad, "kmax")
        for bad in (d_scratch + 4, d_scratch + 1, None):
            refused(call, args, at_s, bad, "d_scratch")
    for bad in (2, -1, 7):
        refused(lib.memo_spectrum_add_dev, add, 5, bad, "mode")
    for bad in (2 ** 31 + 1, 2 ** 40, -1):
        refused(lib.memo_spectrum_add_dev, add, 1, bad, "2^31")
    for bad in (L - 1, 12, 18, 22, 0):
        refused(lib.memo_spectrum_add_dev, add, 2, bad, "pitch")
    refused(lib.memo_spectrum_add_dev, add, 2, 2 ** 31, "2^32")      # 3 planes of 2^31 cells
    huge = list(add)
    huge[1:4] = [2 ** 21, 2 ** 21, 2048]                             # N pitch = 2^32 exactly
    refused(lib.memo_spectrum_add_dev, huge, 0, d_first, "2^32")
    for off in (4, 8, 12):
        refused(lib.memo_spectrum_add_dev, add, 0, d_first + off, "16-byte aligned")
    refused(lib.memo_spectrum_add_dev, add, 0, None, "NULL")
    for bad in (d_exact + 4, d_exact + 2, None):
        refused(lib.memo_spectrum_finish_dev, fin, 3, bad, "d_exact")
    # L == 0: nothing to do, nothing launched, NULL cells are fine
    assert lib.memo_spectrum_add_dev(None, 0, 0, n, kmax, 0, d_scratch, 0, None) == 0 and lib.memo_spectrum_add_dev(d_first, 0, pitch, n, kmax, 1, d_scratch, 0, None) == 0
    assert np.array_equal(dev.get(d_scratch, cells, np.uint64), scratch_was) and np.array_equal(dev.get(d_exact, kmax * (n + 1), np.uint64), exact_was)
    assert [lib.memo_spectrum_tile(*bad) for bad in ((0, 5, 0), (2049, 5, 1), (5, 0, 0), (5, 1025, 1), (5, 5, 2), (5, 5, -1))] == [0] * 6
    assert [lib.memo_spectrum_scratch_bytes(*bad) for bad in ((0, 5), (2049, 5), (5, 0), (5, 1025))] == [0] * 4
    assert lib.memo_spectrum_scratch_bytes(2048, 1024) == 8 * 2049 * 1025
    from memo_amd import spectrum
    assert spectrum.table(np.zeros((3, 0), np.uint32), 4, True).tolist() == [[0] * 4] * 4
    with pytest.raises(ValueError):
        spectrum.table(np.zeros((3, 4), np.uint32), 1025, True)
    with pytest.raises(ValueError):
        spectrum.exact([], [], [], 10, 0, 3, kmax=5, membership=False)


# ---------------------------------------------------------------------------------------
# from rows
# ---------------------------------------------------------------------------------------
def cols(rows):
    arr = np.asarray(rows, np.int64).reshape(-1, 3)
    return arr[:, 0].copy(), arr[:, 1].copy(), arr[:, 2].copy()


def random_rows(rng, qs, qe, kmax, m, annots, overlap=300):
    s = np.sort(rng.integers(qs - 10, qe + min(kmax, 60) + 10, m))
    return s, s + rng.integers(0, overlap, m), rng.choice(np.asarray(annots, np.int64), m)


@pytest.mark.parametrize("membership", (False, True))
def test_from_rows_in_chunks_and_slices(memo, membership):
    from memo_amd import spectrum
    n, kmax = 5, 40
    P = spectrum.tile(n, kmax, membership)
    for qs in (1000, 2 ** 32 + 5):
        L = 2 * P + 3
        qe = qs + L
        rng = np.random.default_rng([int(membership), qs % 1000])
        odd = (-1, n, 2 ** 40)
        cases = [("no rows", cols([])),
                 ("rows of no genome", cols([(qs + 1, qs + 1, a) for a in odd])),
                 ("nested: a later start has a smaller end", cols([(qs + 2, qs + 50, 0), (qs + 10, qs + 12, 0), (qs + 11, qs + 40, n - 1), (qs + 11, qs + 13, 2)])),
                 ("one row per genome at the edges", cols([(s, s + 2 + g, g) for g in range(n) for s in (qs, qs + 1, qe - 1, qe, qe + kmax - 1, qe + kmax)]))]
        for back in (1, 2, 400):                                      # rows with end < start: the formula, literally
            s, _, a = random_rows(rng, qs, qe, kmax, 60, tuple(range(n)) + odd)
            cases.append((f"e = s - {back}", (s, s - back, a)))
        rnd = random_rows(rng, qs, qe, kmax, 4 * L, tuple(range(n)) + odd)
        cases.append(("random sorted rows", rnd))
        for name, rows in cases:
            want = spectrum_oracle.exact(*rows, qs, qe, n, kmax, membership)
            differ(spectrum.exact(*rows, qs, qe, n, kmax=kmax, membership=membership), want, (qs, name))
        want = spectrum_oracle.exact(*rnd, qs, qe, n, kmax, membership)
        assert len(np.unique(want)) > 5 and (want[:, 1:n].sum(axis=1) > 0).any()          # (the rows do bound the window)
        order = rng.permutation(len(rnd[0]))
        shuffled = tuple(c[order] for c in rnd)
        for calls in (1, 2, 7):
            differ(spectrum.exact(*shuffled, qs, qe, n, kmax=kmax, membership=membership, chunk_rows=-(-len(order) // calls)), want, (qs, "shuffled", calls))
        for step in (1, 7, 64, P + 1):
            if step == 1 and qs != 1000:
                continue                                              # (slices of one position: once)
            differ(spectrum.exact(*shuffled, qs, qe, n, kmax=kmax, membership=membership, slice_positions=step, chunk_rows=len(order) // 3 + 1), want, (qs, "slices of", step))


# ---------------------------------------------------------------------------------------
# the shipped sweeps on the device: exact[k] is the bincount of the conservation query, and of the membership query's one-bit counts
# ---------------------------------------------------------------------------------------
KS = (2, 31, 64, 65, 257)
KMAX = 300
LEGAL = sorted({c["index"] for c in G.cases(raises=False)} - {"rnd_negoverlap.parquet"})          # every row has end >= start


@pytest.mark.parametrize("index", LEGAL)
def test_the_sweeps_agree_on_every_golden_window(memo, index):
    from memo_amd import spectrum
    from memo_amd.index import DeviceIndex, bits_to_matrix
    windows = sorted({(c["region"], c["n"], c["membership"]) for c in G.cases(raises=False) if c["index"] == index})
    assert windows
    resident = {}
    try:
        for region, n, membership in windows:
            rec, se = region.split(":")
            qs, qe = map(int, se.split("-"))
            s, e, a = G.index_columns(index, rec)
            assert (e >= s).all()
            got = spectrum.exact(s, e, a, qs, qe, n, kmax=KMAX, membership=membership)
            assert got.shape == (KMAX, n + 1) and (got.sum(axis=1) == qe - qs).all()
            if not len(s):
                assert (got[:, n] == qe - qs).all()                    # no rows: every k-mer is shared at every k
                continue
            if rec not in resident:
                resident[rec] = DeviceIndex.from_host(s, e, a)
            ix = resident[rec]
            for k in KS:
                if membership:
                    held = bits_to_matrix(ix.membership(qs, qe, k, n), n).astype(np.int64).sum(axis=1)
                else:
                    held = ix.conservation(qs, qe, k, n).astype(np.int64)
                assert np.array_equal(got[k - 1], np.bincount(held, minlength=n + 1)), (index, region, membership, k)
    finally:
        for ix in resident.values():
            ix.close()


def test_every_legal_golden_window_is_covered():
    assert len(LEGAL) == 7 and sum(len({(c["region"], c["n"], c["membership"]) for c in G.cases(raises=False) if c["index"] == i}) for i in LEGAL) == 164


# ---------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------
def _memo(*argv, env=None):
    return subprocess.run([sys.executable, EXE, *argv], capture_output=True, timeout=300, env=dict(os.environ, **(env or {})))


@pytest.mark.parametrize("name", ("example_cons.parquet", "example_memb.parquet"))
def test_cli_on_the_example_indexes(memo, tmp_path, name):
    out = str(tmp_path / "s.tsv")
    membership = name == "example_memb.parquet"
    flags = ("-m",) if membership else ()
    index = os.path.join(G.GOLD, name)
    s, e, a = G.index_columns(name, "ref_1")
    r = _memo("spectrum", "-b", index, "-n", "5", "-r", "ref_1:0-26", "-o", out, *flags)
    assert (r.returncode, r.stdout) == (0, b"MEMO - spectrum\n"), r.stderr
    want = spectrum_oracle.exact(s, e, a, 0, 26, 5, 128, membership)                           # -K defaults to 128
    assert open(out, "rb").read() == spectrum_oracle.text(want) and len(np.unique(want)) > 4
    # -K and a window forced into slices of 7 positions
    short = spectrum_oracle.exact(s, e, a, 3, 30, 5, 7, membership)
    assert _memo("spectrum", "-b", index, "-n", "5", "-r", "ref_1:3-30", "-o", out, "-K", "7", *flags, env={"MEMO_LENGTHS_SLICE": "7"}).returncode == 0
    assert open(out, "rb").read() == spectrum_oracle.text(short) and open(out, "rb").read().count(b"\n") == 8
    assert _memo("spectrum", "-b", index, "-n", "5", "-r", "ref_1:5-5", "-o", out, *flags).returncode == 0
    assert open(out, "rb").read() == b""                                                      # an empty window: an empty file
    # -c, and the README's numbers
    assert _memo("spectrum", "-b", index, "-n", "5", "-r", "ref_1:0-20", "-o", out, "-c", "-K", "4", *flags).returncode == 0
    assert open(out, "rb").read() == spectrum_oracle.text(spectrum_oracle.exact(s, e, a, 0, 20, 5, 4, membership), cumulative=True)
    lines = [ln.split("\t") for ln in open(out).read().splitlines()]
    assert lines[0] == ["k", "1", "2", "3", "4", "5"] and [ln[0] for ln in lines[1:]] == ["1", "2", "3", "4"]
    assert (lines[3][5], lines[3][3], lines[4][3], lines[4][5]) == ("8", "20", "12", "1")
    assert sorted(os.listdir(tmp_path)) == ["s.tsv"]                                          # written beside its name and renamed
    if not membership:
        return
    # column N of -c at k = 3 is the core `memo collect` ends with
    collected = str(tmp_path / "c.tsv")
    assert _memo("collect", "-b", index, "-k", "3", "-n", "5", "-r", "ref_1:0-20", "-o", collected).returncode == 0
    assert open(collected).read().splitlines()[-1].split("\t")[1] == lines[3][5] == "8"
    os.unlink(collected)
    never = str(tmp_path / "never.tsv")
    r = _memo("spectrum", "-b", index, "-n", "5", "-r", "ref_1:20-0", "-o", never, "-m")
    assert r.returncode == 1 and b"negative dimensions" in r.stderr and not os.path.exists(never)
    r = _memo("spectrum", "-b", str(tmp_path / "no.parquet"), "-n", "5", "-r", "ref_1:0-26", "-o", never, env={"MEMO_LENGTHS_SLICE": "7"})
    assert r.returncode == 1 and r.stderr.startswith(b"memo spectrum: ") and sorted(os.listdir(tmp_path)) == ["s.tsv"]
