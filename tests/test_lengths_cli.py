"""`memo lengths` without a GPU: the command line (usage bytes, getopts handling, every refusal before the library is even loaded),
memo_emit_u32_rows against a Python formatter and under the host sanitizers, the definition itself (tests/lengths_oracle.py) against
the restated reference (oracle.memo_oracle.np_membership) on the golden membership windows, the slice-and-carry scheme against the
whole-window definition, and the README example's numbers."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import golden_util as G
from tests import lengths_oracle, maxk_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "memo")
CAP_MAX = 2 ** 31 - 1


def _fixture(name):
    return open(os.path.join(G.GOLD, "cli", name), "rb").read()


def _memo(*argv, env=None):
    """bin/memo with the library pointed at a file that is not there: a call that touched _lib.lib() would end in an ImportError's
    traceback, not in the refusal"""
    env = dict(os.environ, MEMO_AMD_LIB=os.path.join(ROOT, "no", "such", "libmemo_amd.so"), **(env or {}))
    return subprocess.run([sys.executable, EXE, *argv], capture_output=True, timeout=120, env=env)


def test_usage_bytes():
    from memo_amd import lengths_cli
    usage = _fixture("memo_lengths_usage.txt")
    assert usage == lengths_cli.USAGE.encode() and usage.startswith(b"\nMEMO lengths - ") and usage.endswith(b"\n\n")
    for argv in ((), ("-h",)):
        r = _memo("lengths", *argv)
        assert (r.returncode, r.stdout, r.stderr) == (0, usage, b""), argv
    for flag in (b"-b [FILE]", b"-n [INT]", b"-r [CHR:START-END]", b"-o [FILE]", b"-t [INT]", b"  -a  ", b"-K [INT]"):
        assert flag in usage
    assert b"-k " not in usage and b"-m " not in usage and b"-d " not in usage


def test_illegal_option_prints_getopts_message_then_usage():
    usage = _fixture("memo_lengths_usage.txt")
    r = _memo("lengths", "-k", "31")
    assert r.returncode == 0 and r.stdout == usage and r.stderr.endswith(b": illegal option -- k\n")
    r = _memo("lengths", "-m")
    assert r.returncode == 0 and r.stdout == usage and r.stderr.endswith(b": illegal option -- m\n")
    r = _memo("lengths", "-n", "5", "-K")
    assert r.returncode == 0 and r.stdout == usage and r.stderr.endswith(b": option requires an argument -- K\n")


def test_the_reference_sub_commands_print_what_they_printed():
    for argv, fixture in (([], "memo_usage.txt"), (["-h"], "memo_usage.txt"), (["bogus"], "memo_bogus.txt")):
        r = _memo(*argv)
        assert r.returncode == 0 and r.stdout == _fixture(fixture), argv
    assert b"lengths" not in _fixture("memo_usage.txt")       # the reference's text: the sub-command is documented in the README
    assert _memo("maxk").stdout == _fixture("memo_maxk_usage.txt")               # `memo maxk` is as it was


def test_refusals_before_the_library_is_touched(tmp_path):
    """(-b names no file and the library path names none: a refusal that came later would be another message)"""
    out = str(tmp_path / "never.txt")
    common = ("-b", str(tmp_path / "no.parquet"), "-r", "ref_1:0-20", "-o", out)
    for extra, env, message in ((("-n", "5"), {"WORLD_SIZE": "2"}, b"sharded launch"),
                                (("-n", "5"), {"MEMO_FORCE_SHARDED": "1"}, b"sharded launch"),
                                (("-n", "5", "-a", "-t", "3"), None, b"-t cannot be combined with -a"),
                                (("-n", "five"), None, b"invalid literal for int()"),
                                (("-n", "0"), None, b"-n must be in [1, 2048]"),
                                (("-n", "2049"), None, b"-n must be in [1, 2048]"),
                                (("-n", "2049", "-a"), None, b"-n must be in [1, 2048]"),
                                (("-n", "5", "-t", "0"), None, b"-t must be an integer in [1, 5]"),
                                (("-n", "5", "-t", "6"), None, b"-t must be an integer in [1, 5]"),
                                (("-n", "5", "-t", "2.5"), None, b"-t must be an integer in [1, 5]"),
                                (("-n", "5", "-t", "x"), None, b"-t must be an integer in [1, 5]"),
                                (("-n", "5", "-K", "0"), None, b"-K must be an integer in [1, 2147483647]"),
                                (("-n", "5", "-a", "-K", str(2 ** 31)), None, b"-K must be an integer in [1, 2147483647]"),
                                (("-n", "5", "-K", "many"), None, b"-K must be an integer in [1, 2147483647]")):
        r = _memo("lengths", *common, *extra, env=env)
        assert r.returncode == 1 and r.stdout == b"MEMO - lengths\n", (extra, r.stderr)
        assert r.stderr.startswith(b"memo lengths: ") and message in r.stderr and r.stderr.count(b"\n") == 1, (extra, r.stderr)
        assert not os.path.exists(out)
    # the same command with nothing to refuse does reach the library, which is not there
    for extra in (("-n", "5"), ("-n", "2048", "-t", "2048", "-K", str(CAP_MAX)), ("-n", "5", "-a", "-K", "1")):
        r = _memo("lengths", *common, *extra)
        assert r.returncode == 1 and not os.path.exists(out)
        assert b"Traceback" in r.stderr or b"memo lengths: " in r.stderr
        assert b"must be" not in r.stderr and b"cannot be combined" not in r.stderr
    assert os.listdir(tmp_path) == []


def test_missing_flags_are_named():
    r = _memo("lengths", "-b", "x.parquet", "-K", "3")
    assert r.returncode == 2 and r.stdout == b"MEMO - lengths\n" and r.stderr == b"memo lengths: -r, -n, -o required\n"
    r = _memo("lengths", "-r", "ref_1:0-20", "-n", "5", "-o", "x", "-a")
    assert r.returncode == 2 and r.stderr == b"memo lengths: -b required\n"


def test_names_are_exported():
    import memo_amd
    from memo_amd import lengths
    assert memo_amd.lengths is lengths and memo_amd.region_planes is lengths.region_planes and memo_amd.region_kth is lengths.region_kth
    assert all(callable(f) for f in (lengths.planes, lengths.kth, lengths.select, lengths.emit_rows, lengths.region_slices))
    assert lengths.default_slice_positions(100) * 100 * 4 <= 2 ** 31 < (lengths.default_slice_positions(100) + 4) * 100 * 4
    assert lengths.default_slice_positions(2048) % 4 == 0 and lengths.default_slice_positions(1) == 2 ** 29


# ---------------------------------------------------------------------------------------
# memo_emit_u32_rows (host code of the library: no device is touched)
# ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import memo_amd
    from memo_amd import _lib
    memo_amd.build()                     # make: a no-op when libmemo_amd.so is up to date
    return _lib.lib()


def _emit(lib, planes, L, pitch, room=None, guard=16):
    """(bytes needed, the buffer's first `room` bytes, whether the `guard` bytes behind them are untouched)"""
    planes = np.ascontiguousarray(planes, np.uint32)
    n = planes.shape[0]
    need = lib.memo_emit_u32_rows(planes.ctypes.data, L, pitch, n, None, 0)
    room = need if room is None else room
    buf = np.full(room + guard, 0xEE, np.uint8)
    got = lib.memo_emit_u32_rows(planes.ctypes.data, L, pitch, n, buf.ctypes.data, room)
    assert got == need
    return need, buf[:room].tobytes(), bool((buf[room:] == 0xEE).all())


def test_emit_u32_rows_against_a_python_formatter(lib):
    edge = np.array([0, 9, 10, 99, 100, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1], np.uint32)
    assert lengths_oracle.rows_text([[0, 7], [4294967295, 10]]) == b"0 4294967295\n7 10\n"     # (the formatter itself, against a literal)
    for n in (1, 2, 5, 33):
        for L in (0, 1, 2, 63, 64, 65, 129):                      # around the emitter's block of positions
            for pitch in (L, L + 3):
                planes = np.full((n, pitch), 77777, np.uint32)    # (the cells at [L, pitch) are not part of the text)
                planes[:, :L] = edge[(np.arange(n)[:, None] * 3 + np.arange(L)[None, :]) % len(edge)]
                want = lengths_oracle.rows_text(planes[:, :L])
                assert _emit(lib, planes, L, pitch) == (len(want), want, True), (n, L, pitch)
    assert _emit(lib, np.zeros((3, 0), np.uint32), 0, 0)[0] == 0  # an empty window is an empty file, not a lone newline


def test_emit_u32_rows_writes_nothing_when_a_byte_is_missing(lib):
    planes = np.array([[7, 2 ** 32 - 1, 10], [0, 1, 123456]], np.uint32)
    want = lengths_oracle.rows_text(planes)
    need, got, clean = _emit(lib, planes, 3, 3, room=len(want) - 1)
    assert need == len(want) and got == b"\xee" * (len(want) - 1) and clean
    need, got, clean = _emit(lib, planes, 3, 3, room=0)
    assert need == len(want) and clean


THREADED = (100_000, 48)                 # lines, planes: 4.8 * 10^6 integers, more than four threads' worth at 2^20 integers a thread


def _wide(L, n):
    """uint32 [n, L] of every width, the same in the child process"""
    return ((np.arange(n * L, dtype=np.uint64) * 2654435761 % 2 ** 32) >> (np.arange(n * L, dtype=np.uint64) % 32)).astype(np.uint32).reshape(n, L)


def _rows_text_fast(planes):
    return ("\n".join(" ".join(map(str, line)) for line in planes.T.tolist()) + "\n").encode()


def test_emit_u32_rows_threaded_path(lib, monkeypatch):
    """10^5 lines over FOUR threads (the library reads MEMO_EMIT_THREADS per call): the shape is wide enough that the emitter does
    split it -- memo_emit_u32_rows_threads says so, and the test fails if it ever falls back to one thread -- so the per-thread byte
    offsets and a block walk that starts inside a block (25000 is no multiple of 64) are what produce the text"""
    L, n = THREADED
    planes = _wide(L, n)
    want = _rows_text_fast(planes)
    assert _rows_text_fast(planes[:5, :70]) == lengths_oracle.rows_text(planes[:5, :70])      # (the fast formatter is the oracle's)
    monkeypatch.setenv("MEMO_EMIT_THREADS", "4")
    assert lib.memo_emit_u32_rows_threads(L, n) == 4 and (L // 4) % 64
    assert lib.memo_emit_u32_rows_threads(L, 3) == 1 and lib.memo_emit_u32_rows_threads(0, n) == 0      # (too narrow to split; no text)
    assert _emit(lib, planes, L, L) == (len(want), want, True)
    need, got, clean = _emit(lib, planes, L, L, room=len(want) - 1)
    assert need == len(want) and clean and got.count(b"\xee") == len(got)                             # a byte short: no thread writes
    monkeypatch.setenv("MEMO_EMIT_THREADS", "3")                  # uneven parts: the last thread's is shorter
    assert lib.memo_emit_u32_rows_threads(L, n) == 3
    assert _emit(lib, planes, L, L) == (len(want), want, True)
    monkeypatch.setenv("MEMO_EMIT_THREADS", "1")
    assert lib.memo_emit_u32_rows_threads(L, n) == 1
    assert _emit(lib, planes, L, L) == (len(want), want, True)
    monkeypatch.delenv("MEMO_EMIT_THREADS")                       # as the machine decides
    assert 1 <= lib.memo_emit_u32_rows_threads(L, n) <= 5
    from memo_amd import lengths
    assert lengths.emit_rows(planes).tobytes() == want and lengths.emit_rows(planes[:, :0]).tobytes() == b""


EMIT_MAIN = r"""
// memo_emit_u32_rows with heap buffers of exactly the sizes it is told: a write past `cap`, or a read past the last plane's [0, L), is the sanitizer's
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include "memo_amd_dap.h"
static uint32_t value(int64_t g, int64_t p) { return (uint32_t)((uint64_t)(g * 1000003 + p) * 2654435761u) >> ((g + p) % 32); }
static int check(int64_t L, int64_t pitch, int32_t n) {
    const size_t cells = n > 0 ? (size_t)(n - 1) * pitch + L : 0;        // exactly up to the last plane's cell L - 1
    uint32_t *planes = (uint32_t *)malloc(cells ? cells * 4 : 1);
    for (size_t i = 0; i < cells; ++i) planes[i] = 4000000000u;
    std::string want;
    for (int32_t g = 0; g < n; ++g) for (int64_t p = 0; p < L; ++p) planes[g * pitch + p] = value(g, p);
    for (int64_t p = 0; p < L; ++p) for (int32_t g = 0; g < n; ++g) want += std::to_string(value(g, p)) + (g + 1 < n ? " " : "\n");
    const size_t need = memo_emit_u32_rows(planes, L, pitch, n, nullptr, 0);
    if (need != want.size()) return 1;
    char *exact = (char *)malloc(need ? need : 1);                       // exactly the bytes needed
    if (memo_emit_u32_rows(planes, L, pitch, n, exact, need) != need || memcmp(exact, want.data(), need)) return 2;
    if (need) {
        char *small = (char *)malloc(need - 1 ? need - 1 : 1);           // one byte too small: nothing may be written
        memset(small, 0x5A, need - 1);
        if (memo_emit_u32_rows(planes, L, pitch, n, small, need - 1) != need) return 3;
        for (size_t i = 0; i + 1 < need; ++i) if (small[i] != 0x5A) return 4;
        free(small);
    }
    free(exact);
    free(planes);
    return 0;
}
int main() {
    for (int32_t n : {1, 2, 5, 130})
        for (int64_t L : {0, 1, 2, 63, 64, 65, 200})
            for (int64_t pad : {0, 4})
                if (int rc = check(L, L + pad, n)) return printf("n=%d L=%lld pad=%lld rc=%d\n", n, (long long)L, (long long)pad, rc), 1;
    // the threaded path: wide enough to be split over the MEMO_EMIT_THREADS threads the caller set, and the library says that it is
    const char *env = getenv("MEMO_EMIT_THREADS");
    const int threads = env ? atoi(env) : 0;
    if (threads && memo_emit_u32_rows_threads(100000, 48) != threads)
        return printf("%d threads asked for, %d used\n", threads, memo_emit_u32_rows_threads(100000, 48)), 1;
    if (int rc = check(100000, 100000 + 4, 48)) return printf("many rc=%d\n", rc), 1;
    puts("ok");
    return 0;
}
"""


def test_emit_u32_rows_under_address_and_undefined_sanitizers(tmp_path):
    """memo_emit.cpp and a stand-alone main, built with the host sanitizers and run as a program of its own"""
    src = tmp_path / "emit_rows_main.cpp"
    src.write_text(EMIT_MAIN)
    exe = str(tmp_path / "emit_rows_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "memo_amd", "csrc"),
                           os.path.join(ROOT, "memo_amd", "csrc", "memo_emit.cpp"), str(src), "-o", exe])
    for threads in ("1", "4"):
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, MEMO_EMIT_THREADS=threads))
        assert (r.returncode, r.stdout) == (0, "ok\n"), (threads, r.stdout, r.stderr[-2000:])


# ---------------------------------------------------------------------------------------
# the definition against the restated reference, on the golden membership windows
# ---------------------------------------------------------------------------------------
KS = tuple(range(1, 40)) + (64, 65, 101, 257, 299)
CAP = 300
LEGAL = ("example_memb.parquet", "rnd_n4.parquet", "rnd_n8.parquet", "rnd_n40.parquet", "rnd_n70_sparse.parquet", "rnd_n130.parquet")


def windows_of(index):
    return sorted({(c["region"], c["n"]) for c in G.cases(raises=False, membership=True) if c["index"] == index})


def test_the_golden_windows_the_promise_is_checked_on():
    """81 membership windows that do not raise, on the six golden membership indexes whose rows all have end >= start"""
    assert sum(len(windows_of(i)) for i in LEGAL) == 81
    members = {c["index"] for c in G.cases(raises=False, membership=True)}
    assert members - set(LEGAL) == {"rnd_negoverlap.parquet"}
    for index in LEGAL:
        for region, _ in windows_of(index):
            s, e, _ = G.index_columns(index, region.split(":")[0])
            assert (e >= s).all(), index


@pytest.mark.parametrize("index", LEGAL)
def test_membership_at_k_is_k_at_most_the_length(index):
    """bit g of the membership row is k <= len[g]; the row has at least T bits exactly when k <= sel_T, for every T from 1 to N"""
    from oracle import memo_oracle as O
    for region, n in windows_of(index):
        rec, se = region.split(":")
        qs, qe = map(int, se.split("-"))
        s, e, a = G.index_columns(index, rec)
        planes = lengths_oracle.planes(s, e, a, qs, qe, CAP, n).astype(np.int64)
        ranked = np.sort(planes, axis=0)[::-1]                     # ranked[T - 1] = sel_T
        assert all(np.array_equal(ranked[t - 1], lengths_oracle.select(planes, t)) for t in (1, max(n // 2, 1), n))
        assert (planes[0] == CAP).all()                            # the pivot has no rows
        for k in KS:
            f = (s > qs) & (s < qe + k)                            # the reference's own filter (memo_query.py:25-27 with main's + k)
            bits = O.bits_to_matrix(O.np_membership(s[f], e[f], a[f], qs, qe, k, n), n).astype(bool)      # [L, N]
            assert np.array_equal(bits.T, k <= planes), (index, region, k)
            held = bits.sum(axis=1)
            assert np.array_equal(held[None, :] >= np.arange(1, n + 1)[:, None], k <= ranked), (index, region, k)


# ---------------------------------------------------------------------------------------
# the slice-and-carry scheme against the whole-window definition
# ---------------------------------------------------------------------------------------
def test_slices_and_carry_give_the_whole_window():
    rng = np.random.default_rng(2024)
    runs = 0
    for trial in range(300):
        n = int(rng.integers(1, 7))
        qs = int(rng.integers(-50, 50))
        L = int(rng.integers(0, 90))
        qe = qs + L
        cap = (1, 2, 5, 40, CAP_MAX)[trial % 5]
        rows = int(rng.integers(0, 120))
        reach = min(cap, 60)
        s = rng.integers(qs - 5, qe + reach + 5, rows)
        e = s + rng.integers(-30, 60, rows)                        # rows with e < s among them: they reach across slices
        a = rng.choice(np.array(list(range(n)) + [-1, n, 2 ** 40], np.int64), rows)
        want = lengths_oracle.planes(s, e, a, qs, qe, cap, n)
        for step in (1, 3, 7, 64):
            got = lengths_oracle.sliced_planes(s, e, a, qs, qe, cap, n, step)
            assert np.array_equal(got, want), (trial, step, cap)
            runs += 1
    assert runs == 1200


def test_a_row_with_end_before_start_reaches_across_three_slices():
    # window [0, 12) in slices of 4; genome 1's row starts in the last slice and ends left of the window
    s, e, a = [11, 9, 3], [-2, 30, 5], [1, 2, 2]
    want = lengths_oracle.planes(s, e, a, 0, 12, 100, 3)
    assert want[1].tolist() == [0] * 11 + [100] and want[2].tolist() == [5, 4, 3, 27, 26, 25, 24, 23, 22, 100, 100, 100]
    assert np.array_equal(lengths_oracle.sliced_planes(s, e, a, 0, 12, 100, 3, 4), want)


# ---------------------------------------------------------------------------------------
# the README example
# ---------------------------------------------------------------------------------------
def test_the_example_numbers():
    s, e, a = G.index_columns("example_memb.parquet", "ref_1")
    planes = lengths_oracle.planes(s, e, a, 0, 20, CAP_MAX, 5)
    assert planes[1].tolist() == [3, 2, 3, 2, 3, 2, 2, 4, 3, 2, 3, 2, 4, 3, 2, 3, 2, 3, 2, 2]
    assert planes[4].tolist() == [3, 3, 4, 3, 2, 4, 3, 4, 3, 3, 4, 3, 2, 3, 4, 3, 3, 4, 3, 3]
    assert lengths_oracle.select(planes, 5).tolist() == [3, 2, 3, 2, 2, 2, 2, 4, 3, 2, 3, 2, 2, 3, 2, 3, 2, 3, 2, 2]
    assert lengths_oracle.select(planes, 3).tolist() == [5, 4, 4, 3, 3, 4, 5, 6, 5, 4, 4, 3, 3, 3, 3, 5, 4, 4, 3, 3]
    assert lengths_oracle.select(planes, 2).tolist() == [6, 5, 4, 3, 3, 8, 7, 6, 6, 5, 4, 3, 4, 4, 4, 6, 5, 4, 3, 5]
    assert (lengths_oracle.select(planes, 1) == CAP_MAX).all() and (planes[0] == CAP_MAX).all()
    # across the two index kinds: the T-th largest length of the membership index is `memo maxk -t T` of the conservation index
    cs, ce, ca = G.index_columns("example_cons.parquet", "ref_1")
    for t in range(1, 6):
        assert np.array_equal(lengths_oracle.select(planes, t), maxk_oracle.maxk(cs, ce, ca, 0, 20, CAP_MAX, threshold=t)), t
    assert lengths_oracle.text(lengths_oracle.select(planes, 5)).startswith(b"3\n2\n3\n2\n2\n")
    assert lengths_oracle.rows_text(planes[:, :2]) == b"2147483647 3 %d %d 3\n2147483647 2 %d %d 3\n" % (planes[2][0], planes[3][0], planes[2][1], planes[3][1])
