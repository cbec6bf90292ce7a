"""`memo maxk` without a GPU: the command line (usage bytes, getopts handling, every refusal before the library is even loaded),
memo_emit_u32 against a Python formatter, and the definition itself (tests/maxk_oracle.py) against the restated reference
(oracle.memo_oracle.np_conservation / np_membership) on the golden windows: for rows with end >= start, "shared at k" is k <= maxk."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import golden_util as G
from tests import maxk_oracle

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
    from memo_amd import maxk_cli
    usage = _fixture("memo_maxk_usage.txt")
    assert usage == maxk_cli.USAGE.encode() and usage.startswith(b"\nMEMO maxk - ") and usage.endswith(b"\n\n")
    for argv in ((), ("-h",)):
        r = _memo("maxk", *argv)
        assert (r.returncode, r.stdout, r.stderr) == (0, usage, b""), argv
    for flag in (b"-b [FILE]", b"-n [INT]", b"-r [CHR:START-END]", b"-o [FILE]", b"-t [INT]", b"  -m  ", b"-d [INT]", b"-K [INT]"):
        assert flag in usage
    assert b"-k " not in usage                                   # there is no k: that is the point


def test_illegal_option_prints_getopts_message_then_usage():
    usage = _fixture("memo_maxk_usage.txt")
    r = _memo("maxk", "-k", "31")
    assert r.returncode == 0 and r.stdout == usage and r.stderr.endswith(b": illegal option -- k\n")
    r = _memo("maxk", "-n", "5", "-K")
    assert r.returncode == 0 and r.stdout == usage and r.stderr.endswith(b": option requires an argument -- K\n")


def test_the_reference_sub_commands_print_what_they_printed():
    for argv, fixture in (([], "memo_usage.txt"), (["-h"], "memo_usage.txt"), (["bogus"], "memo_bogus.txt")):
        r = _memo(*argv)
        assert r.returncode == 0 and r.stdout == _fixture(fixture), argv
    assert b"maxk" not in _fixture("memo_usage.txt")          # the reference's text: the sub-command is documented in the README


def test_refusals_before_the_library_is_touched(tmp_path):
    """(-b names no file and the library path names none: a refusal that came later would be another message)"""
    out = str(tmp_path / "never.txt")
    common = ("-b", str(tmp_path / "no.parquet"), "-r", "ref_1:0-20", "-o", out)
    for extra, env, message in ((("-n", "5"), {"WORLD_SIZE": "2"}, b"sharded launch"),
                                (("-n", "5"), {"MEMO_FORCE_SHARDED": "1"}, b"sharded launch"),
                                (("-n", "5", "-m"), None, b"-m needs -d"),
                                (("-n", "5", "-d", "1"), None, b"it needs -m"),
                                (("-n", "5", "-m", "-d", "1", "-t", "3"), None, b"-t cannot be combined with -m"),
                                (("-n", "five"), None, b"invalid literal for int()"),
                                (("-n", "5", "-t", "0"), None, b"-t must be an integer in [1, 5]"),
                                (("-n", "5", "-t", "6"), None, b"-t must be an integer in [1, 5]"),
                                (("-n", "5", "-t", "2.5"), None, b"-t must be an integer in [1, 5]"),
                                (("-n", "5", "-m", "-d", "5"), None, b"-d must be an integer in [0, 5)"),
                                (("-n", "5", "-m", "-d", "-1"), None, b"-d must be an integer in [0, 5)"),
                                (("-n", "5", "-m", "-d", "x"), None, b"-d must be an integer in [0, 5)"),
                                (("-n", "5", "-K", "0"), None, b"-K must be an integer in [1, 2147483647]"),
                                (("-n", "5", "-K", str(2 ** 31)), None, b"-K must be an integer in [1, 2147483647]"),
                                (("-n", "5", "-K", "many"), None, b"-K must be an integer in [1, 2147483647]")):
        r = _memo("maxk", *common, *extra, env=env)
        assert r.returncode == 1 and r.stdout == b"MEMO - maxk\n", (extra, r.stderr)
        assert r.stderr.startswith(b"memo maxk: ") and message in r.stderr and r.stderr.count(b"\n") == 1, (extra, r.stderr)
        assert not os.path.exists(out)
    # the same command with nothing to refuse does reach the library, which is not there
    for extra in (("-n", "5"), ("-n", "5", "-t", "5", "-K", str(CAP_MAX)), ("-n", "5", "-m", "-d", "0", "-K", "1")):
        r = _memo("maxk", *common, *extra)
        assert r.returncode == 1 and not os.path.exists(out)
        assert b"Traceback" in r.stderr or b"memo maxk: " in r.stderr
        assert b"must be an integer" not in r.stderr and b"needs" not in r.stderr


def test_missing_flags_are_named():
    r = _memo("maxk", "-b", "x.parquet", "-K", "3")
    assert r.returncode == 2 and r.stdout == b"MEMO - maxk\n" and r.stderr == b"memo maxk: -r, -n, -o required\n"
    r = _memo("maxk", "-r", "ref_1:0-20", "-n", "5", "-o", "x", "-m")
    assert r.returncode == 2 and r.stderr == b"memo maxk: -b required\n"


def test_names_are_exported():
    import memo_amd
    from memo_amd import maxk
    assert memo_amd.maxk is maxk and memo_amd.region_maxk is maxk.region_maxk and memo_amd.index_maxk is maxk.index_maxk
    assert callable(maxk.maxk)


# ---------------------------------------------------------------------------------------
# memo_emit_u32 (host code of the library: no device is touched)
# ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import memo_amd
    from memo_amd import _lib
    memo_amd.build()                     # make: a no-op when libmemo_amd.so is up to date
    return _lib.lib()


def _emit(lib, vec, room=None, guard=16):
    """(bytes needed, the buffer's first `room` bytes, whether the `guard` bytes behind them are untouched)"""
    vec = np.ascontiguousarray(vec, np.uint32)
    need = lib.memo_emit_u32(vec.ctypes.data, len(vec), None, 0)
    room = need if room is None else room
    buf = np.full(room + guard, 0xEE, np.uint8)
    got = lib.memo_emit_u32(vec.ctypes.data, len(vec), buf.ctypes.data, room)
    assert got == need
    return need, buf[:room].tobytes(), bool((buf[room:] == 0xEE).all())


def test_emit_u32_against_a_python_formatter(lib):
    edge = [0, 9, 10, 99, 100, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1]
    for vec in ([], [0], [2 ** 32 - 1], edge, edge[::-1]):
        want = maxk_oracle.text(vec)
        need, got, clean = _emit(lib, vec)
        assert (need, got, clean) == (len(want), want, True), vec
    assert _emit(lib, [])[0] == 0                                # an empty window is an empty file, not a lone newline
    assert maxk_oracle.text([0, 4294967295]) == b"0\n4294967295\n"          # (the formatter itself, against a literal)


def test_emit_u32_writes_nothing_when_a_byte_is_missing(lib):
    vec = [7, 2 ** 32 - 1, 10]
    want = maxk_oracle.text(vec)
    need, got, clean = _emit(lib, vec, room=len(want) - 1)
    assert need == len(want) and got == b"\xee" * (len(want) - 1) and clean
    need, got, clean = _emit(lib, vec, room=0)
    assert need == len(want) and clean


def test_emit_u32_threaded_path(lib):
    """10^5 lines of every width; with four emit threads forced (the library reads MEMO_EMIT_THREADS per call) and as the machine
    decides"""
    rng = np.random.default_rng(5)
    vec = (rng.integers(0, 2 ** 32, 100_000, dtype=np.uint64) >> rng.integers(0, 32, 100_000, dtype=np.uint64)).astype(np.uint32)
    vec[:3] = (0, 2 ** 32 - 1, 10)
    want = maxk_oracle.text(vec)
    assert _emit(lib, vec) == (len(want), want, True)
    from memo_amd import maxk
    assert maxk.emit(vec).tobytes() == want and maxk.emit(vec[:0]).tobytes() == b""
    code = ("import sys; sys.path.insert(0, %r)\nimport numpy as np\nfrom memo_amd import maxk\n"
            "v = (np.arange(100000, dtype=np.uint64) * 2654435761 %% 2 ** 32).astype(np.uint32)\n"
            "sys.stdout.buffer.write(maxk.emit(v).tobytes())" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, env=dict(os.environ, MEMO_EMIT_THREADS="4"))
    v = (np.arange(100000, dtype=np.uint64) * 2654435761 % 2 ** 32).astype(np.uint32)
    assert r.returncode == 0 and r.stdout == maxk_oracle.text(v), r.stderr[-500:]


EMIT_MAIN = r"""
// memo_emit_u32 with heap buffers of exactly the sizes it is told: a write past `cap`, or a read past vec[L), is the sanitizer's
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include "memo_amd_dap.h"
static int check(const uint32_t *src, int64_t L) {
    uint32_t *vec = (uint32_t *)malloc(L ? (size_t)L * 4 : 1);          // exactly L values
    if (L) memcpy(vec, src, (size_t)L * 4);
    std::string want;
    for (int64_t i = 0; i < L; ++i) want += std::to_string(vec[i]) + "\n";
    const size_t need = memo_emit_u32(vec, L, nullptr, 0);
    if (need != want.size()) return 1;
    char *exact = (char *)malloc(need ? need : 1);                       // exactly the bytes needed
    if (memo_emit_u32(vec, L, exact, need) != need || memcmp(exact, want.data(), need)) return 2;
    if (need) {
        char *small = (char *)malloc(need - 1 ? need - 1 : 1);           // one byte too small: nothing may be written
        memset(small, 0x5A, need - 1);
        if (memo_emit_u32(vec, L, small, need - 1) != need) return 3;
        for (size_t i = 0; i + 1 < need; ++i) if (small[i] != 0x5A) return 4;
        free(small);
    }
    free(exact);
    free(vec);
    return 0;
}
int main() {
    const uint32_t edge[] = {0u, 9u, 10u, 2147483647u, 4294967295u};
    for (int64_t L = 0; L <= 5; ++L) if (int rc = check(edge, L)) return printf("edge L=%lld rc=%d\n", (long long)L, rc), 1;
    const int64_t many = 100000;                                         // the threaded path (MEMO_EMIT_THREADS)
    uint32_t *v = (uint32_t *)malloc(many * 4);
    for (int64_t i = 0; i < many; ++i) v[i] = (uint32_t)(i * 2654435761u) >> (i % 32);
    if (int rc = check(v, many)) return printf("many rc=%d\n", rc), 1;
    free(v);
    puts("ok");
    return 0;
}
"""


def test_emit_u32_under_address_and_undefined_sanitizers(tmp_path):
    """memo_emit.cpp and a stand-alone main, built with the host sanitizers and run as a program of its own"""
    src = tmp_path / "emit_main.cpp"
    src.write_text(EMIT_MAIN)
    exe = str(tmp_path / "emit_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "memo_amd", "csrc"),
                           os.path.join(ROOT, "memo_amd", "csrc", "memo_emit.cpp"), str(src), "-o", exe])
    for threads in ("1", "4"):
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, MEMO_EMIT_THREADS=threads))
        assert (r.returncode, r.stdout) == (0, "ok\n"), (threads, r.stdout, r.stderr[-2000:])


# ---------------------------------------------------------------------------------------
# the definition against the restated reference, on the golden windows
# ---------------------------------------------------------------------------------------
KS = tuple(range(1, 40)) + (64, 65, 101, 257, 299)
CAP = 300
LEGAL = sorted({c["index"] for c in G.cases(raises=False)} - {"rnd_negoverlap.parquet"})          # every row has end >= start


def test_the_golden_indexes_the_equivalence_is_promised_for():
    """seven files, nine chromosomes with rows: every golden index except rnd_negoverlap.parquet"""
    cases = [c for c in G.cases(raises=False) if c["index"] in LEGAL]
    chromosomes = {(c["index"], G.region(c)[0]) for c in cases if len(G.index_columns(c["index"], G.region(c)[0])[0])}
    windows = {(c["index"], c["region"], c["n"], c["membership"]) for c in cases}
    assert len(LEGAL) == 7 and len(chromosomes) == 9 and len(windows) >= 100
    for index, rec in chromosomes:
        s, e, _ = G.index_columns(index, rec)
        assert (e >= s).all(), index
    s, e, _ = G.index_columns("rnd_negoverlap.parquet", G.region(next(c for c in G.cases() if c["index"] == "rnd_negoverlap.parquet"))[0])
    assert (e < s).any()


@pytest.mark.parametrize("index", LEGAL)
def test_shared_at_k_is_k_at_most_maxk(index):
    from oracle import memo_oracle as O
    windows = {(c["region"], c["n"], c["membership"]) for c in G.cases(raises=False) if c["index"] == index}
    for region, n, membership in sorted(windows):
        rec, se = region.split(":")
        qs, qe = map(int, se.split("-"))
        s, e, a = G.index_columns(index, rec)
        preds = [dict(genome=g) for g in range(min(6, n))] if membership else [dict(threshold=t) for t in sorted({1, max(n // 2, 1), n})]
        longest = [maxk_oracle.maxk(s, e, a, qs, qe, CAP, **p).astype(np.int64) for p in preds]
        for k in KS:
            f = (s > qs) & (s < qe + k)                          # the reference's own filter (memo_query.py:25-27 with main's + k)
            if membership:
                bits = O.bits_to_matrix(O.np_membership(s[f], e[f], a[f], qs, qe, k, n), n)
                shared = [bits[:, p["genome"]].astype(bool) for p in preds]
            else:
                cons = O.np_conservation(s[f], e[f], a[f], qs, qe, k, n).astype(np.int64)
                shared = [cons >= p["threshold"] for p in preds]
            for p, want, got in zip(preds, shared, longest):
                assert np.array_equal(want, k <= got), (index, region, k, p)


def test_the_oracle_on_a_hand_made_window():
    # window [10, 20), rows (start, end, annot); T = 2 selects annots 0 and 1
    s, e, a = [12, 15, 15, 18, 40, 10, 300], [14, 15, 30, 19, 41, 11, 5], [0, 1, 5, 0, 1, 0, 0]
    #  p:           10 11 | 12 13 14 | 15 16 17 | 18 19       bound = the smallest end among the selected rows with start > p
    #  rows right:  14 14 | 15 15 15 | 19 19 19 | 41 41       (start 10 = qs is ignored; start 300 >= qe + cap is ignored)
    want = [4, 3, 3, 2, 1, 4, 3, 2, 23, 22]
    assert maxk_oracle.maxk(s, e, a, 10, 20, 100, threshold=2).tolist() == want
    assert maxk_oracle.maxk(s, e, a, 10, 20, 3, threshold=2).tolist() == [min(v, 3) for v in want]
    assert maxk_oracle.maxk(s, e, a, 10, 20, 100, genome=5).tolist() == [20, 19, 18, 17, 16] + [100] * 5
    assert maxk_oracle.maxk(s, e, a, 10, 20, 100, threshold=1).tolist() == [4, 3, 7, 6, 5, 4, 3, 2, 100, 100]
    assert maxk_oracle.maxk(s, e, a, 10, 20, 1000, threshold=1).tolist() == [0] * 10     # now start 300 counts: its end 5 is left of every p
    assert maxk_oracle.maxk([], [], [], 10, 20, 7, threshold=1).tolist() == [7] * 10
    assert maxk_oracle.maxk(s, e, a, 10, 10, 7, threshold=1).tolist() == []
