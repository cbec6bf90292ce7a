"""`memo mems` without a GPU: the command line (usage bytes, getopts handling, every refusal before the library is even loaded),
memo_emit_intervals against a Python formatter and as a program of its own under the host sanitizers, the definition itself
(tests/mems_oracle.py) on the worked example of DESIGN.md 10.13 and on the golden indexes, and the host-side merge of `-u`."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import golden_util as G
from tests import mems_oracle

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
    from memo_amd import mems_cli
    usage = _fixture("memo_mems_usage.txt")
    assert usage == mems_cli.USAGE.encode() and usage.startswith(b"\nMEMO mems - ") and usage.endswith(b"\n\n")
    for argv in ((), ("-h",)):
        r = _memo("mems", *argv)
        assert (r.returncode, r.stdout, r.stderr) == (0, usage, b""), argv
    for flag in (b"-b [FILE]", b"-n [INT]", b"-r [CHR:START-END]", b"-o [FILE]", b"-t [INT]", b"  -m  ", b"-d [INT]", b"  -a  ", b"-l [INT]",
                 b"-K [INT]", b"  -u  "):
        assert flag in usage
    assert b"-k " not in usage                                   # like `memo maxk` it takes no k


def test_illegal_option_prints_getopts_message_then_usage():
    usage = _fixture("memo_mems_usage.txt")
    r = _memo("mems", "-k", "31")
    assert r.returncode == 0 and r.stdout == usage and r.stderr.endswith(b": illegal option -- k\n")
    r = _memo("mems", "-n", "5", "-l")
    assert r.returncode == 0 and r.stdout == usage and r.stderr.endswith(b": option requires an argument -- l\n")


def test_the_reference_sub_commands_print_what_they_printed():
    for argv, fixture in (([], "memo_usage.txt"), (["-h"], "memo_usage.txt"), (["bogus"], "memo_bogus.txt")):
        r = _memo(*argv)
        assert r.returncode == 0 and r.stdout == _fixture(fixture), argv
    assert b"mems" not in _fixture("memo_usage.txt")          # the reference's text: the sub-command is documented in the README


def test_refusals_before_the_library_is_touched(tmp_path):
    """(-b names no file and the library path names none: a refusal that came later would be another message)"""
    out = str(tmp_path / "never.bed")
    common = ("-b", str(tmp_path / "no.parquet"), "-r", "ref_1:0-20", "-o", out)
    cap_range = b"[1, 2147483647]"
    for extra, env, message in ((("-n", "5"), {"WORLD_SIZE": "2"}, b"sharded launch"),
                                (("-n", "5"), {"MEMO_FORCE_SHARDED": "1"}, b"sharded launch"),
                                (("-n", "5", "-d", "1"), None, b"-d is a genome of a membership index: it needs -m"),
                                (("-n", "5", "-a"), None, b"-a is every genome of a membership index: it needs -m"),
                                (("-n", "5", "-m", "-d", "1", "-a"), None, b"-d cannot be combined with -a"),
                                (("-n", "5", "-m", "-d", "1", "-t", "3"), None, b"-t cannot be combined with -d or -a"),
                                (("-n", "5", "-m", "-a", "-t", "3"), None, b"-t cannot be combined with -d or -a"),
                                (("-n", "five"), None, b"invalid literal for int()"),
                                (("-n", "5", "-t", "0"), None, b"-t must be an integer in [1, 5]"),
                                (("-n", "5", "-t", "6"), None, b"-t must be an integer in [1, 5]"),
                                (("-n", "5", "-m", "-t", "6"), None, b"-t must be an integer in [1, 5]"),
                                (("-n", "5", "-t", "2.5"), None, b"-t must be an integer in [1, 5]"),
                                (("-n", "5", "-m", "-d", "5"), None, b"-d must be an integer in [0, 5)"),
                                (("-n", "5", "-m", "-d", "-1"), None, b"-d must be an integer in [0, 5)"),
                                (("-n", "5", "-m", "-d", "x"), None, b"-d must be an integer in [0, 5)"),
                                (("-n", "5", "-K", "0"), None, b"-K must be an integer in " + cap_range),
                                (("-n", "5", "-K", str(2 ** 31)), None, b"-K must be an integer in " + cap_range),
                                (("-n", "5", "-K", "many"), None, b"-K must be an integer in " + cap_range),
                                (("-n", "5", "-l", "0"), None, b"-l must be an integer in " + cap_range),
                                (("-n", "5", "-l", str(2 ** 31)), None, b"-l must be an integer in " + cap_range),
                                (("-n", "5", "-l", "long"), None, b"-l must be an integer in " + cap_range),
                                (("-n", "5", "-K", "30", "-l", "31"), None, b"-l must be an integer in [1, 30]"),
                                (("-n", "5", "-u", "-l", "0"), None, b"-l must be an integer in " + cap_range),
                                (("-n", "5", "-u", "-K", "31"), None, b"-K cannot be combined with -u"),
                                (("-n", "5", "-u", "-l", "3", "-K", "31"), None, b"-K cannot be combined with -u")):
        r = _memo("mems", *common, *extra, env=env)
        assert r.returncode == 1 and r.stdout == b"MEMO - mems\n", (extra, r.stderr)
        assert r.stderr.startswith(b"memo mems: ") and message in r.stderr and r.stderr.count(b"\n") == 1, (extra, r.stderr)
        assert not os.path.exists(out)
    # the same command with nothing to refuse does reach the library, which is not there
    for extra in (("-n", "5"), ("-n", "5", "-t", "5", "-K", str(CAP_MAX), "-l", str(CAP_MAX)), ("-n", "5", "-m", "-d", "0", "-K", "1"),
                  ("-n", "5", "-m", "-a", "-l", "3"), ("-n", "5", "-m", "-t", "3", "-u", "-l", "31"), ("-n", "5", "-m", "-a", "-u")):
        r = _memo("mems", *common, *extra)
        assert r.returncode == 1 and not os.path.exists(out)
        assert b"Traceback" in r.stderr or b"memo mems: " in r.stderr
        assert b"must be an integer" not in r.stderr and b"needs" not in r.stderr and b"combined" not in r.stderr


def test_missing_flags_are_named():
    r = _memo("mems", "-b", "x.parquet", "-K", "3")
    assert r.returncode == 2 and r.stdout == b"MEMO - mems\n" and r.stderr == b"memo mems: -r, -n, -o required\n"
    r = _memo("mems", "-r", "ref_1:0-20", "-n", "5", "-o", "x", "-m", "-a")
    assert r.returncode == 2 and r.stderr == b"memo mems: -b required\n"


def test_names_are_exported():
    import memo_amd
    from memo_amd import mems
    assert memo_amd.mems is mems and memo_amd.region_mems is mems.region_mems and callable(mems.of_cells)


def test_region_mems_refuses_before_the_library_is_touched(tmp_path):
    from memo_amd import mems
    nowhere = str(tmp_path / "no.parquet")
    for kw in (dict(genome=1), dict(all_genomes=True), dict(membership=True, genome=1, all_genomes=True),
               dict(membership=True, genome=1, threshold=2), dict(membership=True, all_genomes=True, threshold=2), dict(threshold=0),
               dict(threshold=6), dict(membership=True, genome=5), dict(min_len=0), dict(cap=0), dict(cap=2 ** 31), dict(cap=30, min_len=31),
               dict(union=True, cap=31), dict(union=True, min_len=0), dict(union=True, min_len=2 ** 31)):
        with pytest.raises(ValueError):
            mems.region_mems(nowhere, "ref_1:0-20", 5, **kw)
    with pytest.raises(ValueError):
        mems.region_mems(nowhere, "ref_1:0-20", 2049)
    with pytest.raises(ValueError):
        mems.region_mems(nowhere, "ref_1:20-0", 5)
    with pytest.raises(ValueError):
        mems.region_mems(nowhere, "ref_1:-3-20", 5)
    with pytest.raises(ValueError):
        mems.region_mems(nowhere, f"ref_1:0-{2 ** 31}", 5)


# ---------------------------------------------------------------------------------------
# memo_emit_intervals (host code of the library: no device is touched)
# ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import memo_amd
    from memo_amd import _lib
    memo_amd.build()                     # make: a no-op when libmemo_amd.so is up to date
    return _lib.lib()


def _emit(lib, record, starts, ends, genome=None, room=None, guard=16):
    """(bytes needed, the buffer's first `room` bytes, whether the `guard` bytes behind them are untouched)"""
    s, e = np.ascontiguousarray(starts, np.int64), np.ascontiguousarray(ends, np.int64)
    g = None if genome is None else np.ascontiguousarray(genome, np.int32)
    args = (record.encode(), s.ctypes.data, e.ctypes.data, None if g is None else g.ctypes.data, len(s))
    need = lib.memo_emit_intervals(*args, None, 0)
    room = need if room is None else room
    buf = np.full(room + guard, 0xEE, np.uint8)
    got = lib.memo_emit_intervals(*args, buf.ctypes.data, room)
    assert got == need
    return need, buf[:room].tobytes(), bool((buf[room:] == 0xEE).all())


def _python_text(record, starts, ends, genome=None):
    if genome is None:
        return "".join(f"{record}\t{b}\t{e}\n" for b, e in zip(starts, ends)).encode()
    return "".join(f"{record}\t{b}\t{e}\t{g}\n" for b, e, g in zip(starts, ends, genome)).encode()


def test_emit_intervals_against_a_python_formatter(lib):
    edge = [0, 9, 10, 99, 100, 2 ** 31 - 1, 2 ** 31, 2 ** 32 + 5, 2 ** 62]
    ends = [v + 3 for v in edge]
    genomes = [1, 2, 9, 10, 99, 100, 2047, 0, 2 ** 31 - 1]
    for rec in ("ref_1", "c", "a name with blanks"):
        for n in (0, 1, len(edge)):
            want = _python_text(rec, edge[:n], ends[:n])
            assert _emit(lib, rec, edge[:n], ends[:n]) == (len(want), want, True), (rec, n)
            want = _python_text(rec, edge[:n], ends[:n], genomes[:n])
            assert _emit(lib, rec, edge[:n], ends[:n], genomes[:n]) == (len(want), want, True), (rec, n)
    assert _emit(lib, "ref_1", [], [])[0] == 0 and _emit(lib, "ref_1", [], [], [])[0] == 0       # no entries: no bytes
    assert _python_text("r", [0], [4294967301]) == b"r\t0\t4294967301\n" and _python_text("r", [7], [9], [3]) == b"r\t7\t9\t3\n"
    assert mems_oracle.text("r", [7], [9], 3) == b"r\t7\t9\t3\n" and mems_oracle.text("r", [7, 8], [9, 9]) == b"r\t7\t9\nr\t8\t9\n"


def test_emit_intervals_writes_nothing_when_a_byte_is_missing(lib):
    starts, ends, genome = [7, 2 ** 40, 10], [8, 2 ** 40 + 31, 10], [1, 1, 2047]
    for g in (None, genome):
        want = _python_text("chr1", starts, ends, g)
        need, got, clean = _emit(lib, "chr1", starts, ends, g, room=len(want) - 1)
        assert need == len(want) and got == b"\xee" * (len(want) - 1) and clean
        need, got, clean = _emit(lib, "chr1", starts, ends, g, room=0)
        assert need == len(want) and clean


def test_emit_of_a_result_and_the_threaded_path(lib):
    from memo_amd import mems
    rng = np.random.default_rng(3)
    n = 300_000                                                  # more than one thread's share of lines
    starts = np.sort(rng.integers(0, 2 ** 40, n))
    ends = starts + rng.integers(1, 2 ** 31, n)
    genome = np.sort(rng.integers(1, 2048, n)).astype(np.int32)
    assert mems.emit(mems.Mems("chr7", starts, ends, None)).tobytes() == _python_text("chr7", starts.tolist(), ends.tolist())
    assert mems.emit(mems.Mems("chr7", starts, ends, genome)).tobytes() == _python_text("chr7", starts.tolist(), ends.tolist(), genome.tolist())
    assert mems.emit(mems.Mems("chr7", starts[:0], ends[:0], None)).tobytes() == b""
    with pytest.raises(ValueError):
        mems.emit(mems.Mems("chr7", starts, ends[:-1], None))


EMIT_MAIN = r"""
// memo_emit_intervals with heap buffers of exactly the sizes it is told: a write past `cap`, or a read past the entries, is the sanitizer's
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include "memo_amd_dap.h"
static int check(const char *rec, const int64_t *s_, const int64_t *e_, const int32_t *g_, int64_t n, bool with_genome) {
    int64_t *s = (int64_t *)malloc(n ? (size_t)n * 8 : 1), *e = (int64_t *)malloc(n ? (size_t)n * 8 : 1);   // exactly n entries
    int32_t *g = with_genome ? (int32_t *)malloc(n ? (size_t)n * 4 : 1) : nullptr;
    if (n) memcpy(s, s_, (size_t)n * 8), memcpy(e, e_, (size_t)n * 8);
    if (n && g) memcpy(g, g_, (size_t)n * 4);
    char *name = (char *)malloc(strlen(rec) + 1);                       // exactly the name and its terminator
    strcpy(name, rec);
    std::string want;
    for (int64_t i = 0; i < n; ++i)
        want += std::string(rec) + "\t" + std::to_string(s[i]) + "\t" + std::to_string(e[i]) + (g ? "\t" + std::to_string(g[i]) : "") + "\n";
    const size_t need = memo_emit_intervals(name, s, e, g, (uint64_t)n, nullptr, 0);
    if (need != want.size()) return 1;
    char *exact = (char *)malloc(need ? need : 1);                       // exactly the bytes needed
    if (memo_emit_intervals(name, s, e, g, (uint64_t)n, exact, need) != need || memcmp(exact, want.data(), need)) return 2;
    if (need) {
        char *small = (char *)malloc(need - 1 ? need - 1 : 1);           // one byte too small: nothing may be written
        memset(small, 0x5A, need - 1);
        if (memo_emit_intervals(name, s, e, g, (uint64_t)n, small, need - 1) != need) return 3;
        for (size_t i = 0; i + 1 < need; ++i) if (small[i] != 0x5A) return 4;
        free(small);
    }
    free(exact), free(name), free(s), free(e), free(g);
    return 0;
}
int main() {
    const int64_t s[] = {0, 9, 10, 2147483647LL, 4294967301LL, 4611686018427387904LL};
    const int64_t e[] = {1, 19, 10, 4294967294LL, 4294967302LL, 4611686018427387935LL};
    const int32_t g[] = {1, 9, 10, 99, 2047, 2147483647};
    for (int with = 0; with < 2; ++with)
        for (int64_t n = 0; n <= 6; ++n)
            if (int rc = check("ref_1", s, e, g, n, with)) return printf("edge n=%lld genome=%d rc=%d\n", (long long)n, with, rc), 1;
    if (int rc = check("", s, e, g, 3, true)) return printf("empty name rc=%d\n", rc), 1;
    const int64_t many = 300000;                                         // the threaded path (MEMO_EMIT_THREADS)
    int64_t *ms = (int64_t *)malloc(many * 8), *me = (int64_t *)malloc(many * 8);
    int32_t *mg = (int32_t *)malloc(many * 4);
    for (int64_t i = 0; i < many; ++i) ms[i] = (i * 2654435761LL) >> (i % 20), me[i] = ms[i] + 1 + i % 977, mg[i] = (int32_t)(i % 2048);
    for (int with = 0; with < 2; ++with)
        if (int rc = check("chr12", ms, me, mg, many, with)) return printf("many genome=%d rc=%d\n", with, rc), 1;
    free(ms), free(me), free(mg);
    puts("ok");
    return 0;
}
"""


def test_emit_intervals_under_address_and_undefined_sanitizers(tmp_path):
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
# the definition: the worked example, and its promises on the golden indexes
# ---------------------------------------------------------------------------------------
def _pairs(starts, ends):
    return " ".join(f"{b}-{e}" for b, e in zip(np.asarray(starts).tolist(), np.asarray(ends).tolist()))


EXAMPLE_T5 = "0-3 2-5 4-6 5-7 6-8 7-11 10-13 12-14 13-16 15-18 17-20 19-21"
EXAMPLE_T3 = "0-5 2-6 4-7 5-9 6-11 7-13 10-14 12-15 13-16 14-17 15-20 17-21 19-22"
EXAMPLE_G1 = "0-3 2-5 4-7 6-8 7-11 10-13 12-16 15-18 17-20 19-21"
EXAMPLE_G4 = "0-3 1-4 2-6 5-9 7-11 9-12 10-14 13-16 14-18 16-19 17-21 19-22"


def test_the_oracle_on_the_worked_example():
    cons = G.index_columns("example_cons.parquet", "ref_1")
    memb = G.index_columns("example_memb.parquet", "ref_1")
    assert mems_oracle.vector(*cons, 0, 20, CAP_MAX, 5, threshold=5).tolist() == [3, 2, 3, 2, 2, 2, 2, 4, 3, 2, 3, 2, 2, 3, 2, 3, 2, 3, 2, 2]
    t5 = mems_oracle.matches(*cons, 0, 20, CAP_MAX, 5, threshold=5)
    assert _pairs(*t5) == EXAMPLE_T5 and len(t5[0]) == 12
    assert _pairs(*mems_oracle.matches(*cons, 0, 20, CAP_MAX, 5, threshold=5, min_len=3)) == "0-3 2-5 7-11 10-13 13-16 15-18 17-20"
    assert _pairs(*mems_oracle.union(*cons, 0, 20, 5, threshold=5, min_len=3)) == "0-5 7-20"
    t3 = mems_oracle.matches(*cons, 0, 20, CAP_MAX, 5, threshold=3)
    assert _pairs(*t3) == EXAMPLE_T3 and len(t3[0]) == 13
    assert _pairs(*mems_oracle.union(*cons, 0, 20, 5, threshold=3, min_len=3)) == "0-22"
    for t, want in ((5, EXAMPLE_T5), (3, EXAMPLE_T3)):          # the membership index holds the same stretches
        assert _pairs(*mems_oracle.matches(*memb, 0, 20, CAP_MAX, 5, threshold=t, membership=True)) == want
    g1 = mems_oracle.matches(*memb, 0, 20, CAP_MAX, 5, genome=1, membership=True)
    g4 = mems_oracle.matches(*memb, 0, 20, CAP_MAX, 5, genome=4, membership=True)
    assert _pairs(*g1) == EXAMPLE_G1 and len(g1[0]) == 10 and _pairs(*g4) == EXAMPLE_G4 and len(g4[0]) == 12
    every = mems_oracle.all_matches(*memb, 0, 20, CAP_MAX, 5)
    assert [g for g, _, _ in every] == [1, 2, 3, 4] and _pairs(*every[0][1:]) == EXAMPLE_G1 and _pairs(*every[3][1:]) == EXAMPLE_G4
    # the pivot has no rows: one match of the cap, at position 0
    assert _pairs(*mems_oracle.matches(*memb, 0, 20, 31, 5, genome=0, membership=True)) == "0-31"
    assert _pairs(*mems_oracle.matches(*memb, 5, 20, 31, 5, genome=0, membership=True)) == ""


def test_the_start_rule_on_values():
    S = mems_oracle.starts_of
    assert S([], 9, 1, 0).tolist() == [] and S([5], 9, 1, 0).tolist() == [0] and S([5], 9, 1, 1).tolist() == [] and S([5], 9, 6, 0).tolist() == []
    assert S([3, 3, 3], 9, 1, 0).tolist() == [0, 1, 2] and S([3, 3, 3], 3, 1, 0).tolist() == [0]      # equal below the cap; a run at the cap
    assert S([3, 3, 3], 3, 1, 1).tolist() == [] and S([3, 3, 3], 9, 1, 1).tolist() == [1, 2]
    assert S([5, 4, 3, 2, 1, 0], 9, 1, 0).tolist() == [0] and S([1, 2, 3], 9, 1, 1).tolist() == [1, 2]
    assert S([9, 9, 8, 9, 9, 7, 9], 9, 1, 0).tolist() == [0, 3, 6] and S([0, 0, 0], 9, 1, 0).tolist() == []
    assert S([2, 3, 2, 3], 9, 3, 0).tolist() == [1, 3] and S([1, 1, 1], 1, 1, 0).tolist() == [0]
    B = mems_oracle.band_boundaries
    assert B([], 2).tolist() == [] and B([3, 3, 1, 2, 0], 2).tolist() == [0, 2, 3, 4] and B([0, 2, 2], 2).tolist() == [1] and B([2], 2).tolist() == [0]


LEGAL = sorted({c["index"] for c in G.cases(raises=False)} - {"rnd_negoverlap.parquet"})          # every row has end >= start


def _modes(index, n):
    """(the rnd_* files are read as either kind of index by the golden cases: so are they here)"""
    kinds = {c["membership"] for c in G.cases(raises=False) if c["index"] == index}
    modes = [dict(threshold=t) for t in sorted({1, max(n // 2, 1), n})] if False in kinds else []
    if True in kinds:
        modes += [dict(membership=True, genome=g) for g in sorted({0, 1, n - 1})] + [dict(membership=True, threshold=max(n // 2, 1))]
    return modes


def _whole(index):
    case = next(c for c in G.cases(raises=False) if c["index"] == index)
    rec = G.region(case)[0]
    s, e, a = G.index_columns(index, rec)
    return rec, s, e, a, int(s.max()) - 1, case["n"]           # (every position left of the last start is bounded by a row)


@pytest.mark.parametrize("index", LEGAL)
def test_the_promises_hold_on_the_golden_indexes(index):
    """windows laid end to end are the whole; the list expands to `memo maxk`'s vector where no value is the cap; the covered bases are
    the union of the reported matches of at least min_len at any larger cap up to the window's end, where no value is that cap (a run at the cap is reported
    once, as cap bases from its first position, and what lies past them is not in the list)"""
    rec, s, e, a, end, n = _whole(index)
    expanded = unions = 0
    for mode in _modes(index, n):
        for cap in (31, CAP_MAX):
            whole = mems_oracle.matches(s, e, a, 0, end, cap, n, **mode)
            for cut in (end // 3, end // 3 + 1, end // 2):
                left, right = mems_oracle.matches(s, e, a, 0, cut, cap, n, **mode), mems_oracle.matches(s, e, a, cut, end, cap, n, **mode)
                assert np.array_equal(np.concatenate([left[0], right[0]]), whole[0]), (index, mode, cap, cut)
                assert np.array_equal(np.concatenate([left[1], right[1]]), whole[1]), (index, mode, cap, cut)
            v = mems_oracle.vector(s, e, a, 0, end, cap, n, **mode).astype(np.int64)
            if not (v == cap).any():
                assert np.array_equal(mems_oracle.expand(*whole, 0, end), v), (index, mode, cap)
                expanded += 1
        for min_len in (1, 3, 8, 31):
            want = mems_oracle.union(s, e, a, 0, end, n, min_len=min_len, **mode)
            for cap in (31, 300):
                if (mems_oracle.vector(s, e, a, 0, end, cap, n, **mode) == cap).any():
                    continue
                b, q = mems_oracle.matches(s, e, a, 0, end, cap, n, min_len=min_len, **mode)
                got = mems_oracle.merge(b, q)                    # a match is not clipped at the window's end: compare the bases before it
                assert np.array_equal(got[0], want[0]) and np.array_equal(np.minimum(got[1], end), np.minimum(want[1], end)), (index, mode, min_len, cap)
                unions += 1
    assert expanded and unions


# ---------------------------------------------------------------------------------------
# the host-side merge of `-u`
# ---------------------------------------------------------------------------------------
def test_the_host_side_merge():
    from memo_amd import mems

    def merged(pairs):
        arr = np.asarray(pairs, np.int64).reshape(-1, 2)
        b, e = mems.merge(arr[:, 0], arr[:, 1])
        assert b.dtype == np.int64 and e.dtype == np.int64
        want = mems_oracle.merge(arr[:, 0], arr[:, 1])
        assert np.array_equal(b, want[0]) and np.array_equal(e, want[1])
        return list(zip(b.tolist(), e.tolist()))
    assert merged([]) == [] and merged([(3, 9)]) == [(3, 9)]                                       # none; one interval
    assert merged([(0, 5), (5, 8), (9, 12)]) == [(0, 8), (9, 12)]                                  # abutting intervals are one
    assert merged([(0, 5), (4, 8)]) == [(0, 8)] and merged([(0, 5), (6, 8)]) == [(0, 5), (6, 8)]
    assert merged([(0, 20), (2, 5), (6, 9), (19, 21), (22, 23)]) == [(0, 21), (22, 23)]            # nested intervals
    assert merged([(0, 20), (2, 5), (20, 20)]) == [(0, 20)]
    assert merged([(2 ** 40, 2 ** 40 + 3), (2 ** 40 + 3, 2 ** 40 + 4)]) == [(2 ** 40, 2 ** 40 + 4)]
    rng = np.random.default_rng(9)
    for _ in range(50):
        b = np.sort(rng.integers(0, 300, 40))
        merged(np.stack([b, b + rng.integers(0, 12, 40)], axis=1))
    # a plane's boundaries: pairs, an odd count ends at L; widened on the right and merged
    assert [x.tolist() for x in mems.band_intervals([], 10)] == [[], []]
    assert [x.tolist() for x in mems.band_intervals([0, 2, 3, 4, 9], 10)] == [[0, 3, 9], [2, 4, 10]]
    assert [x.tolist() for x in mems.band_intervals([0, 2, 3, 4, 9], 10, widen=1)] == [[0, 9], [5, 11]]
    assert [x.tolist() for x in mems.band_intervals([0, 2, 3, 4, 9], 10, widen=30)] == [[0], [40]]
