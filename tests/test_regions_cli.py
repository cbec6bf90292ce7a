"""`memo regions` without a GPU: the command line (usage bytes, getopts handling, what is refused before any device call), the
bytes of the sub-commands the reference defines, and the two host emitters against a formatter written in Python."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import golden_util as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "memo")
FAR = 2 ** 32 + 5


def _fixture(name):
    return open(os.path.join(G.GOLD, "cli", name), "rb").read()


def _memo(*argv, env=None):
    return subprocess.run([sys.executable, EXE, *argv], capture_output=True, timeout=120, env=dict(os.environ, **(env or {})))


@pytest.fixture(scope="module")
def memo():
    import memo_amd
    memo_amd.build()
    memo_amd.lib()
    return memo_amd


def test_usage_bytes():
    from memo_amd import regions_cli
    usage = _fixture("memo_regions_usage.txt")
    assert usage == regions_cli.USAGE.encode() and usage.startswith(b"\nMEMO regions - ") and usage.endswith(b"\n\n")
    for argv in ((), ("-h",)):
        r = _memo("regions", *argv)
        assert (r.returncode, r.stdout, r.stderr) == (0, usage, b""), argv
    for flag in (b"-b [FILE]", b"-k [INT]", b"-n [INT]", b"-r [CHR:START-END]", b"-o [FILE]", b"-t [INT]", b"-T [INT]", b"  -m  "):
        assert flag in usage


def test_illegal_option_prints_getopts_message_then_usage():
    usage = _fixture("memo_regions_usage.txt")
    r = _memo("regions", "-x")
    assert r.returncode == 0 and r.stdout == usage and r.stderr.endswith(b": illegal option -- x\n")
    r = _memo("regions", "-n", "5", "-t")
    assert r.returncode == 0 and r.stdout == usage and r.stderr.endswith(b": option requires an argument -- t\n")


def test_the_reference_sub_commands_print_what_they_printed():
    for argv, fixture in (([], "memo_usage.txt"), (["-h"], "memo_usage.txt"), (["query"], "memo_query_usage.txt"),
                          (["query", "-h"], "memo_query_usage.txt"), (["bogus"], "memo_bogus.txt")):
        r = _memo(*argv)
        assert r.returncode == 0 and r.stdout == _fixture(fixture), argv
    assert b"regions" not in _fixture("memo_usage.txt")          # the reference's text: the sub-command is documented in the README


REFUSALS = [
    (("-m", "-t", "3"), None, b"-m cannot be combined with -t / -T"),
    (("-m", "-T", "3"), None, b"-m cannot be combined with -t / -T"),
    (("-t", "6"), None, b"-t must be an integer in [0, 5]"),
    (("-t", "-1"), None, b"-t must be an integer in [0, 5]"),
    (("-t", "2.5"), None, b"-t must be an integer in [0, 5]"),
    (("-T", "six"), None, b"-T must be an integer in [0, 5]"),
    (("-T", "6"), None, b"-T must be an integer in [0, 5]"),
    (("-t", "4", "-T", "3"), None, b"-t 4 is above -T 3"),
    ((), {"WORLD_SIZE": "2"}, b"sharded launch"),
    ((), {"MEMO_FORCE_SHARDED": "1"}, b"sharded launch"),
]


@pytest.mark.parametrize("extra,env,message", REFUSALS)
def test_refusals_before_any_device_call(extra, env, message, tmp_path):
    """(-b names no file: a refusal that came after the index was opened would be another message)"""
    out = str(tmp_path / "never.bed")
    r = _memo("regions", "-b", str(tmp_path / "no.parquet"), "-r", "ref_1:0-20", "-k", "3", "-n", "5", "-o", out, *extra, env=env)
    assert r.returncode == 1 and r.stdout == b"MEMO - regions\n"
    assert r.stderr.startswith(b"memo regions: ") and message in r.stderr and r.stderr.count(b"\n") == 1
    assert os.listdir(tmp_path) == []


def test_missing_flags_are_named(tmp_path):
    r = _memo("regions", "-b", "x.parquet", "-k", "3")
    assert r.returncode == 2 and r.stdout == b"MEMO - regions\n" and r.stderr == b"memo regions: -r, -n, -o required\n"


def test_names_are_exported(memo):
    from memo_amd import regions
    assert memo.runs is regions.runs and memo.membership_runs is regions.membership_runs and memo.region_runs is regions.region_runs
    assert regions.tile() > 0 and regions.tile(1) > 0 and regions.tile(2) > 0 and regions.tile(5) > 0


# ---------------------------------------------------------------------------------------
# the emitters
# ---------------------------------------------------------------------------------------
def _ends(starts, L, step=1):
    return [starts[i + 1] if i + 1 < len(starts) else L for i in range(0, len(starts), step)]


def format_runs(record, qs, L, starts, values):
    starts = [int(s) for s in starts]
    if values is None:
        return "".join(f"{record}\t{qs + s}\t{qs + e}\n" for s, e in zip(starts[0::2], _ends(starts, L, 2)))
    return "".join(f"{record}\t{qs + s}\t{qs + e}\t{int(v)}\n" for s, e, v in zip(starts, _ends(starts, L), values))


def format_membership_runs(record, qs, L, starts, run_bits, num_docs):
    starts = [int(s) for s in starts]
    return "".join(f"{record}\t{qs + s}\t{qs + e}\t" + "".join(str((int(row[g >> 5]) >> (g & 31)) & 1) for g in range(num_docs)) + "\n"
                   for s, e, row in zip(starts, _ends(starts, L), run_bits))


def _emit_runs(memo, record, qs, L, starts, values, cap=None):
    """(bytes needed, the buffer of `cap` bytes as the call left it)"""
    s = np.ascontiguousarray(starts, np.int64)
    v = None if values is None else np.ascontiguousarray(values, np.uint16)
    need = memo.lib().memo_emit_runs(record.encode(), qs, L, s.ctypes.data, None if v is None else v.ctypes.data, len(s), None, 0)
    buf = np.full(need if cap is None else cap, 0x7E, np.uint8)
    got = memo.lib().memo_emit_runs(record.encode(), qs, L, s.ctypes.data, None if v is None else v.ctypes.data, len(s),
                                    buf.ctypes.data, len(buf))
    assert got == need
    return need, buf.tobytes()


RUN_CASES = [
    ("no runs", 0, 0, [], []),
    ("one run", 0, 26, [0], [5]),
    ("values 0 and 65535", 7, 1000, [0, 10, 999], [0, 65535, 0]),
    ("every digit count", 99, 200000, [0, 9, 10, 99, 100, 999, 1000, 9999, 10000, 99999, 100000], [0, 9, 10, 99, 100, 999, 1000, 9999, 10000, 65534, 3]),
    ("past 2^32", FAR, 3 * 10 ** 9, [0, 1, 2 ** 31 - 6, 2 ** 31 - 5, 2 * 10 ** 9], [1, 2, 3, 4, 5]),
]


@pytest.mark.parametrize("name,qs,L,starts,values", RUN_CASES, ids=[c[0] for c in RUN_CASES])
def test_emit_runs_equals_the_python_formatter(memo, name, qs, L, starts, values):
    want = format_runs("chr_1", qs, L, starts, values).encode()
    need, text = _emit_runs(memo, "chr_1", qs, L, starts, values)
    assert need == len(want) and text == want
    if name == "no runs":
        assert want == b""
    if name == "past 2^32":
        assert want.startswith(b"chr_1\t4294967301\t4294967302\t1\n") and want.endswith(b"\t%d\t5\n" % (FAR + 3 * 10 ** 9))


@pytest.mark.parametrize("starts", [[], [3], [0, 4], [0, 4, 9], [2, 4, 9, 11], [5, 6, 7, 8, 19]], ids=lambda s: f"{len(s)}_boundaries")
@pytest.mark.parametrize("qs", [0, FAR])
def test_emit_band_intervals_odd_and_even(memo, starts, qs):
    """2j opens, 2j + 1 closes; an odd count: the last interval ends at L"""
    L = 20
    want = format_runs("r", qs, L, starts, None).encode()
    assert want.count(b"\n") == (len(starts) + 1) // 2
    if len(starts) & 1:
        assert want.endswith(b"\t%d\n" % (qs + L))
    need, text = _emit_runs(memo, "r", qs, L, starts, None)
    assert need == len(want) and text == want


@pytest.mark.parametrize("num_docs", [1, 33, 500])
def test_emit_membership_runs_equals_the_python_formatter(memo, num_docs):
    W = (num_docs + 31) // 32
    rng = np.random.default_rng(num_docs)
    for qs, L, starts in ((0, 0, []), (0, 9, [0]), (FAR, 10 ** 6, [0, 1, 31, 32, 33, 4096, 999_999])):
        rows = rng.integers(0, 2 ** 32, (len(starts), W), dtype=np.uint64).astype(np.uint32)
        if num_docs & 31 and len(starts):
            rows[:, -1] &= np.uint32((1 << (num_docs & 31)) - 1)
        if len(starts):
            rows[0] = 0
            rows[0, 0], rows[0, -1] = 1, rows[0, -1] | np.uint32(1 << ((num_docs - 1) & 31))   # genome 0 first, genome num_docs - 1 last
        want = format_membership_runs("ref_1", qs, L, starts, rows, num_docs).encode()
        s = np.ascontiguousarray(starts, np.int64)
        call = lambda buf, cap: memo.lib().memo_emit_membership_runs(b"ref_1", qs, L, s.ctypes.data, rows.ctypes.data, len(s), num_docs, buf, cap)  # noqa: E731
        need = call(None, 0)
        buf = np.full(need, 0x7E, np.uint8)
        assert call(buf.ctypes.data, need) == need == len(want) and buf.tobytes() == want
        if len(starts):
            line = want.split(b"\n")[0].split(b"\t")
            assert len(line[3]) == num_docs and line[3][:1] == b"1" and line[3][-1:] == b"1"
            small = np.full(need - 1, 0x7E, np.uint8)                  # one byte too small: nothing written, the size still returned
            assert call(small.ctypes.data, need - 1) == need and bytes(small) == b"\x7e" * (need - 1)


def test_a_cap_one_byte_too_small_writes_nothing(memo):
    starts, values = [0, 5, 6, 100], [3, 0, 65535, 7]
    for vals in (values, None):
        need, _ = _emit_runs(memo, "chr_1", FAR, 4000, starts, vals)
        assert need > 0
        got, buf = _emit_runs(memo, "chr_1", FAR, 4000, starts, vals, cap=need - 1)
        assert got == need and buf == b"\x7e" * (need - 1)


def test_python_wrappers_return_the_same_bytes(memo):
    from memo_amd import regions
    starts, values = np.array([0, 4, 9], np.int64), np.array([5, 0, 2], np.uint16)
    assert bytes(regions.emit_runs("c", 10, 12, starts, values)) == format_runs("c", 10, 12, starts, values).encode()
    assert bytes(regions.emit_runs("c", 10, 12, starts)) == b"c\t10\t14\nc\t19\t22\n"
    rows = np.array([[0b0110], [0b1001]], np.uint32)
    assert bytes(regions.emit_membership_runs("c", 0, 7, starts[:2], rows, 4)) == b"c\t0\t4\t0110\nc\t4\t7\t1001\n"
    begin, end = regions.band_intervals(starts, 12)
    assert begin.tolist() == [0, 9] and end.tolist() == [4, 12]
    assert regions.expand(starts, values, 12).tolist() == [5] * 4 + [0] * 5 + [2] * 3
