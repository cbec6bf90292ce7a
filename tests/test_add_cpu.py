"""`memo add` without a GPU: the definition (tests/add_oracle.py) against the example's golden indexes and against the closed form of
`memo query -m` (oracle.memo_oracle.np_membership), and the command line: the usage bytes and every refusal, with the library pointed at
a file that is not there -- no refusal may need the device."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import add_oracle
from tests import golden_util as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "memo")
FASTA = [os.path.join(G.GOLD, "example_fa", f"ref_{i}.fa") for i in range(1, 6)]


def _fixture(name):
    return open(os.path.join(G.GOLD, "cli", name), "rb").read()


def _memo(*argv, env=None):
    """bin/memo with the library pointed at a file that is not there: a call that touched _lib.lib() would end in an ImportError's
    traceback, not in the refusal"""
    env = dict(os.environ, MEMO_AMD_LIB=os.path.join(ROOT, "no", "such", "libmemo_amd.so"), **(env or {}))
    return subprocess.run([sys.executable, EXE, *argv], capture_output=True, timeout=120, env=env)


@pytest.fixture(scope="module")
def example():
    """(pivot [(name, sequence)], the four other genomes as lists of sequences)"""
    from memo_amd.build_index import read_fasta
    files = [read_fasta(p) for p in FASTA]
    return files[0], [[s for _, s in f] for f in files[1:]]


def _golden(order):
    return G.index_columns("example_cons.parquet" if order else "example_memb.parquet", "ref_1")


def _same(got, want):
    return len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want))


# ---------------------------------------------------------------------------------------
# the identity the feature rests on, as tests of the oracle
# ---------------------------------------------------------------------------------------
def test_four_genomes_plus_the_fifth_are_the_committed_indexes(example):
    pivot, genomes = example
    four = add_oracle.built_rows(pivot, genomes[:3], order=False)
    assert len(four["ref_1"][0]) == 34
    # reading the four genomes' matching statistics back gives the first three DAP columns exactly
    seq = pivot[0][1]
    assert np.array_equal(add_oracle.matrix(*four["ref_1"], 4, seq, genomes[3:]), add_oracle.new_ms(seq, genomes))
    for order, count in ((False, 48), (True, 56)):
        names, *got = add_oracle.index_rows(pivot, four, 4, genomes[3:], order)
        assert len(got[0]) == count and set(names) == {"ref_1"} and _same(got, _golden(order)), order


def test_a_chain_of_additions_ends_at_the_same_indexes(example):
    pivot, genomes = example
    two = add_oracle.built_rows(pivot, genomes[:1], order=False)
    _, *three = add_oracle.index_rows(pivot, two, 2, genomes[1:2], False)                   # adding one
    assert _same(three, add_oracle.built_rows(pivot, genomes[:2], order=False)["ref_1"])
    for order in (False, True):
        _, *five = add_oracle.index_rows(pivot, {"ref_1": tuple(three)}, 3, genomes[2:], order)   # then two
        assert _same(five, _golden(order)), order
        _, *direct = add_oracle.index_rows(pivot, two, 2, genomes[1:], order)                # or three at once
        assert _same(direct, _golden(order)), order


@pytest.mark.parametrize("old,new", ((3, 1), (1, 1), (1, 3), (2, 2)))
def test_membership_bits_of_the_grown_index(example, old, new):
    """bit g of `memo query -m -k k`: the input's bit for an old genome, k <= new[p][j] for new genome j"""
    from oracle import memo_oracle as O
    pivot, genomes = example
    seq = pivot[0][1]
    L, n = len(seq), old + 1
    source = add_oracle.built_rows(pivot, genomes[:old], order=False)["ref_1"]
    added = genomes[old:old + new]
    s, e, a = add_oracle.rows(*source, n, seq, added, order=False)
    fresh = add_oracle.new_ms(seq, added)
    checked = 0
    for k in range(1, 41):
        before = O.bits_to_matrix(O.np_membership(*source, 0, L, k, n), n)
        after = O.bits_to_matrix(O.np_membership(s, e, a, 0, L, k, n + new), n + new)
        assert np.array_equal(after[:, :n], before), k
        assert np.array_equal(after[:, n:], (k <= fresh).astype(np.uint8)), k
        checked += int(after[:, n:].sum())
    assert checked > 0


# ---------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------
def test_usage_bytes():
    from memo_amd import add_cli
    usage = _fixture("memo_add_usage.txt")
    assert usage == add_cli.USAGE.encode() and usage.startswith(b"\nMEMO add - ") and usage.endswith(b"\n\n")
    for argv in ((), ("-h",)):
        r = _memo("add", *argv)
        assert (r.returncode, r.stdout, r.stderr) == (0, usage, b""), argv
    for flag in (b"-b [FILE]", b"-n [INT]", b"-g [FILE]", b"-o [FILE]", b"-c [FILE]"):
        assert flag in usage
    r = _memo("add", "-k", "31")
    assert r.returncode == 0 and r.stdout == usage and r.stderr.endswith(b": illegal option -- k\n")
    r = _memo("add", "-b", "x", "-n")
    assert r.returncode == 0 and r.stdout == usage and r.stderr.endswith(b": option requires an argument -- n\n")


def test_the_reference_sub_commands_print_what_they_printed():
    for argv, fixture in (([], "memo_usage.txt"), (["-h"], "memo_usage.txt"), (["bogus"], "memo_bogus.txt")):
        r = _memo(*argv)
        assert r.returncode == 0 and r.stdout == _fixture(fixture), argv
    assert b"add" not in _fixture("memo_usage.txt")            # the reference's text: the sub-command is documented in the README
    assert _memo("convert").stdout == _fixture("memo_convert_usage.txt")         # `memo convert` is as it was


def test_missing_flags_are_named():
    r = _memo("add", "-b", "x.parquet", "-o", "y")
    assert r.returncode == 2 and r.stdout == b"MEMO - add\n" and r.stderr == b"memo add: -n, -g required\n"
    r = _memo("add", "-n", "5", "-g", "list", "-c", "x")
    assert r.returncode == 2 and r.stderr == b"memo add: -b required\n"
    r = _memo("add", "-b", "x.parquet", "-n", "5", "-g", "list")
    assert r.returncode == 2 and r.stdout == b"MEMO - add\n" and r.stderr == b"memo add: -o or -c required\n"


def _write(path, f0, s, e, a):
    import pyarrow as pa
    import pyarrow.parquet as pq
    pq.write_table(pa.table({"f0": pa.array(f0, pa.utf8()), "f1": pa.array(s, pa.int64()), "f2": pa.array(e, pa.int64()),
                             "f3": pa.array(a, pa.int64())}), path)


def test_refusals_before_the_library_is_touched_and_before_anything_is_written(tmp_path):
    memb = os.path.join(G.GOLD, "example_memb.parquet")
    out, cons = str(tmp_path / "never.parquet"), str(tmp_path / "never_cons.parquet")

    def listed(name, *paths):
        path = str(tmp_path / name)
        open(path, "w").write("".join(p + "\n" for p in paths))
        return path

    def fasta(name, data):
        path = str(tmp_path / name)
        open(path, "wb").write(data)
        return path
    seq = open(FASTA[0], "rb").read().split(b"\n")[1]
    assert len(seq) == 26
    good = listed("good.txt", FASTA[0], FASTA[1])
    three_new = listed("three.txt", FASTA[0], FASTA[1], FASTA[2], FASTA[3])
    other_name = listed("other_name.txt", fasta("other_name.fa", b">other\n" + seq + b"\n"), FASTA[1])
    one_more = listed("one_more.txt", fasta("one_more.fa", b">ref_1\n" + seq + b"\n>ref_9\nACGT\n"), FASTA[1])
    shorter = listed("shorter.txt", fasta("shorter.fa", b">ref_1\n" + seq[:-1] + b"\n"), FASTA[1])
    longer = listed("longer.txt", fasta("longer.fa", b">ref_1\n" + seq + b"A\n"), FASTA[1])
    twice = listed("twice.txt", fasta("twice.fa", b">ref_1\n" + seq + b"\n>ref_1\n" + seq + b"\n"), FASTA[1])
    gz_pivot = listed("gz_pivot.txt", fasta("pivot.fa.gz", b"\x1f\x8b\x08\x00rest"), FASTA[1])
    nul_pivot = listed("nul_pivot.txt", fasta("nul.fa", b">ref_1\nACG\0T\n"), FASTA[1])
    empty_record = listed("empty_record.txt", fasta("empty_record.fa", b">ref_1\n" + seq + b"\n>ref_2\n\n"), FASTA[1])
    no_records = listed("no_records.txt", fasta("no_records.fa", b"\n"), FASTA[1])
    gz_new = listed("gz_new.txt", FASTA[0], fasta("new.fa.gz", b"\x1f\x8b\x08\x00rest"))
    nul_new = listed("nul_new.txt", FASTA[0], FASTA[1], fasta("nul_new.fa", b">x\nAC\0GT\n"))
    no_new = listed("no_new.txt", FASTA[0], str(tmp_path / "no.fa"))
    pivot_only = listed("pivot_only.txt", FASTA[0])
    far = str(tmp_path / "far.parquet")
    _write(far, ["ref_1", "ref_1"], [5, 2 ** 31], [9, 2 ** 31 + 4], [1, 1])
    long = str(tmp_path / "long.parquet")
    _write(long, ["ref_1", "ref_1"], [5, 2 ** 30], [9, 2 ** 30 + 4], [1, 1])
    copy = str(tmp_path / "copy.parquet")
    with open(copy, "wb") as fh:
        fh.write(open(memb, "rb").read())
    before = sorted(os.listdir(tmp_path))
    ok = ("-b", memb, "-n", "5", "-g", good, "-o", out, "-c", cons)

    def change(**flags):
        argv = dict(zip(ok[::2], ok[1::2]))
        for flag, value in flags.items():
            flag = "-" + flag
            if value is None:
                del argv[flag]
            else:
                argv[flag] = value
        return tuple(x for pair in argv.items() for x in pair)
    for argv, env, message in ((ok, {"WORLD_SIZE": "2"}, b"sharded launch"),
                               (ok, {"MEMO_FORCE_SHARDED": "1"}, b"sharded launch"),
                               (change(n="five"), None, b"invalid literal for int()"),
                               (change(n="1"), None, b"-n must be in [2, 2047]"),
                               (change(n="2048", o=None), None, b"-n must be in [2, 2047]"),
                               (change(n="2046", g=three_new), None, b"the limit is 2048"),
                               # everything convert.scan_index refuses
                               (change(n="4"), None, b"has annot 4 outside [1, 3]"),
                               (change(n="4", c=None), None, b"-n value is probably wrong"),
                               (change(b=os.path.join(G.GOLD, "rnd_negoverlap.parquet"), n="12"), None, b"ends before it starts"),
                               (change(b=far, n="2"), None, b"above 2^31 - 1"),
                               (change(b=long, n="2", o=None), None, b"above 2^30 - 1"),
                               (change(b=str(tmp_path / "no.parquet")), None, b"no.parquet"),
                               # the pivot held against the index
                               (change(g=other_name), None, b"'ref_1' of " + memb.encode() + b" is not a record of the pivot"),
                               (change(g=one_more), None, b"pivot record 'ref_9'"),
                               (change(g=one_more, o=None), None, b"has no rows in"),
                               (change(g=shorter), None, b"the largest row start in " + memb.encode() + b" is 26, the record in"),
                               (change(g=shorter, c=None), None, b"has 25 positions"),
                               (change(g=longer), None, b"has 27 positions"),
                               (change(g=twice), None, b"occurs twice"),
                               # everything read_fasta, pivot_layout and the list reader refuse
                               (change(g=gz_pivot), None, b"gzip-compressed FASTA is not supported"),
                               (change(g=nul_pivot), None, b"holds a NUL byte"),
                               (change(g=empty_record), None, b"pivot record 'ref_2' has length 0"),
                               (change(g=no_records), None, b"the pivot has no records"),
                               (change(g=gz_new), None, b"new.fa.gz: gzip-compressed FASTA is not supported"),
                               (change(g=nul_new), None, b"nul_new.fa: holds a NUL byte"),
                               (change(g=no_new), None, b"no.fa"),
                               (change(g=pivot_only), None, b"needs the pivot and at least one more genome"),
                               (change(g=str(tmp_path / "no.txt")), None, b"cannot read the genome list"),
                               # the outputs
                               (change(b=copy, o=copy), None, b"is the input file"),
                               (change(b=copy, c=os.path.join(str(tmp_path), ".", "copy.parquet")), None, b"is the input file"),
                               (change(b=copy, o=None, c=copy), None, b"is the input file"),
                               (change(c=out), None, b"is named for both outputs"),
                               (change(c=os.path.join(str(tmp_path), ".", "never.parquet")), None, b"is named for both outputs"),
                               # the settings
                               (ok, {"MEMO_ADD_SLICE": "0"}, b"MEMO_ADD_SLICE must be"),
                               (ok, {"MEMO_ADD_BATCH": "many"}, b"MEMO_ADD_BATCH must be"),
                               (ok, {"MEMO_INDEX_PIECE_BYTES": "1"}, b"MEMO_INDEX_PIECE_BYTES"),
                               (ok, {"MEMO_INDEX_DAP_LAYOUT": "sparse"}, b"MEMO_INDEX_DAP_LAYOUT"),
                               (ok, {"MEMO_INDEX_WALK_BUDGET": "-1"}, b"MEMO_INDEX_WALK_BUDGET")):
        r = _memo("add", *argv, env=env)
        assert r.returncode == 1 and r.stdout == b"MEMO - add\n", (argv, env, r.stderr)
        assert r.stderr.startswith(b"memo add: ") and message in r.stderr and r.stderr.count(b"\n") == 1, (argv, env, r.stderr)
        assert sorted(os.listdir(tmp_path)) == before, (argv, env)
    assert open(copy, "rb").read() == open(memb, "rb").read()
    # the same command with nothing to refuse does reach the library, which is not there
    for argv in (ok, change(o=None), change(c=None), change(g=three_new)):
        r = _memo("add", *argv)
        assert r.returncode == 1 and (b"Traceback" in r.stderr or b"memo add: " in r.stderr), (argv, r.stderr)
        assert b"must be" not in r.stderr and b"libmemo_amd.so" in r.stderr, (argv, r.stderr)
        assert sorted(os.listdir(tmp_path)) == before


def test_an_over_long_pivot_record_is_refused_on_the_host(tmp_path, monkeypatch):
    """pivot_layout's limit is 2^30 - 1 positions; the check is reached with the limit lowered, not with a gigabyte of FASTA"""
    from memo_amd import add, build_index
    monkeypatch.setattr(build_index, "MAX_RECORD", 25)
    with pytest.raises(build_index.FastaError, match=r"pivot record 'ref_1' has 26 positions \(the limit is 25\)"):
        add._match_pivot(os.path.join(G.GOLD, "example_memb.parquet"), 5, FASTA[0])


def test_the_library_functions_refuse_what_the_command_refuses(example):
    from memo_amd import add
    pivot, genomes = example
    seq = pivot[0][1]
    s, e, a = G.index_columns("example_memb.parquet", "ref_1")
    new = genomes[:1]
    for bad, message in ((lambda: add.rows(s, e, a, 1, seq, new), "n_docs must be in"), (lambda: add.rows(s, e, a, 2048, seq, new), "n_docs must be in"),
                         (lambda: add.rows(s, e, a, 5, seq, []), "no new genome"),
                         (lambda: add.rows(s, e, a, 2040, seq, [[b"A"]] * 9), "the limit is 2048"),
                         (lambda: add.rows(s, e, a, 4, seq, new), "annot 4 outside"), (lambda: add.rows(s, s - 1, a, 5, seq, new), "ends before it starts"),
                         (lambda: add.rows(s, e, a, 5, seq[:-1], new), "the record has 25 positions"),
                         (lambda: add.rows([], [], [], 5, seq, new), "no rows"),
                         (lambda: add.rows(s, e, a[:-1], 5, seq, new), "differ in length"),
                         (lambda: add.rows(s, e, a, 5, seq, new, slice_positions=0), "slice_positions must be"),
                         (lambda: add.rows(s, e, a, 5, seq, new, batch_positions=-3), "batch_positions must be"),
                         (lambda: add.dap(np.zeros((3, 8), np.uint32), np.zeros((4, 2), np.int32), 0, 5, 8), "new has 4 rows for 5 positions"),
                         (lambda: add.dap(np.zeros((1, 8), np.uint32), np.zeros((4, 2), np.int32), 0, 4, 8), "n_docs must be in"),
                         (lambda: add.dap(np.zeros((3, 8), np.uint32), np.zeros((4, 0), np.int32), 0, 4, 8), "no new genome"),
                         (lambda: add.add_index("x.parquet", "list.txt", 5), "no output")):
        with pytest.raises(ValueError, match=message):
            bad()
    import memo_amd
    assert memo_amd.add is add and memo_amd.add_index is add.add_index
