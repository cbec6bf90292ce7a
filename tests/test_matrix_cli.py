"""`memo matrix` without a GPU: the command line (usage bytes, getopts handling, what is refused before the library is even
loaded) and the host half of memo_amd/matrix.py (Jaccard distances, the text of a matrix, the labels of -g) against literals."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import golden_util as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "memo")


def _fixture(name):
    return open(os.path.join(G.GOLD, "cli", name), "rb").read()


def _memo(*argv, env=None):
    """bin/memo with the library pointed at a file that is not there: a call that touched _lib.lib() would end in an ImportError's
    traceback, not in the refusal"""
    env = dict(os.environ, MEMO_AMD_LIB=os.path.join(ROOT, "no", "such", "libmemo_amd.so"), **(env or {}))
    return subprocess.run([sys.executable, EXE, *argv], capture_output=True, timeout=120, env=env)


def test_usage_bytes():
    from memo_amd import matrix_cli
    usage = _fixture("memo_matrix_usage.txt")
    assert usage == matrix_cli.USAGE.encode() and usage.startswith(b"\nMEMO matrix - ") and usage.endswith(b"\n\n")
    for argv in ((), ("-h",)):
        r = _memo("matrix", *argv)
        assert (r.returncode, r.stdout, r.stderr) == (0, usage, b""), argv
    for flag in (b"-b [FILE]", b"-k [INT]", b"-n [INT]", b"-r [CHR:START-END]", b"-o [FILE]", b"  -j  ", b"-g [FILE]"):
        assert flag in usage
    assert b"MEMBERSHIP" in usage and b"conservation index" in usage          # the index must be a membership index: said here


def test_illegal_option_prints_getopts_message_then_usage():
    usage = _fixture("memo_matrix_usage.txt")
    r = _memo("matrix", "-x")
    assert r.returncode == 0 and r.stdout == usage and r.stderr.endswith(b": illegal option -- x\n")
    r = _memo("matrix", "-n", "5", "-g")
    assert r.returncode == 0 and r.stdout == usage and r.stderr.endswith(b": option requires an argument -- g\n")


def test_the_reference_sub_commands_print_what_they_printed():
    for argv, fixture in (([], "memo_usage.txt"), (["-h"], "memo_usage.txt"), (["bogus"], "memo_bogus.txt")):
        r = _memo(*argv)
        assert r.returncode == 0 and r.stdout == _fixture(fixture), argv
    assert b"matrix" not in _fixture("memo_usage.txt")          # the reference's text: the sub-command is documented in the README


def _genome_list(tmp_path, lines):
    path = tmp_path / "genomes.txt"
    path.write_text("".join(ln + "\n" for ln in lines))
    return str(path)


def test_refusals_before_the_library_is_touched(tmp_path):
    """(-b names no file and the library path names none: a refusal that came later would be another message)"""
    out = str(tmp_path / "never.tsv")
    common = ("-b", str(tmp_path / "no.parquet"), "-r", "ref_1:0-20", "-k", "3", "-o", out)
    four = _genome_list(tmp_path, ["a.fa", "", "b.fa", "c.fa", "  ", "d.fa"])
    for extra, env, message in ((("-n", "5"), {"WORLD_SIZE": "2"}, b"sharded launch"),
                                (("-n", "5"), {"MEMO_FORCE_SHARDED": "1"}, b"sharded launch"),
                                (("-n", "five"), None, b"invalid literal for int()"),
                                (("-n", "5", "-k", "3.5"), None, b"invalid literal for int()"),
                                (("-n", "5", "-g", four), None, b"names 4 genomes, -n says 5"),
                                (("-n", "5", "-g", str(tmp_path / "no.txt")), None, b"cannot read the genome list")):
        r = _memo("matrix", *common, *extra, env=env)
        assert r.returncode == 1 and r.stdout == b"MEMO - matrix\n", (extra, r.stderr)
        assert r.stderr.startswith(b"memo matrix: ") and message in r.stderr and r.stderr.count(b"\n") == 1, (extra, r.stderr)
        assert not os.path.exists(out)
    # the same command with nothing to refuse does reach the library, which is not there
    r = _memo("matrix", *common, "-n", "4", "-g", four)
    assert r.returncode == 1 and not os.path.exists(out)
    assert b"Traceback" in r.stderr or b"memo matrix: " in r.stderr


def test_missing_flags_are_named():
    r = _memo("matrix", "-b", "x.parquet", "-k", "3")
    assert r.returncode == 2 and r.stdout == b"MEMO - matrix\n" and r.stderr == b"memo matrix: -r, -n, -o required\n"
    r = _memo("matrix", "-r", "ref_1:0-20", "-n", "5", "-o", "x", "-j")
    assert r.returncode == 2 and r.stderr == b"memo matrix: -b required\n"


def test_names_are_exported():
    import memo_amd
    from memo_amd import matrix
    assert memo_amd.cooccurrence is matrix.cooccurrence and memo_amd.region_matrix is matrix.region_matrix


def test_jaccard_on_hand_made_counts():
    from memo_amd import matrix
    # genome 0 holds 10 positions, genome 1 five of them and one of its own, genome 2 nothing
    counts = np.array([[10, 5, 0], [5, 6, 0], [0, 0, 0]], np.uint64)
    d = matrix.jaccard(counts)
    assert d.dtype == np.float64 and d.shape == (3, 3)
    want = [[0.0, 1 - 5 / 11, 1.0], [1 - 5 / 11, 0.0, 1.0], [1.0, 1.0, 0.0]]          # [2][2]: an empty union is distance 0.0
    assert d.tolist() == want
    assert matrix.jaccard(np.zeros((2, 2), np.uint64)).tolist() == [[0.0, 0.0], [0.0, 0.0]]
    big = np.array([[2 ** 40, 2 ** 39], [2 ** 39, 2 ** 39]], np.uint64)              # uint64 in, no wrap in the union
    assert matrix.jaccard(big).tolist() == [[0.0, 0.5], [0.5, 0.0]]


def test_format_matrix_against_literals():
    from memo_amd import matrix
    counts = np.array([[20, 3], [3, 2 ** 32 + 7]], np.uint64)
    assert matrix.format_matrix(counts) == "20\t3\n3\t4294967303\n"
    assert matrix.format_matrix(counts, ["pivot", "g1"]) == "\tpivot\tg1\npivot\t20\t3\ng1\t3\t4294967303\n"
    d = np.array([[0.0, 1 / 3], [1 / 3, 1.0]])
    assert matrix.format_matrix(d) == "0.0\t0.3333333333333333\n0.3333333333333333\t1.0\n"
    assert matrix.format_matrix(d, ["a", "b"]) == "\ta\tb\na\t0.0\t0.3333333333333333\nb\t0.3333333333333333\t1.0\n"
    assert matrix.format_matrix(np.zeros((1, 1), np.uint64)) == "0\n"
    with pytest.raises(ValueError):
        matrix.format_matrix(counts, ["only one"])


def test_labels_are_base_names_without_extension(tmp_path):
    from memo_amd import matrix_cli
    assert matrix_cli.label_of("/data/hprc/HG002.mat.fa") == "HG002.mat"
    assert matrix_cli.label_of("genomes/chm13.fasta.gz") == "chm13"
    assert matrix_cli.label_of("pivot") == "pivot"
    assert matrix_cli.label_of("  rel/dir.v2/g3.fna \n") == "g3"
    path = _genome_list(tmp_path, ["ref/pivot.fa", "", "other/g1.fa.gz", "g2.fasta"])
    assert matrix_cli.read_labels(path, 3) == ["pivot", "g1", "g2"]          # first line the pivot: genome 0
