"""`memo tracks` without a GPU: the command line (usage bytes, getopts handling, what is refused before the library is even
loaded) and the host half of memo_amd/tracks.py (the bin edges, fractions, the text of a table, the labels of -g) against literals."""
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
    from memo_amd import tracks_cli
    usage = _fixture("memo_tracks_usage.txt")
    assert usage == tracks_cli.USAGE.encode() and usage.startswith(b"\nMEMO tracks - ") and usage.endswith(b"\n\n")
    for argv in ((), ("-h",)):
        r = _memo("tracks", *argv)
        assert (r.returncode, r.stdout, r.stderr) == (0, usage, b""), argv
    for flag in (b"-b [FILE]", b"-k [INT]", b"-n [INT]", b"-r [CHR:START-END]", b"-o [FILE]", b"-o [FILE].tsv", b"-B [INT]", b"  -f  ",
                 b"-g [FILE]", b"-d [INT]", b"[500]", b"[600]"):
        assert flag in usage
    assert b"MEMBERSHIP" in usage and b"conservation index" in usage          # the index must be a membership index: said here


def test_illegal_option_prints_getopts_message_then_usage():
    usage = _fixture("memo_tracks_usage.txt")
    r = _memo("tracks", "-x")
    assert r.returncode == 0 and r.stdout == usage and r.stderr.endswith(b": illegal option -- x\n")
    r = _memo("tracks", "-n", "5", "-B")
    assert r.returncode == 0 and r.stdout == usage and r.stderr.endswith(b": option requires an argument -- B\n")


def test_the_reference_sub_commands_print_what_they_printed():
    for argv, fixture in (([], "memo_usage.txt"), (["-h"], "memo_usage.txt"), (["bogus"], "memo_bogus.txt")):
        r = _memo(*argv)
        assert r.returncode == 0 and r.stdout == _fixture(fixture), argv
    assert b"tracks" not in _fixture("memo_usage.txt")          # the reference's text: the sub-command is documented in the README


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
                                (("-n", "5", "-B", "many"), None, b"invalid literal for int()"),
                                (("-n", "5", "-d", "6e2"), None, b"invalid literal for int()"),
                                (("-n", "5", "-B", "0"), None, b"-B 0: the number of bins must be at least 1"),
                                (("-n", "5", "-B", "-3"), None, b"-B -3: the number of bins must be at least 1"),
                                (("-n", "5", "-g", four), None, b"names 4 genomes, -n says 5"),
                                (("-n", "5", "-g", str(tmp_path / "no.txt")), None, b"cannot read the genome list")):
        r = _memo("tracks", *common, *extra, env=env)
        assert r.returncode == 1 and r.stdout == b"MEMO - tracks\n", (extra, r.stderr)
        assert r.stderr.startswith(b"memo tracks: ") and message in r.stderr and r.stderr.count(b"\n") == 1, (extra, r.stderr)
        assert not os.path.exists(out)
    # the same command with nothing to refuse does reach the library, which is not there
    r = _memo("tracks", *common, "-n", "4", "-B", "4", "-g", four)
    assert r.returncode == 1 and not os.path.exists(out)
    assert b"Traceback" in r.stderr or b"memo tracks: " in r.stderr
    assert sorted(os.listdir(tmp_path)) == ["genomes.txt"]


def test_missing_flags_are_named():
    r = _memo("tracks", "-b", "x.parquet", "-k", "3")
    assert r.returncode == 2 and r.stdout == b"MEMO - tracks\n" and r.stderr == b"memo tracks: -r, -n, -o required\n"
    r = _memo("tracks", "-r", "ref_1:0-20", "-n", "5", "-o", "x", "-f")
    assert r.returncode == 2 and r.stderr == b"memo tracks: -b required\n"


def test_names_are_exported():
    import memo_amd
    from memo_amd import tracks
    assert memo_amd.bin_tracks is tracks.bin_tracks and memo_amd.region_tracks is tracks.region_tracks


def test_the_bin_edges_are_memo_views():
    from memo_amd import tracks, view
    assert tracks.region_edges(20, 4).tolist() == [0, 5, 10, 15, 20]
    assert tracks.region_edges(20, 3).tolist() == [0, 6, 13, 20]
    assert tracks.region_edges(1000, 7).tolist() == [0, 142, 285, 428, 571, 714, 857, 1000]      # floor(1000 i / 7)
    for positions, bins in ((20, 4), (20, 3), (1000, 7), (12345, 500), (500, 500), (1, 1)):
        edges = tracks.region_edges(positions, bins)
        assert edges.dtype == np.int64 and np.array_equal(edges, view.bin_edges(positions, bins))
        assert np.array_equal(edges, np.array(list(map(int, np.linspace(0, positions, bins + 1)))))          # the reference's rule, restated
        assert np.all(np.diff(edges) > 0)                                                                  # no bin is empty
    for positions, bins in ((20, 0), (20, -1), (20, 21), (1, 2)):
        with pytest.raises(ValueError) as exc:
            tracks.region_edges(positions, bins)
        assert str(bins) in str(exc.value) and str(positions) in str(exc.value)


def test_fractions_on_hand_made_counts():
    from memo_amd import tracks
    counts = np.array([[5, 5, 7], [3, 0, 2], [0, 1, 7]], np.uint64)
    f = tracks.fractions(counts, [0, 5, 10, 17])
    assert f.dtype == np.float64 and f.tolist() == [[1.0, 1.0, 1.0], [0.6, 0.0, 2 / 7], [0.0, 0.2, 1.0]]
    big = np.array([[2 ** 40]], np.uint64)                                     # uint64 in
    assert tracks.fractions(big, [10, 10 + 2 ** 41]).tolist() == [[0.5]]
    with pytest.raises(ZeroDivisionError):
        tracks.fractions(counts, [0, 5, 5, 17])


def test_format_tracks_against_literals():
    from memo_amd import tracks
    counts = np.array([[5, 5], [3, 2 ** 32 + 7]], np.uint64)
    assert tracks.format_tracks(counts, 0, [0, 5, 10]) == "genome\t0-5\t5-10\n0\t5\t5\n1\t3\t4294967303\n"
    assert tracks.format_tracks(counts, 1000, [0, 5, 10]) == "genome\t1000-1005\t1005-1010\n0\t5\t5\n1\t3\t4294967303\n"
    assert tracks.format_tracks(counts, 0, [0, 5, 10], ["pivot", "g1"]) == "genome\t0-5\t5-10\npivot\t5\t5\ng1\t3\t4294967303\n"
    f = np.array([[1.0, 1 / 3], [0.0, 0.6]])
    assert tracks.format_tracks(f, 7, [0, 3, 8]) == "genome\t7-10\t10-15\n0\t1.0\t0.3333333333333333\n1\t0.0\t0.6\n"
    assert tracks.format_tracks(np.zeros((1, 1), np.uint64), 0, [0, 1]) == "genome\t0-1\n0\t0\n"
    with pytest.raises(ValueError):
        tracks.format_tracks(counts, 0, [0, 5, 10], ["only one"])
    with pytest.raises(ValueError):
        tracks.format_tracks(counts, 0, [0, 5, 10, 15])


def test_labels_are_read_as_memo_matrix_reads_them(tmp_path):
    from memo_amd import matrix_cli, tracks_cli
    path = _genome_list(tmp_path, ["ref/pivot.fa", "", "other/g1.fa.gz", "g2.fasta"])
    assert tracks_cli.read_labels(path, 3) == ["pivot", "g1", "g2"] == matrix_cli.read_labels(path, 3)      # first line the pivot: genome 0
