"""`memo index` without a GPU: the command line (src/index.sh's usage text, getopts handling, refusals before
the device is touched), FASTA parsing, and the genome text the matching statistics are taken against."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "memo")
USAGE = open(os.path.join(ROOT, "tests", "golden", "cli", "memo_index_usage.txt"), "rb").read()


def _memo(*argv, cwd=None):
    return subprocess.run([sys.executable, EXE, "index", *argv], capture_output=True, cwd=cwd, timeout=120)


@pytest.mark.parametrize("argv", [[], ["-h"]])
def test_usage_bytes(argv):
    r = _memo(*argv)
    assert r.returncode == 0
    assert r.stdout == USAGE
    assert r.stderr == b""


def test_illegal_option_prints_getopts_message_then_usage():
    r = _memo("-x")
    assert r.returncode == 0
    assert r.stdout == USAGE
    assert r.stderr.endswith(b": illegal option -- x\n")
    r = _memo("-p", "x", "-g")
    assert r.returncode == 0 and r.stdout == USAGE
    assert r.stderr.endswith(b": option requires an argument -- g\n")


def test_missing_or_unreadable_genome_list(tmp_path):
    r = _memo("-p", "test", "-o", str(tmp_path))
    assert r.returncode != 0 and b"genome list" in r.stderr
    r = _memo("-g", str(tmp_path / "nothere.txt"), "-p", "test", "-o", str(tmp_path))
    assert r.returncode != 0 and b"cannot read the genome list" in r.stderr
    lone = tmp_path / "one.txt"
    lone.write_text(os.path.join(ROOT, "tests", "golden", "example_fa", "ref_1.fa") + "\n")
    r = _memo("-g", str(lone), "-p", "test", "-o", str(tmp_path))
    assert r.returncode != 0 and b"at least one more genome" in r.stderr
    assert not (tmp_path / "test.parquet").exists()


def test_bad_pivot_is_refused_before_the_device(tmp_path):
    """a pivot with an empty record, a gzip file, a NUL byte: a message and exit 1, no index"""
    ok = tmp_path / "ok.fa"
    ok.write_bytes(b">a\nACGT\n")
    for name, data, what in (("empty.fa", b">a\nACGT\n>b\n\n>c\nGG\n", b"length 0"),
                             ("gz.fa", b"\x1f\x8b\x08\x00rest", b"gzip"),
                             ("nul.fa", b">a\nAC\0GT\n", b"NUL")):
        bad = tmp_path / name
        bad.write_bytes(data)
        lst = tmp_path / (name + ".txt")
        lst.write_text(f"{bad}\n{ok}\n")
        r = _memo("-g", str(lst), "-p", "idx", "-o", str(tmp_path))
        assert r.returncode == 1 and what in r.stderr, (name, r.stderr)
        assert not (tmp_path / "idx.parquet").exists()


def test_view_is_still_refused():
    r = subprocess.run([sys.executable, EXE, "view"], capture_output=True, timeout=60)
    assert r.returncode == 1 and b"not part of the MI355X query build" in r.stderr


# ---- FASTA parsing --------------------------------------------------------------------------------------

def test_fasta_records_names_and_sequence_lines():
    from memo_amd.build_index import parse_fasta
    data = (b">chr1 a description\r\nACgt\r\nnnAC \r\n\r\n"
            b">chr2\tmore words\nac\n gt\n"
            b">empty\n"
            b">chr3\nRYKMbvdh\n")
    assert parse_fasta(data) == [("chr1", b"ACGTNNAC"), ("chr2", b"ACGT"), ("empty", b""), ("chr3", b"RYKMBVDH")]
    assert parse_fasta(b"\n\n>x\nA\nC") == [("x", b"AC")]             # leading blank lines, no final newline
    assert parse_fasta(b"") == []


@pytest.mark.parametrize("data,what", [(b"\x1f\x8b\x08\x00\x00", "gzip"), (b">a\nAC\x00G\n", "NUL"),
                                       (b"ACGT\n>a\nAC\n", "not FASTA")])
def test_fasta_refusals(data, what):
    from memo_amd.build_index import FastaError, parse_fasta
    with pytest.raises(FastaError, match=what):
        parse_fasta(data)


def test_pivot_layout_offsets_and_refusals():
    from memo_amd.build_index import FastaError, pivot_layout
    names, seq, rb = pivot_layout([("a", b"ACG"), ("b", b"T"), ("c", b"GGGG")])
    assert names == ["a", "b", "c"] and seq == b"ACGTGGGG" and rb.tolist() == [0, 3, 4, 8]
    with pytest.raises(FastaError, match="length 0"):
        pivot_layout([("a", b"ACG"), ("b", b"")])
    with pytest.raises(FastaError, match="no records"):
        pivot_layout([])


# ---- the genome text --------------------------------------------------------------------------------------

_PAIRS = {"A": "T", "C": "G", "R": "Y", "K": "M", "B": "V", "D": "H"}
_COMP = {**_PAIRS, **{v: k for k, v in _PAIRS.items()}}


def _text_rule(records):
    """S_1 $ ... S_s $ rc(S_1) $ ... rc(S_s) $, rc as samtools faidx -i (IUPAC pairs swap, the rest stays)"""
    rc = ["".join(_COMP.get(ch, ch) for ch in reversed(s)) for s in records]
    return "".join(s + "\0" for s in records + rc).encode("latin-1") if records else b""


def test_genome_text_matches_the_rule():
    import numpy as np
    from memo_amd.build_index import genome_text, revcomp
    assert revcomp(b"ACGTRYKMBVDHNSW*") == b"*WSNDHBVKMRYACGT"
    rng = np.random.default_rng(5)
    alphabet = list("ACGTNRYKMBVDHSW")
    for trial in range(50):
        recs = ["".join(rng.choice(alphabet, int(rng.integers(0, 40)))) for _ in range(int(rng.integers(0, 5)))]
        assert genome_text([r.encode() for r in recs]) == _text_rule(recs), recs
    assert genome_text([b"AC", b"", b"G"]) == b"AC\0\0G\0GT\0\0C\0"
