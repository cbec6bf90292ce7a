"""`memo view` without a GPU: the command line (src/view.sh's usage bytes, getopts handling), the table's TSV form, the
matplotlib renderer and the host reader that takes the texts the device reader hands back."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "memo")
USAGE = open(os.path.join(ROOT, "tests", "golden", "cli", "memo_view_usage.txt"), "rb").read()


def _memo(*argv):
    return subprocess.run([sys.executable, EXE, "view", *argv], capture_output=True, timeout=120)


def test_usage_bytes_then_the_extension():
    r = _memo("-h")
    assert r.returncode == 0
    assert r.stdout.startswith(USAGE)
    assert b"-r [CHR:START-END]" in r.stdout[len(USAGE):] and b".tsv" in r.stdout[len(USAGE):]
    assert r.stderr == b""


def test_illegal_option_prints_getopts_message_then_usage():
    r = _memo("-x")
    assert r.returncode == 0
    assert r.stdout.startswith(USAGE)
    assert r.stderr.endswith(b": illegal option -- x\n")
    r = _memo("-n", "5", "-i")
    assert r.returncode == 0 and r.stdout.startswith(USAGE)
    assert r.stderr.endswith(b": option requires an argument -- i\n")


def read_tsv(path):
    """what view_cli.write_tsv wrote, as the same dict of arrays"""
    from memo_amd import view_cli
    with open(path) as fh:
        assert fh.readline() == view_cli.TSV_HEADER
        rows = [line.rstrip("\n").split("\t") for line in fh]
    return {"bin": np.array([int(r[0]) for r in rows], np.int64),
            "No. Genomes": np.array([float(r[1]) for r in rows], np.float64),
            "value": np.array([float(r[2]) for r in rows], np.float64)}


def test_tsv_round_trips_float_bits(oracle, tmp_path):
    from memo_amd import view_cli
    rng = np.random.default_rng(11)
    vec = rng.integers(0, 8, 1000)                      # bins of 142 and 143 positions: quotients that need all 17 digits
    table = oracle.view_table(vec, 7, 7)
    path = tmp_path / "t.tsv"
    view_cli.write_tsv(table, str(path))
    lines = path.read_text().split("\n")
    assert lines[0] == "bin\tNo. Genomes\tvalue" and lines[-1] == "" and len(lines) == 7 * 7 + 2
    assert lines[1].split("\t")[:2] == ["0", "0.0"] and lines[8].split("\t")[:2] == ["0", "1.0"]     # melt order: bins innermost
    back = read_tsv(str(path))
    for key in ("bin", "No. Genomes", "value"):
        assert back[key].dtype == table[key].dtype
        assert back[key].tobytes() == table[key].tobytes(), key
    assert not [f for f in os.listdir(tmp_path) if f != "t.tsv"]            # (written beside and renamed: nothing stays)


def test_renderer_writes_a_png_of_the_figure_size(oracle, tmp_path):
    pytest.importorskip("matplotlib")
    from memo_amd import view_cli
    vec = np.array([5, 5, 3, 4, 5, 2, 1, 2, 5, 5, 4, 4, 0, 5, 5, 1, 2, 3, 5, 5])
    table = oracle.view_table(vec, 5, 4)
    path = tmp_path / "plot.png"
    view_cli.render(table, 5, 4, str(path), dpi=50)
    data = path.read_bytes()
    assert data[:8] == b"\x89PNG\r\n\x1a\n" and data[12:16] == b"IHDR"
    assert struct.unpack(">II", data[16:24]) == (20 * 50, 4 * 50)
    assert os.listdir(tmp_path) == ["plot.png"]
    colours = view_cli.fill_colours(5)                   # the scale's limits are 1 .. n_docs - 1
    assert np.allclose(colours[1], (0, 0, 0)) and np.allclose(colours[4], (0xc6 / 255, 0xdb / 255, 0xef / 255))


def _reference_reading(path):
    """plot_conservation.py:40-49, and what a uint16 vector makes of it: outside [0, 65534] -> 65535"""
    values = [int(line.strip()) for line in open(path)]
    return [v if 0 <= v < 65535 else 65535 for v in values]


@pytest.mark.parametrize("text", ["+3\n", "1_0\n", "-2\n", "70000\n", "5\n+3\n1_0\n-2\n70000\n 7 \r\n65534\n65535", "4\r5\n"])
def test_fallback_reader_reads_what_the_reference_reads(text, tmp_path):
    from memo_amd import view
    path = tmp_path / "c.txt"
    path.write_bytes(text.encode())
    got = view._read_text_reference(str(path))
    assert got.dtype == np.uint16 and got.tolist() == _reference_reading(str(path))


def test_reference_reading_of_the_tests_is_not_vacuous(tmp_path):
    """what the expectation above is made of: a sign and an underscore are read, a negative and 70000 become 65535"""
    path = tmp_path / "c.txt"
    path.write_text("+3\n1_0\n-2\n70000\n")
    assert _reference_reading(str(path)) == [3, 10, 65535, 65535]


@pytest.mark.parametrize("text", ["5\n\n6\n", "5\n  \n", "5\nx\n", "\n"])
def test_fallback_reader_raises_value_error(text, tmp_path):
    from memo_amd import view
    path = tmp_path / "c.txt"
    path.write_text(text)
    with pytest.raises(ValueError):
        view._read_text_reference(str(path))
