"""`memo view` on the GPU: the device reader of conservation text (memo_parse_conservation_text_dev), the table straight from an
index (view.preprocess_region) and the command line end to end.

The expected vector is always the reference's own reading of the same file (plot_conservation.py:40-49), written here and never
produced by the code under test; what a uint16 vector cannot hold (negatives, 65535 and more) is 65535, which no column of the
table counts and every bin's width does."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import golden_util as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "memo")
TILE = 16384


@pytest.fixture(scope="module")
def memo():
    import memo_amd
    from memo_amd import _lib
    memo_amd.build()                     # make: a no-op when libmemo_amd.so is up to date
    assert _lib.lib().memo_device_count() > 0, "no HIP device: the product has no CPU fallback"
    return memo_amd


def reference_reading(path):
    values = [int(line.strip()) for line in open(path)]
    return np.array([v if 0 <= v < 65535 else 65535 for v in values], np.uint16)


def parse_on_device(data, cap=None):
    """(vector, lines, first_odd_offset) of memo_parse_conservation_text_dev on these bytes"""
    from memo_amd._lib import check, lib
    n = len(data)
    cap = n // 2 + 1 if cap is None else cap
    d_text, d_vec = C.c_void_p(), C.c_void_p()
    check(lib().memo_dev_malloc(0, n, C.byref(d_text)))
    check(lib().memo_dev_malloc(0, 2 * cap, C.byref(d_vec)))
    try:
        host = np.frombuffer(data, np.uint8)
        check(lib().memo_dev_upload(0, d_text, host.ctypes.data if n else None, n, None))
        lines, odd = C.c_int64(-7), C.c_int64(-7)
        check(lib().memo_parse_conservation_text_dev(d_text, n, d_vec, cap, C.byref(lines), C.byref(odd), 0, None))
        vec = np.empty(lines.value, np.uint16)
        check(lib().memo_dev_download(0, vec.ctypes.data, d_vec, vec.nbytes, None))
    finally:
        lib().memo_dev_free(0, d_text)
        lib().memo_dev_free(0, d_vec)
    return vec, lines.value, odd.value


@pytest.fixture(scope="module")
def random_values():
    return np.random.default_rng(20).integers(0, 70000, 50_001)         # 1 - 5 digits; some of 65535 and more


def _dressed(values):
    """leading and trailing blanks and tabs, zero padding: at most 3 + 3 + 5 + 3 bytes a line"""
    rng = np.random.default_rng(21)
    blanks = ["", " ", "\t", "  ", " \t", "\t  "]
    lines = ["  007\t\n"]
    for v, a, z, b in zip(values[1:], rng.integers(0, 6, len(values)), rng.integers(0, 4, len(values)), rng.integers(0, 6, len(values))):
        lines.append(f"{blanks[a]}{'0' * z}{v}{blanks[b]}\n")
    return "".join(lines)


@pytest.mark.parametrize("form", ["plain", "no_final_newline", "crlf", "blanks_and_zero_padding"])
def test_reader_random_text(memo, random_values, form, tmp_path):
    text = "".join(f"{v}\n" for v in random_values)
    if form == "no_final_newline":
        text = text[:-1]
    elif form == "crlf":
        text = text.replace("\n", "\r\n")
    elif form == "blanks_and_zero_padding":
        text = _dressed(random_values)
    data = text.encode()
    assert len(data) > 3 * TILE and len(data) % TILE and len(data) % 16          # several tiles, a ragged tail
    starts = np.flatnonzero(np.frombuffer(b"\n" + data[:-1], np.uint8) == 10)    # a line starts behind every \n
    assert set((starts % 16).tolist()) == set(range(16))                         # ... on every one of the 16 byte lanes
    path = tmp_path / "c.txt"
    path.write_bytes(data)
    want = reference_reading(str(path))
    assert len(want) == 50_001 and (want == 65535).sum() > 1000 and want.max() == 65535
    vec, lines, odd = parse_on_device(data)
    assert (lines, odd) == (50_001, -1)
    assert np.array_equal(vec, want)


@pytest.mark.parametrize("data", [b"7\n", b"7", b"65534\r\n", b" 12 "])
def test_reader_one_line(memo, data, tmp_path):
    path = tmp_path / "c.txt"
    path.write_bytes(data)
    vec, lines, odd = parse_on_device(data)
    assert (lines, odd) == (1, -1) and np.array_equal(vec, reference_reading(str(path)))


def test_reader_line_of_exactly_the_longest_form(memo, tmp_path):
    """32 bytes and nine digits are inside the grammar, at a tile's edge too: the line ends on the first byte of the second tile"""
    head = "1\n" * ((TILE - 32) // 2)
    text = head + " " * 20 + "123456789" + "\t" * 3 + "\n" + "0" * 30 + "42\n" + "3"
    data = text.encode()
    assert data[TILE] == 10
    path = tmp_path / "c.txt"
    path.write_bytes(data)
    vec, lines, odd = parse_on_device(data)
    assert odd == len(data) - 2                          # the 32 digits of the line before the last: ten or more, at its \n
    data = data.replace(b"0" * 30 + b"42", b" " * 30 + b"42")
    path.write_bytes(data)
    vec, lines, odd = parse_on_device(data)
    assert odd == -1 and lines == len(vec) == (TILE - 32) // 2 + 3
    assert np.array_equal(vec, reference_reading(str(path))) and vec[-3:].tolist() == [65535, 42, 3]


def test_reader_empty_file(memo, tmp_path):
    from memo_amd import view
    vec, lines, odd = parse_on_device(b"")
    assert (lines, odd, len(vec)) == (0, -1, 0)
    path = tmp_path / "empty.txt"
    path.write_bytes(b"")
    d_vec, L, free = view.read_conservation_text_dev(str(path))
    free()
    assert L == 0
    with pytest.raises(ZeroDivisionError):
        view.preprocess_data(str(path), 5, 4)


def test_reader_refuses_a_vector_that_is_too_short(memo):
    from memo_amd import MemoError
    with pytest.raises(MemoError, match="3 lines"):
        parse_on_device(b"1\n2\n3\n", cap=2)


# what is odd, and at which byte of it the header says so (offsets from the oddity's first byte)
ODDITIES = [("blank_line", b"\n", 0), ("line_of_blanks", b" \t \n", 3), ("lone_cr", b"5\r6\n", 1), ("sign", b"+1\n", 0),
            ("underscore", b"1_0\n", 1), ("ten_digits", b"1234567890\n", 10), ("forty_bytes", b" " * 39 + b"5\n", 40),
            ("blank_inside", b"1 2\n", 3), ("nul", b"4\x00\n", 1)]


@pytest.mark.parametrize("name,oddity,at", ODDITIES, ids=[o[0] for o in ODDITIES])
def test_reader_reports_the_first_odd_byte(memo, name, oddity, at):
    head = b"12345\n" * 20_000                           # seven whole tiles and a third
    for tail in (b"8\n9\n", b""):
        data = head + oddity + tail
        assert len(head) // TILE == (len(data) - 1) // TILE == 7         # the oddity sits in the last tile, and nowhere else
        vec, lines, odd = parse_on_device(data)
        assert odd == len(head) + at, (name, tail)
    # of two, the first; a \r that ends the text; a last line that no \n ends reports the end of the text
    assert parse_on_device(b"5\n\n" + head + oddity)[2] == 2
    assert parse_on_device(head + b"5\r")[2] == len(head) + 1
    assert parse_on_device(head + b"1 2")[2] == len(head) + 3


@pytest.mark.parametrize("name,oddity,at", ODDITIES, ids=[o[0] for o in ODDITIES])
def test_odd_texts_give_what_the_reference_gives(memo, oracle, name, oddity, at, tmp_path):
    from memo_amd import view
    rng = np.random.default_rng(22)
    data = "".join(f"{v}\n" for v in rng.integers(0, 10, 300)).encode() + oddity + b"3\n4\n"
    path = tmp_path / "c.txt"
    path.write_bytes(data)
    try:
        want = oracle.view_table(reference_reading(str(path)), 9, 7)
    except ValueError:
        with pytest.raises(ValueError):
            view.preprocess_data(str(path), 9, 7)
        assert name in ("blank_line", "line_of_blanks", "blank_inside", "nul")
        return
    got = view.preprocess_data(str(path), 9, 7)
    for key in want:
        assert np.array_equal(got[key], want[key]), key


def test_reader_conservation_goldens(memo):
    with_out = [c for c in G.cases(membership=False, raises=False) if "out" in c]
    empty = [c for c in with_out if G.load(c)["vec"].size == 0]          # an empty window's file is a lone \n
    assert len(with_out) - len(empty) > 50 and empty
    for c in with_out:
        path = os.path.join(G.GOLD, c["out"])
        vec, lines, odd = parse_on_device(open(path, "rb").read())
        if c in empty:                                   # a blank line: odd at byte 0, and the reference's reader refuses it too
            assert (lines, odd) == (1, 0), c["name"]
            with pytest.raises(ValueError):
                reference_reading(path)
            continue
        want = reference_reading(path)
        assert (lines, odd) == (len(want), -1), c["name"]
        assert np.array_equal(vec, want) and np.array_equal(vec, G.load(c)["vec"]), c["name"]


def test_view_goldens_from_text(memo, tmp_path):
    from memo_amd import view
    for c in json.load(open(os.path.join(G.GOLD, "view", "manifest.json"))):
        z = np.load(os.path.join(G.GOLD, "view", c["name"] + ".npz"))
        path = tmp_path / (c["name"] + ".txt")
        path.write_bytes(memo.emit_conservation(z["vec"]))
        if "raises" in c:
            assert c["name"] == "view4"
            with pytest.raises(ZeroDivisionError):
                view.preprocess_data(str(path), c["n_docs"], c["n_bins"])
            continue
        got = view.preprocess_data(str(path), c["n_docs"], c["n_bins"])
        assert np.array_equal(got["bin"], z["bin"]) and np.array_equal(got["No. Genomes"], z["genomes"])
        assert got["value"].tobytes() == z["value"].tobytes()              # float64, bit for bit


REGION_CASES = ["ex_cons_k3_0_20", "rnd_n40_cons_k31_c0w0", "rnd_n40_cons_k3_c1w1", "rnd_n130_cons_k31_c0w0", "rnd_n130_cons_k5_c0w1"]


@pytest.mark.parametrize("name", REGION_CASES)
def test_table_straight_from_an_index(memo, oracle, name):
    from memo_amd import view
    c = next(x for x in G.cases() if x["name"] == name)
    vec = G.load(c)["vec"]
    index = os.path.join(G.GOLD, c["index"])
    for n_bins in ([4] if name.startswith("ex_") else []) + [1, 7, len(vec)]:
        got = view.preprocess_region(index, c["region"], c["k"], c["n"], n_bins)
        want = oracle.view_table(vec, c["n"], n_bins)
        for key in want:
            assert got[key].dtype == want[key].dtype and got[key].tobytes() == want[key].tobytes(), (n_bins, key)
    with pytest.raises(ZeroDivisionError):
        view.preprocess_region(index, c["region"], c["k"], c["n"], len(vec) + 1)
    with pytest.raises(ValueError):                      # a reversed window: as `memo query` raises it
        rec, qs, qe = G.region(c)
        view.preprocess_region(index, f"{rec}:{qe}-{qs}", c["k"], c["n"], 4)


def _memo(*argv):
    return subprocess.run([sys.executable, EXE, *argv], capture_output=True, timeout=300)


def test_cli_text_route_and_index_route_write_the_same_table(memo, oracle, tmp_path):
    index = os.path.join(G.GOLD, "example_cons.parquet")
    out, t, u = (str(tmp_path / f) for f in ("out.txt", "t.tsv", "u.tsv"))
    assert _memo("query", "-b", index, "-r", "ref_1:0-20", "-k", "3", "-n", "5", "-o", out).returncode == 0
    r = _memo("view", "-i", out, "-o", t, "-n", "5", "-b", "4")
    assert r.returncode == 0 and r.stdout == b"MEMO - plotting sequence conservation\n", r.stderr
    r = _memo("view", "-i", index, "-r", "ref_1:0-20", "-k", "3", "-n", "5", "-b", "4", "-o", u)
    assert r.returncode == 0 and r.stdout == b"MEMO - plotting sequence conservation\n", r.stderr
    assert open(t, "rb").read() == open(u, "rb").read()
    from tests.test_view_cli import read_tsv
    want = oracle.view_table(reference_reading(out), 5, 4)
    assert read_tsv(t)["value"].tobytes() == want["value"].tobytes()


def test_cli_plot_and_errors(memo, tmp_path):
    vec = np.array([5, 5, 3, 4, 5, 2, 1, 2, 5, 5, 4, 4], np.uint16)
    text, png, tsv = (str(tmp_path / f) for f in ("c.txt", "p.png", "t.tsv"))
    open(text, "wb").write(memo.emit_conservation(vec))
    r = _memo("view", "-i", text, "-o", png, "-n", "5", "-b", "3", "-d", "50")
    try:
        import matplotlib  # noqa: F401
    except ImportError:
        assert r.returncode == 1 and b".tsv" in r.stderr and not os.path.exists(png)
    else:
        assert r.returncode == 0, r.stderr
        assert open(png, "rb").read(8) == b"\x89PNG\r\n\x1a\n"
    r = _memo("view", "-i", text, "-o", tsv, "-n", "5", "-b", "13")       # more bins than positions
    assert r.returncode == 1 and b"division by zero" in r.stderr and not os.path.exists(tsv)
    open(text, "ab").write(b"x\n")
    r = _memo("view", "-i", text, "-o", tsv, "-n", "5", "-b", "3")        # int('x')
    assert r.returncode == 1 and b"invalid literal" in r.stderr and not os.path.exists(tsv)
    assert sorted(os.listdir(tmp_path)) in (["c.txt"], ["c.txt", "p.png"])   # nothing half written either
