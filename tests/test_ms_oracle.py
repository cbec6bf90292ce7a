"""The CPU references of `memo index` (oracle/ms_oracle.py) against definitions that share nothing with them: the
suffix-automaton matching statistics (MS) against brute-force substring search and against tools/ms_sam.cpp, and the
Burkhardt-Kaerkkaeinen suffix-array checker against sorted() and against suffix arrays broken on purpose.  No GPU:
tests/test_ms_gpu.py trusts these references, so they answer to this file first."""
import os
import subprocess

import numpy as np
import pytest

from oracle import ms_oracle as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rand_case(rng):
    """a NUL-separated genome text over bytes 1..255 (from a small or a full alphabet) and pivot records, some
    empty, some one byte long, some copied from the text so that their matches would run on into the next record"""
    sigma = int(rng.choice([1, 2, 4, 20, 255]))
    alpha = rng.choice(np.arange(1, 256), sigma, replace=False).astype(np.uint8)
    draw = lambda n: alpha[rng.integers(0, sigma, n)].tobytes()  # noqa: E731
    recs = [draw(int(rng.integers(0, 40))) for _ in range(int(rng.integers(1, 5)))]
    text = b"\0".join(recs) + b"\0" if rng.random() < 0.8 else draw(int(rng.integers(0, 80)))
    piv = []
    for _ in range(int(rng.integers(1, 6))):
        kind = rng.integers(4)
        if kind == 0 and len(text) > 2:                 # a piece of the text, cut where the text goes on
            a = int(rng.integers(0, len(text) - 1))
            piece = text[a:a + int(rng.integers(1, 30))].replace(b"\0", b"")
            piv.append(piece)
        elif kind == 1:
            piv.append(draw(1))
        elif kind == 2:
            piv.append(b"")
        else:
            piv.append(draw(int(rng.integers(1, 50))))
    return text, piv


@pytest.mark.parametrize("seed", range(10))
def test_ms_oracle_equals_brute_force(seed):
    rng = np.random.default_rng(1000 + seed)
    for _ in range(20):
        text, piv = _rand_case(rng)
        got, want = M.ms_records(piv, text), M.brute_ms(piv, text)
        assert np.array_equal(got, want), (text, piv, got, want)


def test_ms_oracle_edges():
    assert M.ms_records([b"ACGT"], b"").tolist() == [0, 0, 0, 0]
    assert M.ms_records([b"AC", b"GT"], b"ACGT\0").tolist() == [2, 1, 2, 1]      # stops at the record end
    assert M.ms_records([b"\xff\x01", b"\x80"], b"\x01\xff\x01\0\x80").tolist() == [2, 1, 1]
    assert M.ms_records([b"A" * 10], b"A" * 4).tolist() == [4] * 7 + [3, 2, 1]
    assert M.ms_records([b"N" * 5], b"NN\0NNN\0").tolist() == [3, 3, 3, 2, 1]    # never across a separator
    with pytest.raises(ValueError):
        M.ms(b"AC", b"ACG", np.array([0, 2]))


def test_ms_oracle_equals_ms_sam(tmp_path):
    """tools/ms_sam.cpp (ACGT codes, a fixed 5-way automaton) on a multi-record pivot against mutated genomes"""
    exe = str(tmp_path / "ms_sam")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", os.path.join(ROOT, "tools", "ms_sam.cpp"), "-o", exe])
    rng = np.random.default_rng(44)
    letters = np.frombuffer(b"ACGT", np.uint8)
    recs = [rng.integers(0, 4, n).astype(np.uint8) for n in (40_000, 1, 3_000, 17)]
    recs[2][1000:2000] = 2                                       # a homopolymer run
    pivot_bin = np.concatenate([np.append(r, 4) for r in recs])[:-1].astype(np.uint8)
    pivot_bin.tofile(tmp_path / "pivot.bin")
    texts, paths = [], []
    for g in range(3):
        seqs = []
        for r in recs:
            s = r.copy()
            hit = rng.random(len(s)) < 0.01 * g
            s[hit] = (s[hit] + 1) & 3
            seqs.append(s)
        seqs.append(rng.integers(0, 4, 500).astype(np.uint8))
        rc = [3 - s[::-1] for s in seqs]
        body = np.concatenate([np.append(s, 4) for s in seqs + rc]).astype(np.uint8)
        body.tofile(tmp_path / f"g{g}.bin")
        paths.append(str(tmp_path / f"g{g}.bin"))
        texts.append(np.where(body == 4, 0, letters[np.minimum(body, 3)]).astype(np.uint8).tobytes())
    subprocess.run([exe, str(tmp_path / "pivot.bin"), str(tmp_path / "dap.i32")] + paths, check=True, timeout=300,
                   capture_output=True, env=dict(os.environ, MS_THREADS="2"))
    want = np.fromfile(tmp_path / "dap.i32", np.int32).reshape(len(pivot_bin), 3)[pivot_bin != 4]
    for g in range(3):
        got = M.ms_records([letters[r].tobytes() for r in recs], texts[g])
        assert np.array_equal(got, want[:, g]), (g, np.flatnonzero(got != want[:, g])[:5])


# ---- the suffix-array checker -----------------------------------------------------------------------------------

def _sa_texts():
    rng = np.random.default_rng(8)
    yield b"A"
    yield b"banana"
    yield b"A" * 300
    yield b"AB" * 150 + b"A"
    yield bytes(rng.integers(0, 256, 2000).astype(np.uint8))
    yield bytes(rng.choice(list(b"AC\0"), 1500).astype(np.uint8))
    yield bytes(rng.choice([0, 1, 255], 1200).astype(np.uint8))


def _sorted_sa(text):
    return np.array(sorted(range(len(text)), key=lambda i: text[i:]), np.int32)


@pytest.mark.parametrize("i", range(7))
def test_sa_checker_accepts_sorted(i):
    text = list(_sa_texts())[i]
    assert M.check_sa(text, _sorted_sa(text)) is None
    assert M.check_sa(text, _sorted_sa(text), block=7) is None                # the block seams


def test_sa_checker_accepts_empty():
    assert M.check_sa(b"", np.zeros(0, np.int32)) is None


@pytest.mark.parametrize("i", range(7))
def test_sa_checker_rejects_broken(i):
    text = list(_sa_texts())[i]
    sa = _sorted_sa(text)
    n = len(text)
    rng = np.random.default_rng(i)
    broken = []
    if n > 1:
        for x in sorted({1, n - 1, int(rng.integers(1, n))}):               # adjacent swaps
            b = sa.copy()
            b[x - 1], b[x] = b[x], b[x - 1]
            broken.append(("adjacent swap", b))
        x, y = rng.choice(n, 2, replace=False)
        b = sa.copy()
        b[x], b[y] = b[y], b[x]
        broken.append(("random swap", b))
        b = sa.copy()
        b[int(rng.integers(1, n))] = b[0]
        broken.append(("duplicate", b))
        rev = _sorted_sa(text[::-1])
        if not np.array_equal(rev, sa):
            broken.append(("SA of the reversed text", rev))
    broken.append(("too short", sa[:-1]))
    b = sa.copy()
    b[-1] = n
    broken.append(("out of range", b))
    for what, b in broken:
        assert M.check_sa(text, b) is not None, what
        assert M.check_sa(text, b, block=5) is not None, what
