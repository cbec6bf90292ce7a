"""The piece plan of `memo index` without a GPU: a genome's text S_1 $ ... S_s $ rc(S_1) $ ... rc(S_s) $ is cut into pieces of
whole strings (memo_ms_plan_pieces, the plan memo_ms_add_records follows), and the piece cap that MEMO_INDEX_PIECE_BYTES sets
is checked before the device is touched."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import golden_util as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "memo")
MAX_PIECE = (1 << 31) - 2


@pytest.fixture(scope="module")
def bi():
    from memo_amd import _lib, build_index
    _lib.lib()
    return build_index


def _greedy(lengths, cap):
    """the rule, restated: strings in order S_1 .. S_s, rc(S_1) .. rc(S_s), len + 1 bytes each; a piece takes strings
    while it stays at or under the cap"""
    costs = [n + 1 for n in lengths] * 2
    piece, p, used = [], 0, 0
    for c in costs:
        if used + c > cap:
            p, used = p + 1, 0
        used += c
        piece.append(p)
    return (p + 1 if costs else 0), piece


def test_order_and_greedy_rule_count_the_separator(bi):
    pieces, piece = bi.plan_pieces([3, 4, 5], 9)          # strings of 4 5 6 4 5 6 bytes
    assert (pieces, piece.tolist()) == (4, [0, 0, 1, 2, 2, 3])
    pieces, piece = bi.plan_pieces([3, 4, 5], 8)          # 4 + 5 > 8: the separators count
    assert (pieces, piece.tolist()) == (6, [0, 1, 2, 3, 4, 5])
    pieces, piece = bi.plan_pieces([2, 2], 6)             # S_1 and S_2 fill the first piece exactly
    assert (pieces, piece.tolist()) == (2, [0, 0, 1, 1])
    pieces, piece = bi.plan_pieces([1, 1, 1], 4)
    assert (pieces, piece.tolist()) == (3, [0, 0, 1, 1, 2, 2])


def test_one_piece_exactly_when_the_text_fits(bi):
    lengths = [5, 0, 17, 2]
    text = 2 * sum(n + 1 for n in lengths)
    pieces, piece = bi.plan_pieces(lengths, text)
    assert pieces == 1 and not piece.any()
    pieces, piece = bi.plan_pieces(lengths, text - 1)    # one byte over: the last string opens a second piece
    assert pieces == 2 and piece.tolist() == [0] * 7 + [1]
    pieces, _ = bi.plan_pieces(lengths, MAX_PIECE)
    assert pieces == 1


def test_a_string_at_cap_minus_one_fits_one_at_cap_is_refused(bi):
    from memo_amd._lib import MemoError
    pieces, piece = bi.plan_pieces([9, 3], 10)
    assert pieces == 4 and piece.tolist() == [0, 1, 2, 3]
    with pytest.raises(MemoError, match=r"genome record 1 of 10 bases needs 11 bytes .* piece cap of 10"):
        bi.plan_pieces([3, 10], 10)
    with pytest.raises(MemoError, match="piece cap of 2147483646"):
        bi.plan_pieces([MAX_PIECE], MAX_PIECE)
    assert bi.plan_pieces([MAX_PIECE - 1], MAX_PIECE)[0] == 2


def test_empty_records_no_records_and_cap_bounds(bi):
    from memo_amd._lib import MemoError
    assert bi.plan_pieces([], 2)[0] == 0
    assert bi.plan_pieces([], MAX_PIECE)[0] == 0
    pieces, piece = bi.plan_pieces([0, 0, 0], 2)          # an empty record is its separator alone
    assert pieces == 3 and piece.tolist() == [0, 0, 1, 1, 2, 2]
    pieces, piece = bi.plan_pieces([0, 1, 0], 3)
    assert (pieces, piece.tolist()) == _greedy([0, 1, 0], 3)
    for cap in (1, 0, -5, MAX_PIECE + 1, 1 << 40):
        with pytest.raises(MemoError, match=r"piece cap .* outside \[2, 2\^31 - 2\]"):
            bi.plan_pieces([1], cap)
    with pytest.raises(MemoError, match="has length -1"):
        bi.plan_pieces([4, -1], 100)


def test_plan_matches_the_rule_on_random_lengths(bi):
    rng = np.random.default_rng(7)
    for _ in range(200):
        lengths = rng.integers(0, 50, int(rng.integers(0, 40))).tolist()
        cap = int(rng.integers(max(lengths, default=0) + 1, 400))
        cap = max(cap, 2)
        pieces, piece = bi.plan_pieces(lengths, cap)
        want_pieces, want_piece = _greedy(lengths, cap)
        assert pieces == want_pieces and piece.tolist() == want_piece, (lengths, cap)
        costs = np.array([n + 1 for n in lengths] * 2, np.int64)
        if len(costs):
            assert np.bincount(piece, weights=costs).max() <= cap


def test_piece_bytes_from_env(bi):
    assert bi.piece_bytes_from_env({}) == 0
    assert bi.piece_bytes_from_env({"MEMO_INDEX_PIECE_BYTES": ""}) == 0
    assert bi.piece_bytes_from_env({"MEMO_INDEX_PIECE_BYTES": "2"}) == 2
    assert bi.piece_bytes_from_env({"MEMO_INDEX_PIECE_BYTES": str(MAX_PIECE)}) == MAX_PIECE
    for bad in ("1", "0", "-3", "abc", "1e9", str(MAX_PIECE + 1), " "):
        with pytest.raises(bi.FastaError, match="MEMO_INDEX_PIECE_BYTES"):
            bi.piece_bytes_from_env({"MEMO_INDEX_PIECE_BYTES": bad})


@pytest.mark.parametrize("bad", ["0", "1", "-1", "12k", "0x40", str(MAX_PIECE + 1)])
def test_bad_piece_cap_refused_by_memo_index(tmp_path, bad):
    example = [os.path.join(G.GOLD, "example_fa", f"ref_{i}.fa") for i in range(1, 6)]
    lst = tmp_path / "genome_list.txt"
    lst.write_text("".join(p + "\n" for p in example))
    env = dict(os.environ, MEMO_INDEX_PIECE_BYTES=bad)
    r = subprocess.run([sys.executable, EXE, "index", "-g", str(lst), "-o", str(tmp_path / "w"), "-p", "test"],
                       capture_output=True, timeout=120, env=env)
    assert r.returncode == 1, r
    assert b"MEMO_INDEX_PIECE_BYTES" in r.stderr and r.stderr.startswith(b"memo index: "), r.stderr
    assert r.stdout == b""
    assert not (tmp_path / "w" / "test.parquet").exists()
