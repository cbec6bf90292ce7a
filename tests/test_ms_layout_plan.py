"""The DAP layout of `memo index` without a GPU: which of the two layouts a pivot gets (memo_ms_plan_layout, the decision
memo_ms_create_layout takes with the device's free memory), what the coded layout needs at the least, and the layout that
MEMO_INDEX_DAP_LAYOUT asks for, checked before the device is touched."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import golden_util as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "memo")
HBM = int(288e9)
BLOCK = 2048                                   # positions per coding block (memo_ms_layout_info reports it on the device)
WORKING_SET = (1 << 20) * 56 + (1 << 18) + (64 << 20)   # of a 1 MiB text: what memo_ms_create has always added


@pytest.fixture(scope="module")
def bi():
    from memo_amd import _lib, build_index
    _lib.lib()
    return build_index


def _dense_need(positions, columns):
    return positions * columns * 4 + positions + WORKING_SET


def _coded_floor(positions, columns):
    """the header's rule: scratch column + pivot (and its 64 bytes of padding) + every column's flag words and block offsets
    with no value yet + the same working set"""
    nblocks = -(-positions // BLOCK)
    return positions * 4 + positions + 64 + columns * (8 * (BLOCK // 64) * nblocks + 8 * nblocks) + WORKING_SET


def test_the_issue_shapes(bi):
    from memo_amd._lib import MEMO_EINVAL, MemoError
    assert bi.plan_layout(20_000_000, 15, HBM) == ("dense", _dense_need(20_000_000, 15))
    layout, floor = bi.plan_layout(3_100_000_000, 46, HBM)
    assert layout == "coded" and floor == _coded_floor(3_100_000_000, 46)
    # 12.4 GB scratch + 3.1 GB pivot + 17.8 GB flags + 0.6 GB offsets + 0.1 GB working set
    assert 33e9 < floor < 60e9
    with pytest.raises(MemoError, match="device memory") as exc:
        bi.plan_layout((1 << 30) - 1, 4096, HBM)
    assert exc.value.code == MEMO_EINVAL
    with pytest.raises(MemoError, match="the DAP matrix needs .* of device memory"):
        bi.plan_layout(3_100_000_000, 46, HBM, "dense")
    assert bi.plan_layout(1000, 3, HBM, "coded") == ("coded", _coded_floor(1000, 3))
    assert bi.plan_layout(1000, 3, HBM, "dense") == ("dense", _dense_need(1000, 3))
    assert bi.plan_layout(1000, 3, HBM, "auto")[0] == "dense"
    with pytest.raises(MemoError, match="device memory"):
        bi.plan_layout(1 << 33, 64, 1 << 30, "coded")
    for bad in (3, -1, 99):
        with pytest.raises(MemoError, match="layout") as exc:
            bi.plan_layout(1000, 3, HBM, bad)
        assert exc.value.code == MEMO_EINVAL
    with pytest.raises(ValueError, match="layout"):
        bi.plan_layout(1000, 3, HBM, "sparse")
    for positions, columns in ((0, 1), (1 << 40, 1), (10, 0), (10, 4097)):
        with pytest.raises(MemoError):
            bi.plan_layout(positions, columns, HBM)


def test_null_outputs_are_allowed(bi):
    from memo_amd import _lib
    assert _lib.lib().memo_ms_plan_layout(1000, 3, HBM, 0, None, None) == 0


def test_auto_is_dense_wherever_dense_fits_else_coded_else_refused(bi):
    """against the two formulas restated above, at the exact byte where each stops fitting"""
    from memo_amd._lib import MemoError
    rng = np.random.default_rng(2048)
    for _ in range(300):
        positions = int(rng.integers(1, 1 << int(rng.integers(1, 36))))
        columns = int(rng.integers(1, 4097))
        dense, floor = _dense_need(positions, columns), _coded_floor(positions, columns)
        assert bi.plan_layout(positions, columns, dense) == ("dense", dense)
        assert bi.plan_layout(positions, columns, floor, "coded") == ("coded", floor)
        with pytest.raises(MemoError, match="device memory"):
            bi.plan_layout(positions, columns, dense - 1, "dense")
        with pytest.raises(MemoError, match="device memory"):
            bi.plan_layout(positions, columns, floor - 1, "coded")
        if floor < dense:
            assert bi.plan_layout(positions, columns, dense - 1) == ("coded", floor)
            assert bi.plan_layout(positions, columns, floor) == ("coded", floor)
        with pytest.raises(MemoError, match="device memory"):
            bi.plan_layout(positions, columns, min(dense, floor) - 1)


def test_more_free_memory_never_turns_an_accepted_shape_away(bi):
    from memo_amd._lib import MemoError
    rng = np.random.default_rng(7)

    def accepted(positions, columns, free, layout):
        try:
            return bi.plan_layout(positions, columns, free, layout)[0]
        except MemoError:
            return None
    for _ in range(200):
        positions = int(rng.integers(1, 1 << int(rng.integers(1, 40))))
        columns = int(rng.integers(1, 4097))
        frees = np.sort(rng.integers(0, 1 << int(rng.integers(20, 50)), 12)).tolist()
        frees += [_dense_need(positions, columns) + d for d in (-1, 0, 1)] + [_coded_floor(positions, columns) + d for d in (-1, 0, 1)]
        for layout in ("auto", "dense", "coded"):
            seen = [accepted(positions, columns, f, layout) for f in sorted(frees)]
            first = next((i for i, s in enumerate(seen) if s), len(seen))
            assert all(seen[first:]), (positions, columns, layout, seen)
            if layout == "auto" and "dense" in seen:           # ... nor dense back into coded
                assert all(s == "dense" for s in seen[seen.index("dense"):]), (positions, columns, seen)


def test_layout_info_struct_matches_the_header(tmp_path):
    """memo_ms_layout_info_t as a C compiler lays it out == the ctypes mirror"""
    from memo_amd import _lib
    names = [n for n, _ in _lib.MsLayoutInfo._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "memo_amd_dap.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(memo_ms_layout_info_t));\n'
                   + "".join(f'  printf("%zu\\n", offsetof(memo_ms_layout_info_t, {n}));\n' for n in names)
                   + '  printf("%d %d %d\\n", MEMO_MS_LAYOUT_AUTO, MEMO_MS_LAYOUT_DENSE, MEMO_MS_LAYOUT_CODED);\n  return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    assert int(out[0]) == C.sizeof(_lib.MsLayoutInfo)
    assert [int(x) for x in out[1:1 + len(names)]] == [getattr(_lib.MsLayoutInfo, n).offset for n in names]
    from memo_amd import build_index
    assert out[1 + len(names)].split() == [str(build_index.LAYOUTS[k]) for k in ("auto", "dense", "coded")]


def test_dap_layout_from_env(bi):
    assert bi.dap_layout_from_env({}) == "auto"
    assert bi.dap_layout_from_env({"MEMO_INDEX_DAP_LAYOUT": ""}) == "auto"
    for good in ("auto", "dense", "coded"):
        assert bi.dap_layout_from_env({"MEMO_INDEX_DAP_LAYOUT": good}) == good
    for bad in ("Coded ", "2", "sparse", " ", "CODED", "coded\n", "0"):
        with pytest.raises(bi.FastaError, match="MEMO_INDEX_DAP_LAYOUT"):
            bi.dap_layout_from_env({"MEMO_INDEX_DAP_LAYOUT": bad})


@pytest.mark.parametrize("bad", ["Coded ", "2", "sparse"])
def test_bad_layout_refused_by_memo_index(tmp_path, bad):
    example = [os.path.join(G.GOLD, "example_fa", f"ref_{i}.fa") for i in range(1, 6)]
    lst = tmp_path / "genome_list.txt"
    lst.write_text("".join(p + "\n" for p in example))
    env = dict(os.environ, MEMO_INDEX_DAP_LAYOUT=bad)
    r = subprocess.run([sys.executable, EXE, "index", "-g", str(lst), "-o", str(tmp_path / "w"), "-p", "test"],
                       capture_output=True, timeout=120, env=env)
    assert r.returncode == 1, r
    assert b"MEMO_INDEX_DAP_LAYOUT" in r.stderr and r.stderr.startswith(b"memo index: "), r.stderr
    assert r.stdout == b""
    assert not (tmp_path / "w" / "test.parquet").exists()
