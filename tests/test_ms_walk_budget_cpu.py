"""The walk budget of `memo index` without a GPU: MEMO_INDEX_WALK_BUDGET is checked before the device is touched, and
memo_ms_walk_info_t is laid out as its ctypes mirror says."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from tests import golden_util as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "memo")
BAD = ["-1", "x", " 5", "5 ", "+5", "1.5", "1e3", "0x10", "٥", "5\n", "9" * 19]
GOOD = {"0": 0, "1": 1, "64": 64, "007": 7, str(1 << 30): 1 << 30, str(1 << 40): 1 << 40}


@pytest.fixture(scope="module")
def bi():
    from memo_amd import _lib, build_index
    _lib.lib()
    return build_index


def test_walk_budget_from_env(bi):
    assert bi.walk_budget_from_env({}) is None
    assert bi.walk_budget_from_env({"MEMO_INDEX_WALK_BUDGET": ""}) is None
    for raw, value in GOOD.items():
        assert bi.walk_budget_from_env({"MEMO_INDEX_WALK_BUDGET": raw}) == value
    for bad in BAD:
        with pytest.raises(bi.FastaError, match="MEMO_INDEX_WALK_BUDGET"):
            bi.walk_budget_from_env({"MEMO_INDEX_WALK_BUDGET": bad})


def _no_device(monkeypatch):
    """every device entry point of the MS stage raises: what is refused must be refused before any of them"""
    from memo_amd import _lib
    L = _lib.lib()

    def boom(*a):
        raise AssertionError("the device was touched")
    for name in ("memo_ms_create", "memo_ms_create_layout", "memo_ms_add_genome", "memo_ms_add_records", "memo_dap_create"):
        monkeypatch.setattr(L, name, boom, raising=True)


@pytest.mark.parametrize("bad", BAD[:4])
def test_bad_budget_is_refused_before_any_device_call(bi, tmp_path, monkeypatch, capsys, bad):
    example = [os.path.join(G.GOLD, "example_fa", f"ref_{i}.fa") for i in range(1, 6)]
    lst = tmp_path / "genome_list.txt"
    lst.write_text("".join(p + "\n" for p in example))
    _no_device(monkeypatch)
    monkeypatch.setenv("MEMO_INDEX_WALK_BUDGET", bad)
    with pytest.raises(SystemExit) as exc:
        bi.main(["-g", str(lst), "-o", str(tmp_path / "w"), "-p", "test"])
    assert exc.value.code == 1
    out = capsys.readouterr()
    assert out.err.startswith("memo index: ") and "MEMO_INDEX_WALK_BUDGET" in out.err and out.out == ""
    assert not (tmp_path / "w" / "test.parquet").exists()


def test_good_budget_reaches_the_device_call(bi, tmp_path, monkeypatch):
    """an accepted value gets as far as creating the handle (which is made to raise here: there is no device), with the
    budget it names"""
    example = [os.path.join(G.GOLD, "example_fa", f"ref_{i}.fa") for i in range(1, 6)]
    lst = tmp_path / "genome_list.txt"
    lst.write_text("".join(p + "\n" for p in example))
    seen = []

    class Stop(Exception):
        pass

    def create(pivot, rec_begin, columns, device=0, chunk=0, layout="auto", walk_budget=None):
        seen.append(walk_budget)
        raise Stop()
    monkeypatch.setattr(bi, "MatchingStatistics", create)
    for raw, value in list(GOOD.items()) + [("", None)]:
        monkeypatch.setenv("MEMO_INDEX_WALK_BUDGET", raw)
        with pytest.raises(Stop):
            bi.main(["-g", str(lst), "-o", str(tmp_path / "w"), "-p", "test"])
        assert seen[-1] == value


def test_bad_budget_refused_by_the_command(tmp_path):
    example = [os.path.join(G.GOLD, "example_fa", f"ref_{i}.fa") for i in range(1, 6)]
    lst = tmp_path / "genome_list.txt"
    lst.write_text("".join(p + "\n" for p in example))
    env = dict(os.environ, MEMO_INDEX_WALK_BUDGET="-1")
    r = subprocess.run([sys.executable, EXE, "index", "-g", str(lst), "-o", str(tmp_path / "w"), "-p", "test"],
                       capture_output=True, timeout=120, env=env)
    assert r.returncode == 1, r
    assert b"MEMO_INDEX_WALK_BUDGET" in r.stderr and r.stderr.startswith(b"memo index: "), r.stderr
    assert r.stdout == b"" and not (tmp_path / "w" / "test.parquet").exists()


def test_walk_info_struct_matches_the_header(tmp_path):
    """memo_ms_walk_info_t as a C compiler lays it out == the ctypes mirror"""
    from memo_amd import _lib
    names = [n for n, _ in _lib.MsWalkInfo._fields_]
    assert names == ["text_reads", "max_chunk_text_reads", "seeds", "seed_text_reads", "budget"]
    src = tmp_path / "walk.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "memo_amd_dap.h"\nint main(void) {\n'
                   '  memo_ms_walk_info_t w;\n  printf("%zu\\n", sizeof(memo_ms_walk_info_t));\n'
                   + "".join(f'  printf("%zu %zu\\n", offsetof(memo_ms_walk_info_t, {n}), sizeof w.{n});\n' for n in names)
                   + '  w.budget = -1;\n  printf("%d\\n", w.budget < 0);\n  return 0;\n}\n')
    exe = str(tmp_path / "walk")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    assert int(out[0]) == C.sizeof(_lib.MsWalkInfo)
    want = [f"{getattr(_lib.MsWalkInfo, n).offset} {getattr(_lib.MsWalkInfo, n).size}" for n in names]
    assert out[1:1 + len(names)] == want
    assert out[1 + len(names)] == "1"                              # budget is signed
    # the two entry points refuse a NULL handle without touching a device
    L = _lib.lib()
    assert L.memo_ms_set_walk_budget(None, 0) == _lib.MEMO_EINVAL
    assert L.memo_ms_walk_info(None, C.byref(_lib.MsWalkInfo())) == _lib.MEMO_EINVAL
