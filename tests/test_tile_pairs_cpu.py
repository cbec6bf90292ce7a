"""The wide tiles' pair kernel, what can be said of it without a device: the A/B entry and the switch are declared and bound, the
kernel keeps within the preloaded head, the tile table holds whole pairs.  (The launcher's rule needs a resident view and what a sweep
read of it: tests/test_tile_pairs_gpu.py::test_the_launchers_rule.)"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_the_entry_and_the_switch_are_declared():
    header = _read("include", "memo_amd_debug.h")
    assert re.search(r"int memo_debug_last_tiles_per_group\(const memo_index_t \*ix, int32_t \*out\);", header)
    assert "Bit 11 (2048)" in header and "sweep_conservation_wide_pair_kernel" in header
    debug = _read("memo_amd", "csrc", "memo_debug.hip")
    assert "int memo_debug_last_tiles_per_group(const memo_index_t *ix, int32_t *out)" in debug
    assert "(scatter >> 8) & 15" in debug                          # bits 8 .. 11 are the wide-tile sweep's


def test_the_python_host_binds_it():
    from memo_amd import _lib
    from memo_amd.index import DeviceIndex
    assert "memo_debug_last_tiles_per_group" in _lib.DEBUG_SYMBOLS
    assert "memo_debug_last_tiles_per_group" not in _lib.SYMBOLS   # (the product library exports no switch)
    assert callable(DeviceIndex.debug_last_tiles_per_group)


def test_the_info_struct_is_what_it_was():
    """who answered is asked through the A/B library: memo_index_info_t gained no field"""
    assert "tiles_per_group" not in _read("include", "memo_amd.h")


def test_the_kernel_keeps_the_head_and_the_table_whole_pairs():
    src = _read("memo_amd", "csrc", "memo_sweep_cons3t.hip")
    m = re.search(r"void sweep_conservation_wide_pair_kernel\((.*?)\) \{", src, re.S)
    assert m
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    # two pointers and ten 32-bit counts: the fourteen dwords gfx950 preloads, then SweepArgs
    assert len(params) == 13 and params[-1] == "const SweepArgs A"
    assert sum(2 if "*" in p else 1 for p in params[:-1]) == 14
    assert "s_load_dwordx16" in src                               # both descriptors of a pair in one scalar load
    assert "& ~(int64_t)1;" in src and "% 64" in src              # an even number of entries, a 64-byte aligned table
    assert os.path.exists(os.path.join(ROOT, "tools", "tile_pairs_ab.py"))
