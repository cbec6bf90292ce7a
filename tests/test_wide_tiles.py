"""Six-row views swept on radix-4 level arrays in wide tiles (memo_sweep_cons3t.hip: R4).  At k - 1 = 16 .. 31 a six-row view with few
rows per tile -- the live copy of config 3 -- is swept on three arrays of 1664 cells (blocks of 16, 4 and 1) instead of five doubling
arrays of 1024: 1568 positions per tile at k = 31 instead of 928.  A group carries its bucket mod 32 only, which places it within 1024
cells; the tile table's g_wrap says where a wide tile's slice passes that.  MEMO_OPT_WIDE_TILES 0 (option 7) keeps the doubling
tiles: the same bytes.  memo_index_info_t.last_tile_width says which geometry ran."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

OPT_BUILD_COST_PCT, OPT_WIDE_TILES = 3, 7
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _widths(k, cells):
    """positions per tile of the table-driven sweep: arrays of `cells`, halo (k - 1 + 3) & ~3 left, (k + 33) & ~3 right, whole buckets"""
    km1 = k - 1
    hl, hr = (km1 + 3) & ~3, (km1 + 31 + 3) & ~3
    return (cells - hl - hr) // 32 * 32


def test_the_option_and_the_field_are_declared():
    with open(os.path.join(ROOT, "include", "memo_amd.h")) as f:
        text = f.read()
    assert re.search(r"#define MEMO_OPT_WIDE_TILES 7\b", text)
    assert "MEMO_OPT_WIDE_TILES       1 (default)" in text
    assert re.search(r"int32_t last_tile_width;", text)
    assert (_widths(31, 1664), _widths(31, 1024)) == (1568, 928)
    assert _widths(17, 1664) == 1600 and _widths(21, 1664) == _widths(25, 1664) == 1568


@pytest.fixture(scope="module")
def memo():
    import memo_amd
    from memo_amd import _lib
    memo_amd.build()
    assert _lib.lib().memo_device_count() > 0, "no HIP device: the product has no CPU fallback"
    return memo_amd


def _both_ways(ix, qs, qe, k, n, dtype):
    """(wide-tile result, its info, doubling-tile result, its info)"""
    got = ix.conservation(qs, qe, k, n, dtype)
    inf = ix.info()
    assert ix.set_option(OPT_WIDE_TILES, 0) == 1
    ref = ix.conservation(qs, qe, k, n, dtype)
    inf0 = ix.info()
    assert ix.set_option(OPT_WIDE_TILES, 1) == 0
    return got, inf, ref, inf0


@pytest.mark.gpu
def test_config3_windows(memo, oracle):
    """config 3's rows (5 per position, 100 genomes) on a shorter chromosome: windows on and off the 4-position raster and the tile
    raster, short windows inside one tile, windows whose tiles' slices pass the 1024-cell wrap; uint8 and uint16 results"""
    from memo_amd import synth
    n, L = 100, 300_000
    num, den = synth.rows_per_position(n)
    wide = 0
    for k in (17, 21, 25, 31, 32):
        ix, (r0, r1) = synth.device_index(0, L, k, n, L, pack="dense")
        s, e, o = oracle.synth_rows(r0, r1 - r0, num, den, n)
        tw = _widths(k, 1664)
        windows = [(0, L), (1, L - 1), (3 * tw + 5, L - 7 * tw - 3), (37, tw + 1030), (50 * tw - 1, 50 * tw + 2),
                   (1024 + 3, 3 * tw + 1023), (9 * tw + 1021, 9 * tw + 1027), (L - tw - 2, L)]
        with ix:
            ix.set_option(OPT_BUILD_COST_PCT, 0)
            ix.prepare(k, n)
            ix.conservation(0, L, k, n, np.uint8)            # (the class's view, its copy without dead groups)
            for qs, qe in windows:
                want = oracle.conservation(*oracle.filter_rows(s, e, o, qs, qe, k), qs, qe, k, n, literal=False)
                for dt in (np.uint8, np.uint16):
                    got, inf, ref, inf0 = _both_ways(ix, qs, qe, k, n, dt)
                    assert got.dtype == dt and np.array_equal(got, want), (k, qs, qe, dt, int(np.argmax(got != want)))
                    assert np.array_equal(ref, got), (k, qs, qe, dt)
                    assert inf["last_sweep"] == 5 and inf0["last_sweep"] == 5, (k, inf)
                    if k <= 31:                                   # six-row views on the table-driven kernel: k - 1 <= 30 here
                        assert inf["last_variant"] == 3 and inf["last_view_rows_per_group"] == 6, (k, inf)
                        assert inf["last_tile_width"] == tw, (k, inf["last_tile_width"])
                        assert inf0["last_variant"] == 3 and inf0["last_tile_width"] == _widths(k, 1024), (k, inf0)
                        wide += 1
                    else:
                        assert inf["last_tile_width"] in (0, tw, _widths(k, 1024)), inf
    assert wide == 4 * 8 * 2


@pytest.mark.gpu
def test_tables_by_width(memo, oracle):
    """the tile table of the wide tiles is kept with the index like any other (keyed by its width): a later query finds it, a switch
    to the doubling tiles adds theirs; nothing changes a result"""
    from memo_amd import synth
    n, L, k = 100, 200_000, 31
    num, den = synth.rows_per_position(n)
    ix, (r0, r1) = synth.device_index(0, L, k, n, L, pack="dense")
    s, e, o = oracle.synth_rows(r0, r1 - r0, num, den, n)
    want = oracle.conservation(*oracle.filter_rows(s, e, o, 5, L - 9, k), 5, L - 9, k, n, literal=False)
    with ix:
        ix.set_option(OPT_BUILD_COST_PCT, 0)
        ix.prepare(k, n)
        first = ix.conservation(5, L - 9, k, n, np.uint8)        # (builds the copy: a new row source, its own table)
        before = ix.info()
        assert before["last_tile_width"] == 1568 and before["tile_tables_resident"] >= 1, before
        again = ix.conservation(5, L - 9, k, n, np.uint8)
        inf = ix.info()
        assert inf["tile_tables_resident"] == before["tile_tables_resident"] and inf["last_tile_width"] == 1568, inf
        assert ix.set_option(OPT_WIDE_TILES, 0) == 1
        old = ix.conservation(5, L - 9, k, n, np.uint8)
        assert ix.info()["last_tile_width"] == 928
        assert ix.info()["tile_tables_resident"] == before["tile_tables_resident"] + 1
        with pytest.raises(Exception):
            ix.set_option(OPT_WIDE_TILES, 2)
        for r in (first, again, old):
            assert np.array_equal(r, want)


@pytest.fixture(scope="module")
def real_index(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("real_wide"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "realistic_index.py"), "--length", "600000", "--genomes", "48",
                        "--out", out, "--threads", "8"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    json.loads(r.stdout.strip().splitlines()[-1])
    return out


@pytest.mark.gpu
def test_sequence_built_index(memo, oracle, real_index):
    """an index built from sequences (long overlaps, positions without rows): the same bytes from the wide and the doubling tiles,
    both the oracle's, whichever view the library picks"""
    z = np.load(os.path.join(real_index, "cons.npz"))
    s, e, o, n, L = z["start"], z["end"], z["annot"], int(z["num_docs"]), int(z["length"])
    from memo_amd.index import dense_rows_can_answer
    assert all(dense_rows_can_answer(len(s), int(s[0]), int(s[-1]), int(o.max()), k, n, False) for k in (17, 31))
    seen = set()
    with memo.DeviceIndex.from_host_packed(s, e, o, dense=True) as ix:
        ix.set_option(OPT_BUILD_COST_PCT, 0)
        for k in (17, 21, 25, 31):
            ix.prepare(k, n)
            ix.conservation(0, L, k, n)                           # (the class's copy, where its view has dead groups)
            for qs, qe in ((0, L), (L // 3 + 5, L // 3 + 70_001)):
                want = oracle.conservation(*oracle.filter_rows(s, e, o, qs, qe, k), qs, qe, k, n, literal=False)
                got, inf, ref, inf0 = _both_ways(ix, qs, qe, k, n, np.uint16)
                assert np.array_equal(got, want), (k, qs, qe, int(np.argmax(got != want)))
                assert np.array_equal(ref, got), (k, qs, qe)
                seen.add((k, inf["last_variant"], inf["last_tile_width"]))
    print("sequence-built index: (k, last_variant, last_tile_width)", sorted(seen))
