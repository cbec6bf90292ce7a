"""CPU-only checks of the host side: the C-ABI library loads and exports every symbol the
header declares, the text emitters and the Parquet region slice match the golden vectors.
No compute call is made here (there is no GPU in this tier)."""
import os
import re

import numpy as np
import pytest

from tests import golden_util as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def memo():
    import memo_amd
    memo_amd.build()
    memo_amd.lib()
    return memo_amd


def _declared(*headers):
    out = set()
    for h in headers:
        src = open(os.path.join(ROOT, "include", h)).read()
        src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)            # declarations only, not comments
        out |= set(re.findall(r"\b(memo_[a-z_0-9]+)\s*\(", src))
    return out


def _exported(path):
    import subprocess
    txt = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in txt.splitlines() if ln.split()[-1].startswith("memo_")}


def test_library_exports_every_declared_symbol(memo):
    """the product library exports exactly what the product headers declare -- and none of the A/B
    switches, which live in include/memo_amd_debug.h and libmemo_amd_ab.so"""
    from memo_amd import _lib
    declared = _declared("memo_amd.h", "memo_amd_multi.h", "memo_amd_dap.h", "memo_amd_transport.h")
    assert declared, "no declarations parsed"
    assert declared == set(_lib.SYMBOLS), (declared ^ set(_lib.SYMBOLS))
    assert len(_declared("memo_amd.h")) <= 44          # (round 6: + memo_host_threads, the three *_rows forms)
    L = _lib.lib()
    for name in declared:
        assert hasattr(L, name)
    assert b"gfx950" in L.memo_version()
    assert _exported(_lib.SO_PATH) == declared
    debug = _declared("memo_amd_debug.h")
    assert debug == set(_lib.DEBUG_SYMBOLS) and all(n.startswith("memo_debug_") for n in debug)
    assert _exported(_lib.AB_SO_PATH) == declared | debug


def test_host_threads_follow_the_cpu_budget(memo):
    """memo_host_threads: the pool's size = min(CPUs allowed, cgroup CFS quota, 32), MEMO_HOST_THREADS overrides; the inputs come
    back through the pointers.  (The GPU boxes of the pool show 256 CPUs and grant 16: round 6, profiles/r06_oneshot.txt.)"""
    import ctypes as C
    import subprocess
    import sys
    from memo_amd import _lib
    allowed, quota = C.c_int32(-1), C.c_double(-1.0)
    n = _lib.lib().memo_host_threads(C.byref(allowed), C.byref(quota))
    assert 1 <= n <= 32 and allowed.value >= 1 and quota.value >= 0.0
    assert n <= allowed.value and (quota.value == 0.0 or n <= max(1, int(quota.value)))
    assert n == _lib.lib().memo_host_threads(None, None)
    code = ("import sys; sys.path.insert(0, %r)\nfrom memo_amd import _lib\nprint(_lib.lib().memo_host_threads(None, None))" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, MEMO_HOST_THREADS="5"))
    assert out.returncode == 0 and out.stdout.strip() == "5", out.stderr[-500:]


def test_cgroup_quota_parser(tmp_path):
    """memo_cpus.h against made-up cgroup trees: v2 `cpu.max` on the way up from the process's own group, v1 quota / period, `max`
    = no quota, the smallest quota wins -- compiled into a tiny program with the file-system root redirected"""
    import subprocess
    src = tmp_path / "q.cpp"
    hdr = open(os.path.join(ROOT, "memo_amd", "csrc", "memo_cpus.h")).read()
    hdr = hdr.replace('"/sys/fs/cgroup', 'std::string(getenv("FAKE_ROOT")) + "/sys/fs/cgroup').replace('fopen("/proc/self/cgroup", "r")',
                                                                                                      'fopen((std::string(getenv("FAKE_ROOT")) + "/proc/self/cgroup").c_str(), "r")')
    src.write_text(hdr + '\nint main() { printf("%.3f\\n", memo::cgroup_cpu_quota()); return 0; }\n')
    exe = str(tmp_path / "q")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", str(src), "-o", exe])

    def run(files):
        root = tmp_path / ("root%d" % len(os.listdir(tmp_path)))
        for path, text in files.items():
            f = root / path.lstrip("/")
            f.parent.mkdir(parents=True, exist_ok=True)
            f.write_text(text)
        return float(subprocess.run([exe], capture_output=True, text=True, check=True, env=dict(os.environ, FAKE_ROOT=str(root))).stdout)
    assert run({"/proc/self/cgroup": "0::/\n", "/sys/fs/cgroup/cpu.max": "1600000 100000\n"}) == 16.0        # the pool's GPU boxes
    assert run({"/proc/self/cgroup": "0::/\n", "/sys/fs/cgroup/cpu.max": "max 100000\n"}) == 0.0
    assert run({"/proc/self/cgroup": "0::/a/b\n", "/sys/fs/cgroup/cpu.max": "max 100000\n", "/sys/fs/cgroup/a/cpu.max": "400000 100000\n",
                "/sys/fs/cgroup/a/b/cpu.max": "800000 100000\n"}) == 4.0                                       # an ancestor's is smaller
    assert run({"/proc/self/cgroup": "4:cpu,cpuacct:/x\n1:name=systemd:/\n", "/sys/fs/cgroup/cpu/x/cpu.cfs_quota_us": "250000\n",
                "/sys/fs/cgroup/cpu/x/cpu.cfs_period_us": "100000\n"}) == 2.5                                  # cgroup v1
    assert run({"/proc/self/cgroup": "4:cpu,cpuacct:/x\n", "/sys/fs/cgroup/cpu/x/cpu.cfs_quota_us": "-1\n",
                "/sys/fs/cgroup/cpu/x/cpu.cfs_period_us": "100000\n"}) == 0.0
    assert run({}) == 0.0


def test_index_info_layout_matches_the_header(memo, tmp_path):
    """memo_index_info_t as a C compiler lays it out (gcc on include/memo_amd.h) == the ctypes mirror the Python host binds:
    size, every field's offset; the struct starts with its own size and a version, and the call refuses a struct whose size
    was never set (no index needed for that)"""
    import ctypes as C
    import subprocess
    from memo_amd import _lib
    names = [n for n, _ in _lib.IndexInfo._fields_]
    assert names[:2] == ["struct_bytes", "version"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "memo_amd.h"\nint main(void) {\n'
                   '  printf("%zu %d\\n", sizeof(memo_index_info_t), MEMO_INDEX_INFO_VERSION);\n' +
                   "".join(f'  printf("{n} %zu\\n", offsetof(memo_index_info_t, {n}));\n' for n in names) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    size, version = (int(x) for x in lines[0].split())
    assert size == C.sizeof(_lib.IndexInfo) and version == 5
    for ln in lines[1:]:
        if ln:
            n, off = ln.split()
            assert getattr(_lib.IndexInfo, n).offset == int(off), n
    assert _lib.lib().memo_index_get_info_v5(None, None) == _lib.MEMO_EINVAL


def test_no_gpu_fails_loudly(memo):
    from memo_amd import _lib
    if _lib.lib().memo_device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(memo.MemoError) as ei:
        memo.conservation([1], [2], [1], 0, 10, 3, 5)
    assert ei.value.code == _lib.MEMO_EHIP


def test_product_never_imports_oracle():
    for dp, _, fs in os.walk(os.path.join(ROOT, "memo_amd")):
        for f in fs:
            if f.endswith((".py", ".hip", ".h", ".cpp", "Makefile")):
                txt = open(os.path.join(dp, f)).read()
                assert "import oracle" not in txt and "from oracle" not in txt and "libmemo_oracle" not in txt, f


@pytest.mark.parametrize("c", G.cases(raises=False), ids=lambda c: c["name"])
def test_emitters_match_reference_text(c, memo):
    z = G.load(c)
    if c["membership"]:
        m = G.expected_matrix(c, z)
        W = (c["n"] + 31) // 32
        bits = np.zeros((m.shape[0], W), np.uint32)
        for g in range(c["n"]):
            bits[:, g >> 5] |= m[:, g].astype(np.uint32) << np.uint32(g & 31)
        text = memo.emit_membership(bits, c["n"])
        from memo_amd.index import bits_to_matrix
        assert np.array_equal(bits_to_matrix(bits, c["n"]), m)
    else:
        text = memo.emit_conservation(z["vec"].astype(np.uint16))
    assert G.sha(text) == c["sha256"]
    if "out" in c:
        assert text == G.out_bytes(c)


@pytest.mark.parametrize("c", G.cases(raises=False)[::7], ids=lambda c: c["name"])
def test_filter_pq_matches_reference_rows(c, memo):
    from memo_amd import memo_query as mq
    rec, qs, qe = G.region(c)
    z = G.load(c)
    path = os.path.join(G.GOLD, c["index"])
    rows = mq.filter_pq(path, rec, qs, qe + c["k"], spanning_rows=True)
    assert np.array_equal(rows.as_array(), z["rows"].reshape(-1, 3))
    live = mq.filter_pq(path, rec, qs, qe + c["k"])
    ref = z["rows"].reshape(-1, 3).astype(np.int64)
    keep = ref[:, 0] > qs
    assert np.array_equal(live.as_array().astype(np.int64), ref[keep])


def test_cli_argument_surface(memo):
    from memo_amd import memo_query as mq
    a = mq.parse_arguments(["-b", "x.parquet", "-o", "o.txt", "-n", "5", "-k", "31", "-r", "chr1:0-10"])
    assert (a.in_file, a.out_file, a.num_docs, a.k, a.genome_region, a.membership_query) == \
        ("x.parquet", "o.txt", "5", "31", "chr1:0-10", False)
    assert mq.parse_arguments(["-m", "-b", "x", "-o", "o", "-n", "5", "-k", "3", "-r", "c:1-2"]).membership_query
    with pytest.raises(SystemExit):
        mq.parse_arguments(["-b", "x.parquet"])          # -o -n -k -r are required (memo_query.py:79-83)


def test_synth_shard_rows_match_oracle(oracle):
    from memo_amd import synth
    for num_docs, qs, qe, k in ((10, 0, 5000, 31), (10, 1234, 7777, 21), (100, 300, 900, 101), (7, 5, 6, 3)):
        num, den = synth.rows_per_position(num_docs)
        pivot = 10_000
        r0, r1 = synth.shard_rows(qs, qe, k, num, den, pivot)
        total = synth.first_row_at_or_after(pivot, num, den)
        s, _, _ = oracle.synth_rows(0, total, num, den, num_docs)
        want = np.nonzero((s > qs) & (s < qe + k))[0]
        assert (r0, r1) == ((int(want[0]), int(want[-1]) + 1) if len(want) else (r0, r0))


def test_cli_front_end_usage_bytes():
    """bin/memo prints the reference dispatcher's usage text and exits 0 (src/memo:4-20,
    src/query.sh:14-33); fixtures captured from the reference's bash scripts."""
    import subprocess
    import sys
    exe = os.path.join(ROOT, "bin", "memo")
    for argv, fixture in (([], "memo_usage.txt"), (["-h"], "memo_usage.txt"), (["query"], "memo_query_usage.txt"),
                          (["query", "-h"], "memo_query_usage.txt"), (["bogus"], "memo_bogus.txt")):
        r = subprocess.run([sys.executable, exe] + argv, capture_output=True)
        assert r.returncode == 0
        assert r.stdout == open(os.path.join(G.GOLD, "cli", fixture), "rb").read(), argv
    r = subprocess.run([sys.executable, exe, "query", "-x"], capture_output=True)
    assert r.returncode == 0 and r.stdout == open(os.path.join(G.GOLD, "cli", "memo_query_usage.txt"), "rb").read()
    r = subprocess.run([sys.executable, exe, "query", "-b", "x.parquet"], capture_output=True)
    assert r.returncode == 2 and r.stdout == b"MEMO - conservation query\n"      # argparse: required flags


def test_region_chunks_equal_filter_pq(memo, tmp_path):
    """the streaming region slice (row groups pruned by statistics) returns filter_pq's rows"""
    import pyarrow as pa
    import pyarrow.parquet as pq
    from memo_amd import memo_query as mq
    rng = np.random.default_rng(8)
    tabs = []
    for name, n in (("chrA", 7300), ("chrB", 12000), ("chrC", 300)):   # (row groups of 1000: two of them hold two records)
        s = np.sort(rng.integers(1, 50_000, n))
        tabs.append(pa.table({"f0": pa.array([name] * n, pa.utf8()), "f1": s, "f2": s + rng.integers(0, 60, n),
                              "f3": rng.integers(1, 9, n)}))
    path = str(tmp_path / "multi_rg.parquet")
    pq.write_table(pa.concat_tables(tabs), path, row_group_size=1000, compression="ZSTD")
    assert pq.ParquetFile(path).metadata.num_row_groups >= 19
    for rec, qs, qe in (("chrB", 10_000, 20_031), ("chrA", 0, 50_031), ("chrC", 49_000, 60_000), ("chrB", 70_000, 70_100),
                        ("nochr", 0, 1000), ("chrA", 25_000, 25_001)):
        want = mq.filter_pq(path, rec, qs, qe)
        bound, chunks = mq.region_chunks(path, rec, qs, qe)
        got = list(chunks)
        cat = [np.concatenate([c[i] for c in got]) if got else np.zeros(0, np.int64) for i in range(3)]
        assert np.array_equal(cat[0], want.start) and np.array_equal(cat[1], want.end) and np.array_equal(cat[2], want.annot)
        assert len(want) <= bound
        if rec == "chrB" and qs == 10_000:
            assert bound < 12_000                      # pruning really skipped row groups
    # rows with a null name or a null start: the reference's filter drops them, and so does the slice (a group whose
    # statistics count a null is filtered row by row, never taken whole)
    s = np.arange(1, 4001)
    f0 = pa.array(["chrA"] * 1500 + [None] + ["chrA"] * 2499, pa.utf8())
    f1 = pa.array([None if i == 3200 else int(v) for i, v in enumerate(s)], pa.int64())
    path2 = str(tmp_path / "nulls.parquet")
    pq.write_table(pa.table({"f0": f0, "f1": f1, "f2": s + 3, "f3": s % 7}), path2, row_group_size=1000)
    want = mq.filter_pq(path2, "chrA", 0, 10_000)
    got = list(mq.region_chunks(path2, "chrA", 0, 10_000)[1])
    assert len(want) == 3998 and np.array_equal(np.concatenate([c[0] for c in got]), want.start)
    for c in G.cases(raises=False)[::23]:
        rec, qs, qe = G.region(c)
        want = mq.filter_pq(os.path.join(G.GOLD, c["index"]), rec, qs, qe + c["k"])
        _, chunks = mq.region_chunks(os.path.join(G.GOLD, c["index"]), rec, qs, qe + c["k"])
        got = list(chunks)
        assert sum(len(x[0]) for x in got) == len(want)


def test_synth_host_rows_equal_oracle(oracle):
    from memo_amd import synth
    for rb, n, num, den, nd in ((0, 5000, 5, 1, 100), (123456789, 3000, 1, 2, 10), (7_000_000_000, 2000, 25, 1, 500)):
        got = synth.host_rows(rb, n, num, den, nd)
        want = oracle.synth_rows(rb, n, num, den, nd)
        assert all(np.array_equal(g, w) for g, w in zip(got, want))


def test_region_chunks_without_statistics_or_with_dictionary_f0(memo, tmp_path):
    """index files written by other tools: no row-group statistics (nothing can be pruned), f0
    dictionary-encoded -- the slice is the same"""
    import pyarrow as pa
    import pyarrow.parquet as pq
    from memo_amd import memo_query as mq
    rng = np.random.default_rng(5)
    n = 9000
    s = np.sort(rng.integers(1, 30_000, n))
    names = np.where(np.arange(n) < 6000, "chr1", "chr2")
    order = np.lexsort((s, names))
    tab = pa.table({"f0": pa.array(names[order]).dictionary_encode(), "f1": s[order], "f2": s[order] + 3,
                    "f3": rng.integers(1, 5, n)})
    for kw in (dict(write_statistics=False), dict(use_dictionary=True), dict(compression="NONE")):
        path = str(tmp_path / "x.parquet")
        pq.write_table(tab, path, row_group_size=700, **kw)
        for rec, qs, qe in (("chr1", 100, 9000), ("chr2", 0, 40_000), ("chr3", 0, 10)):
            want = mq.filter_pq(path, rec, qs, qe)
            bound, chunks = mq.region_chunks(path, rec, qs, qe)
            got = list(chunks)
            cat = np.concatenate([c[0] for c in got]) if got else np.zeros(0, np.int64)
            assert np.array_equal(cat, want.start) and len(want) <= bound


def test_transport_coding_choice_model():
    """memo_amd.shard.pick_coding: the step model bench.py uses to choose what a slice travels as.
    Inputs = the figures measured on config 3: fewer bytes win while rank 0's
    decoding of world - 1 slices stays under the link time."""
    from memo_amd import shard
    sweep = 0.37e-3
    usable = {"plain": (100_000_000, 0.0, 0.0),
              "nibble": (53_101_352, 0.031e-3, 0.108e-3),
              "dense": (41_250_080, 0.058e-3, 0.153e-3)}
    picks = {w: shard.pick_coding(w, sweep, usable)[0] for w in (2, 4, 8)}
    assert picks == {2: "dense", 4: "dense", 8: "nibble"}
    best, model = shard.pick_coding(8, sweep, usable)
    assert abs(model["plain"] - 100e6 / 75e9) < 1e-9                      # link-bound
    assert abs(model["dense"] - (sweep + 7 * 0.058e-3)) < 1e-9           # rank 0's decoding
    assert abs(model["nibble"] - 53_101_352 / 75e9) < 1e-9               # link-bound
    # a slow link makes bytes matter more; a fast one makes the coding pointless
    assert shard.pick_coding(8, sweep, usable, link=20e9)[0] == "dense"
    assert shard.pick_coding(2, sweep, usable, link=1e12)[0] == "plain"
    assert shard.modelled_step(1, sweep, 10, 1.0, 0.0) == sweep          # nobody to decode for
    # coding and root weight together: at 8 GPUs the dense coding pays once rank 0 sweeps less than a full share
    coding, w, rate = shard.pick_plan(8, sweep, usable)
    assert coding == "dense" and w < 1.0
    assert abs(rate - (7 + w) / max(sweep + 0.153e-3, w * sweep + 7 * 0.058e-3, 41_250_080 / 75e9)) < 1e-6
    assert shard.pick_plan(2, sweep, usable)[:2] == ("dense", 1.0)       # one slice to decode: nothing to give up
    assert shard.pick_plan(1, sweep, usable)[1] == 1.0


def test_split_window_rule(memo):
    """memo_split_window (include/memo_amd_multi.h; memo_amd.shard.split_window calls it): contiguous cover
    of [qs, qe), part lengths multiples of the alignment except the tail, equal parts at weight 1 (the
    round-1 Python rule), a lighter first part for weights < 1, empty windows past the end."""
    from memo_amd import shard
    rng = np.random.default_rng(4)
    for _ in range(400):
        qs = int(rng.integers(-1000, 10 ** 9))
        L = int(rng.choice([0, 1, 7, 8, 9, 1000, 123_457, 10 ** 8]))
        world = int(rng.integers(1, 10))
        align = int(rng.choice([1, 8, 32]))
        w = float(rng.choice([1.0, 0.0, 0.25, 0.5, 0.9, 2.0]))
        wins, per = shard.split_window(qs, qs + L, world, align=align, root_weight=w)
        assert len(wins) == world and wins[0][0] == qs and wins[-1][1] == qs + L
        assert all(a <= b for a, b in wins) and all(wins[i][1] == wins[i + 1][0] for i in range(world - 1))
        lens = [b - a for a, b in wins]
        nonempty = [x for x in lens if x]
        assert all(x % align == 0 for x in nonempty[:-1]) and per % align == 0 and per >= max(lens)
        if w == 1.0:                                   # the equal split of round 1
            p = -(-L // world)
            p = -(-p // align) * align if p else 0
            assert wins == [(min(qs + g * p, qs + L), min(qs + (g + 1) * p, qs + L)) for g in range(world)]
        if world > 1 and L >= 10 ** 6:
            if w < 1.0:
                assert lens[0] <= lens[1] and abs(lens[0] - w * lens[1]) <= align + w * align
            if w == 0.0:
                assert lens[0] == 0
    with pytest.raises(memo.MemoError):
        shard.split_window(0, 10, 2, root_weight=-1.0)


def _cache_header(cache, body):
    """a header that describes a (zero-filled) body of `body` bytes: 10 rows in format 4, a 2-entry table"""
    return {"version": cache.VERSION, "record": "?", "source": None, "rows": 10, "format": 4, "bucket_shift": 5, "buckets": 2,
            "min_start": 0, "max_start": 31, "max_annot": 3, "long_rows": 0, "off_pk": cache.HEADER_BYTES,
            "off_pa": cache.HEADER_BYTES + 40, "off_p3": cache.HEADER_BYTES + 48, "off_boff3": cache.HEADER_BYTES + 80,
            "rows3": 10, "off_boff": cache.HEADER_BYTES + 80, "off_long": cache.HEADER_BYTES + 96, "bytes": cache.HEADER_BYTES + body}


def test_sidecar_cache_lock_and_negative_marker(memo, tmp_path, monkeypatch):
    """round-2 ADVICE: one builder per record at a time (O_EXCL lock; a stale one is replaced), and a record whose rows
    cannot be packed is remembered (keyed by the Parquet file's size / mtime) so that no later query rebuilds or respawns."""
    from memo_amd import cache
    index = tmp_path / "idx.parquet"
    index.write_bytes(b"not really parquet")
    f = str(index)
    assert cache.take_lock(f, "chr1") and not cache.take_lock(f, "chr1")
    assert cache.take_lock(f, "chr2")                                       # per record
    spawned = []
    monkeypatch.setattr("subprocess.Popen", lambda *a, **k: spawned.append(a))
    assert cache.build_in_background(f, "chr1") is False and not spawned    # somebody holds the lock: no second builder
    cache.release_lock(f, "chr1")
    assert cache.build_in_background(f, "chr1") is True and len(spawned) == 1
    assert not cache.take_lock(f, "chr1")                                   # the spawned builder owns it now
    old = cache.LOCK_STALE_SECONDS
    monkeypatch.setattr(cache, "LOCK_STALE_SECONDS", -1.0)
    assert cache.take_lock(f, "chr1")                                       # a builder that died an hour ago
    monkeypatch.setattr(cache, "LOCK_STALE_SECONDS", old)
    cache.release_lock(f, "chr1")
    assert not cache.uncacheable(f, "chr1")
    cache._mark_uncacheable(f, "chr1", "annot > 4095")
    assert cache.uncacheable(f, "chr1") and not cache.uncacheable(f, "chr2")
    assert cache.build_in_background(f, "chr1") is False and len(spawned) == 1
    index.write_bytes(b"the index file changed, the verdict is void")
    assert not cache.uncacheable(f, "chr1")


def test_sidecar_cache_file_validation(memo, tmp_path, monkeypatch):
    """memo_amd.cache: a cache file is visible only while its header matches the index file it was made from
    (size + mtime_ns), its own size, its format version and its record; anything else reads as "no cache".
    (Reading rows out of a valid file needs the GPU: tests/test_gpu_parity.py::test_sidecar_cache_round_trip.)"""
    import json
    from memo_amd import cache
    index = tmp_path / "idx.parquet"
    index.write_bytes(b"not really parquet")
    path = cache.cache_path(str(index), "chr 1/x")
    assert path.startswith(str(index) + ".memo" + os.sep) and "/" not in os.path.basename(path) and " " not in os.path.basename(path)
    assert cache._open(str(index), "chr 1/x") is None                        # no file
    os.makedirs(os.path.dirname(path))

    def write(head, body=b"\0" * 100):
        blob = cache.MAGIC + json.dumps(head).encode()
        with open(path, "wb") as fh:
            fh.write(blob.ljust(cache.HEADER_BYTES, b"\0") + body)
    good = dict(_cache_header(cache, 100), record="chr 1/x", source=cache._source_key(str(index)))
    write(good)
    assert cache._open(str(index), "chr 1/x") is not None
    # round-2 ADVICE: a header whose `bytes` still matches but whose offsets / counts point outside the file must make
    # the cache invisible (it used to reach struct.unpack_from and raw pointer arithmetic)
    for bad in (dict(good, rows=1000), dict(good, off_pk=10), dict(good, off_boff=cache.HEADER_BYTES + 96),
                dict(good, buckets=1), dict(good, long_rows=3), dict(good, rows=-1), dict(good, format=5),
                dict(good, off_p3=cache.HEADER_BYTES + 90), dict(good, rows3=11), dict(good, off_boff3=cache.HEADER_BYTES + 90),
                dict(good, bucket_shift=40), {k: v for k, v in good.items() if k != "off_long"}):
        write(bad)
        assert cache._open(str(index), "chr 1/x") is None, bad
    write(good)
    # the file-name form of a record is injective ('_' is escaped too)
    assert cache.cache_path(str(index), "chr 1") != cache.cache_path(str(index), "chr_201")
    assert len({cache.cache_path(str(index), r) for r in ("a_b", "a b", "a_5fb", "a/b", "A_B")}) == 5
    assert cache._open(str(index), "chr2") is None                           # another record's name
    for bad in (dict(good, version=cache.VERSION + 1), dict(good, record="other"), dict(good, bytes=5),
                dict(good, source={"size": 1, "mtime_ns": 2})):
        write(bad)
        assert cache._open(str(index), "chr 1/x") is None
    write(good)
    with open(path, "r+b") as fh:
        fh.write(b"XXXXXXXX")                                                # magic gone
    assert cache._open(str(index), "chr 1/x") is None
    write(good)
    index.write_bytes(b"the index file changed")                            # size / mtime differ now
    assert cache._open(str(index), "chr 1/x") is None
    for v, want in (("0", "off"), ("off", "off"), ("read", "read"), ("sync", "sync"), ("1", "on"), ("", "on")):
        monkeypatch.setenv("MEMO_CACHE", v)
        assert cache.mode() == want


def test_fast_query_path_declines_what_it_cannot_answer(tmp_path, monkeypatch):
    """memo_amd._fastquery (the ctypes-only cache-hit path of `memo query`) keeps the same file rules as memo_amd.cache
    and answers False -- "take the regular path" -- before it touches the library for everything else: no cache,
    a stale or foreign one, caching off, k > 256, sharded runs, arguments it cannot parse.  It must not import NumPy."""
    import json
    import subprocess
    import sys
    from memo_amd import _fastquery as fq, cache
    assert (fq.VERSION, fq.HEADER_BYTES, fq.MAGIC) == (cache.VERSION, cache.HEADER_BYTES, cache.MAGIC)
    index = tmp_path / "idx.parquet"
    index.write_bytes(b"not really parquet")
    out = str(tmp_path / "out.txt")
    for record in ("chr1", "chr 1/x", ""):
        assert fq._cache_path(str(index), record) == cache.cache_path(str(index), record)
    monkeypatch.setenv("MEMO_CACHE", "read")
    assert fq.try_query(str(index), "chr1:0-100", "31", "5", out, False) is False          # no cache file
    path = cache.cache_path(str(index), "chr1")
    os.makedirs(os.path.dirname(path))
    st = os.stat(index)
    good = dict(_cache_header(cache, 100), record="chr1", source={"size": st.st_size, "mtime_ns": st.st_mtime_ns})

    def write(head):
        with open(path, "wb") as fh:
            fh.write((cache.MAGIC + json.dumps(head).encode()).ljust(cache.HEADER_BYTES, b"\0") + b"\0" * 100)
    write(good)
    assert fq._open(str(index), "chr1") is not None
    for bad in (dict(good, version=cache.VERSION + 1), dict(good, record="other"), dict(good, bytes=5),
                dict(good, source={"size": 1, "mtime_ns": 2}), dict(good, rows=1000), dict(good, off_boff=cache.HEADER_BYTES + 96),
                dict(good, buckets=1), dict(good, off_p3=1 << 40)):
        write(bad)
        assert fq._open(str(index), "chr1") is None
        assert fq.try_query(str(index), "chr1:0-100", "31", "5", out, False) is False
    write(good)
    for region, k, n in (("chr1", "31", "5"), ("chr1:5", "31", "5"), ("chr1:a-b", "31", "5"), ("chr1:0-100", "300", "5"),
                         ("chr1:0-100", "1", "5"), ("chr1:0-100", "x", "5"), ("chr1:0-100", "31", "many")):
        assert fq.try_query(str(index), region, k, n, out, False) is False
    for var, val in (("MEMO_CACHE", "0"), ("MEMO_QUERY_WIDE", "1"), ("WORLD_SIZE", "2"), ("MEMO_FORCE_SHARDED", "1")):
        monkeypatch.setenv(var, val)
        assert fq.try_query(str(index), "chr1:0-100", "31", "5", out, False) is False
        monkeypatch.delenv(var)
        monkeypatch.setenv("MEMO_CACHE", "read")
    assert not os.path.exists(out)
    code = "import sys; from memo_amd import _fastquery; assert 'numpy' not in sys.modules and 'pyarrow' not in sys.modules"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert subprocess.run([sys.executable, "-c", code], cwd=root).returncode == 0


def _run_bench_parent(tmp_path, stub_body, extra_env=None, args=("--gpus", "8", "--steps", "20", "--warmup", "5")):
    """`python bench.py --gpus N` with no WORLD_SIZE: the parent of bench.launch_ranks(), with a stub in the
    place of `python -m torch.distributed.run ... bench.py` (MEMO_BENCH_CHILD_CMD)."""
    import json
    import subprocess
    import sys
    stub = tmp_path / "stub_child.py"
    stub.write_text(stub_body)
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["MEMO_BENCH_CHILD_CMD"] = json.dumps([sys.executable, str(stub)])
    env["MEMO_BENCH_ASSUME_DEVICES"] = "8"
    env.update(extra_env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                          env=env, timeout=120)


def test_bench_launches_its_own_ranks_and_relays_the_line(tmp_path):
    """The driver spells N > 1 as `python bench.py --gpus N ...` (no torchrun in front, no WORLD_SIZE): the parent
    starts ONE child process, hands it the same arguments, relays rank 0's single JSON line (banners a rank
    printed on fd 1 go to stderr) and exits with the child's code.  The parent must not have loaded the HIP
    runtime, torch.cuda or the library by then (it only counts devices)."""
    import json
    r = _run_bench_parent(tmp_path, (
        "import json, os, sys\n"
        "print('some RCCL banner on fd 1')\n"
        "print(json.dumps({'metric': 'stub', 'argv': sys.argv[1:], 'value': 1.5, 'n_gpus': 8,\n"
        "                  'ipc': os.environ.get('HSA_ENABLE_IPC_MODE_LEGACY')}))\n"))
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == 1
    j = json.loads(lines[0])
    assert j["argv"] == ["--gpus", "8", "--steps", "20", "--warmup", "5"] and j["value"] == 1.5 and j["ipc"] == "0"
    assert "some RCCL banner" in r.stderr and "some RCCL banner" not in r.stdout


def test_bench_launcher_exit_codes(tmp_path):
    # the child's failure is the parent's
    r = _run_bench_parent(tmp_path, "import sys\nsys.stderr.write('rank 3 died\\n')\nsys.exit(7)\n")
    assert r.returncode == 7 and r.stdout == "" and "rank 3 died" in r.stderr
    # a child that succeeds without the line is an error too
    r = _run_bench_parent(tmp_path, "print('no json here')\n")
    assert r.returncode == 3 and r.stdout == ""
    # fewer GPUs than asked for: one clear line, non-zero, no child started
    r = _run_bench_parent(tmp_path, "raise SystemExit('the child must not run')\n", {"MEMO_BENCH_ASSUME_DEVICES": "1"})
    assert r.returncode == 2 and "--gpus 8 but 1 GPU(s) visible" in r.stderr and "must not run" not in r.stderr
    # --launch: the same path at N = 1 (what tools/gpu_torchrun.sh uses on the one-GPU pool); the flag itself is
    # not handed down, or the child would launch again
    r = _run_bench_parent(tmp_path, "import json, sys\nprint(json.dumps({'argv': sys.argv[1:]}))\n",
                          args=("--gpus", "1", "--launch", "--force-dist"))
    assert r.returncode == 0 and '"--launch"' not in r.stdout and '"--force-dist"' in r.stdout


def test_bench_parent_does_not_touch_the_gpu_stack(tmp_path):
    """launch_ranks() runs before numpy / torch / memo_amd are imported by bench.py itself."""
    import subprocess
    import sys
    code = ("import sys, os\nsys.argv = ['bench.py', '--gpus', '8']\n"
            "os.environ['MEMO_BENCH_ASSUME_DEVICES'] = '8'\n"
            "os.environ['MEMO_BENCH_CHILD_CMD'] = '[\"%s\", \"-c\", \"print(chr(123)+chr(125))\"]'\n"
            "os.environ.pop('WORLD_SIZE', None); os.environ.pop('RANK', None)\n"
            "sys.path.insert(0, %r)\nimport bench\n"
            "try:\n    bench.main()\nexcept SystemExit as e:\n    assert e.code == 0, e.code\n"
            "bad = [m for m in ('torch', 'memo_amd', 'numpy') if m in sys.modules]\n"
            "assert not bad, bad\n") % (sys.executable, ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr


def test_bench_dump_outputs(tmp_path, monkeypatch):
    """--dump-outputs: the whole result while it fits the budget, else one position per equal stratum with a fixed seed
    (the same positions however the result is split into pieces); every value exact (uint8 / uint16 counts as float32,
    uint32 membership words as float64); the file within the budget."""
    import types
    import torch
    import bench
    rng = np.random.default_rng(5)
    cons = rng.integers(0, 256, 100_000).astype(np.uint8)
    e = bench.dump_outputs(types.SimpleNamespace(membership=False, narrow=True), [torch.from_numpy(cons)], str(tmp_path / "a"))
    got = np.load(tmp_path / "a" / "conservation.npy")
    assert got.dtype == np.float32 and np.array_equal(got, cons) and e["sample"] is None and e["positions"] == 100_000
    memb = rng.integers(0, 2 ** 32, (5000, 3), dtype=np.uint64).astype(np.uint32)
    bench.dump_outputs(types.SimpleNamespace(membership=True, narrow=False), [torch.from_numpy(memb.view(np.int32))], str(tmp_path / "m"))
    got = np.load(tmp_path / "m" / "membership.npy")
    assert got.dtype == np.float64 and got.shape == (5000, 3) and np.array_equal(got.astype(np.uint32), memb)
    monkeypatch.setattr(bench, "DUMP_BYTES", 4096 + 4 * 1000)
    wide = rng.integers(0, 65536, 100_000).astype(np.uint16)
    R = types.SimpleNamespace(membership=False, narrow=False)
    e = bench.dump_outputs(R, [torch.from_numpy(wide[:30_001].view(np.int16)), torch.from_numpy(wide[30_001:].view(np.int16))],
                           str(tmp_path / "b"))
    bench.dump_outputs(R, [torch.from_numpy(wide.view(np.int16))], str(tmp_path / "c"))
    b, c = (np.load(tmp_path / d / "conservation.npy") for d in "bc")
    assert len(b) == 1000 and e["sample"] and e["positions"] == 100_000 and np.array_equal(b, c)
    assert all(v in wide[i * 100:(i + 1) * 100] for i, v in enumerate(b.astype(np.uint16)))
    assert os.path.getsize(tmp_path / "b" / "conservation.npy") <= bench.DUMP_BYTES


def _device_disassembly(obj, tmp_path):
    """gfx950 disassembly of the device code inside a hipcc object file"""
    import shutil
    import subprocess
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    if not os.path.exists(objdump):
        pytest.skip("llvm-objdump not installed")
    local = str(tmp_path / os.path.basename(obj))
    shutil.copy(obj, local)
    subprocess.run([objdump, "--offloading", local], capture_output=True, check=True)      # extracts the bundles beside it
    dev = [f for f in os.listdir(tmp_path) if "amdgcn" in f and "gfx950" in f]
    assert len(dev) == 1, dev
    return subprocess.run([objdump, "-d", str(tmp_path / dev[0])], capture_output=True, text=True, check=True).stdout


@pytest.mark.parametrize("obj", ["memo_sweep_cons.o", "memo_sweep_cons3t.o", "memo_sweep_memb.o"])
def test_row_blocks_run_with_every_lane_enabled(memo, tmp_path, obj):
    """The branch-free row blocks narrow EXEC themselves (v_cmpx) and restore it with `s_mov_b64 exec, -1` -- which is
    only right when every lane was enabled on entry, something the compiler is never told (round-2 VERDICT, weak 6) -- or,
    the membership blocks since round 6, from the SGPR pair they saved it in.
    Scan the shipped gfx950 code: inside every kernel, no v_cmpx may sit between an `s_and_saveexec_b64` (or another
    instruction that narrows EXEC) and the `s_or_b64 exec, exec, ...` that restores it, and every v_cmpx region must
    end in `s_mov_b64 exec, -1` before the next instruction that reads EXEC as a mask."""
    text = _device_disassembly(os.path.join(ROOT, "memo_amd", "csrc", obj), tmp_path)
    kernels, cur = {}, None
    for ln in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", ln)
        if m:
            cur = kernels.setdefault(m.group(1), [])
            continue
        m = re.match(r"^\s+([a-z_0-9]+)\s*(.*?)\s*//", ln)
        if m and cur is not None:
            cur.append((m.group(1), m.group(2)))
    blocks = 0
    for name, ins in kernels.items():
        if not any(op.startswith("v_cmpx") for op, _ in ins):
            continue
        # EXEC is all ones at a kernel's entry (whole waves: every launch is a multiple of 64 threads); s_and_saveexec
        # opens a divergent region that the matching s_or_b64 exec, exec, <saved> closes; inside one, further narrowing
        # (s_and_b64 / s_andn2_b64 exec, exec, ...) is undone by that same s_or; outside any, it would be permanent
        saved, narrowed, in_block, kept = [], False, False, None
        for op, args in ins:
            a = args.replace(" ", "")
            if op.startswith("s_and_saveexec") or op.startswith("s_or_saveexec") or op.startswith("s_andn2_saveexec"):
                assert not in_block, (name, op, args)
                saved.append(a.split(",")[0])
            elif op in ("s_andn2_b64", "s_and_b64", "s_xor_b64") and a.startswith("exec,"):
                assert not in_block, (name, op, args)
                if not saved:
                    narrowed = True
            elif op == "s_or_b64" and a.startswith("exec,exec,"):
                if saved and saved[-1] == a.split(",")[2]:
                    saved.pop()
                elif a.split(",")[2] in saved:            # (a region closed out of order: everything inside it is closed too)
                    del saved[saved.index(a.split(",")[2]):]
            elif op.startswith("v_cmpx"):
                assert not saved and not narrowed, \
                    f"{name}: {op} {args} inside a divergent region {saved} (EXEC is not all ones there)"
                if not in_block:
                    blocks += 1
                in_block = True
            elif op == "s_mov_b64" and a == "exec,-1":
                in_block = narrowed = False
            elif op == "s_mov_b64" and re.fullmatch(r"s\[\d+:\d+\],exec", a) and not in_block:
                kept = a.split(",")[0]          # (the membership row blocks: EXEC kept in an SGPR pair in front of the block ...)
            elif op == "s_mov_b64" and kept and a == "exec," + kept:
                in_block = narrowed = False     # (... and put back from it at the end: round 6)
            elif in_block:
                assert not op.startswith("s_cbranch") and op not in ("s_barrier", "s_endpgm"), \
                    f"{name}: {op} inside a row block, before EXEC is restored"
        assert not in_block, name
    assert blocks >= 100, blocks          # (the scan found the blocks it is about)
