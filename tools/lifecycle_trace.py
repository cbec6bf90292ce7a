#!/usr/bin/env python
"""tools/lifecycle_trace.py -- one line per step of an index's life, for comparing two builds of the library byte for byte.

Drives indexes through every call that makes, changes or drops device data -- create -> upload -> finalize -> pack ->
pack_dense -> prepare -> queries -> each row-changing call -> ..., the builder (4-byte words and dense rows), export / import
(words and dense rows, with and without rows that have end < start, whole and as a region slice, the 6-byte format) and every
memo_index_set_option -- and prints after each call every field of memo_index_info that is not a time, plus the sha256 of every
result and of every exported array.  device_bytes and side_bytes are among the fields: a buffer that is dropped late, early or
not at all shows.  Choose the build with MEMO_AMD_LIB; `diff` the outputs of two builds run on the same box.

    python tools/lifecycle_trace.py > trace.txt
"""
import ctypes as C
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import memo_amd                                    # noqa: E402
from memo_amd import _lib, synth                   # noqa: E402
from memo_amd.index import DeviceIndex             # noqa: E402

TIMES = ("pack_ms", "last_view_ms")
N, L = 100, 400_000
SEED_B = 0x5EED


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def show(tag, ix):
    inf = ix.info()
    print(tag, " ".join(f"{f}={v}" for f, v in inf.items() if f not in TIMES), flush=True)


def call(tag, ix, fn, *args):
    """a raw ABI call: its return code and, when it fails, its message; then the index's state"""
    rc = fn(*args)
    print(tag, "rc", rc, _lib.lib().memo_last_error().decode() if rc < 0 else "", flush=True)
    if ix is not None:
        show(tag, ix)
    return rc


def queries(tag, ix, n=N, length=L):
    for kind, k, qs, qe in (("cons", 31, 0, length), ("cons", 17, 0, length), ("cons", 31, 1003, length // 3), ("cons", 101, 0, length),
                            ("cons", 64, -50, length // 2), ("memb", 31, 1000, length // 4), ("memb", 101, 1000, length // 8)):
        try:
            got = ix.conservation(qs, qe, k, n) if kind == "cons" else ix.membership(qs, qe, k, n)
            print(tag, kind, k, qs, qe, sha(got))
        except memo_amd.MemoError as ex:
            print(tag, kind, k, qs, qe, "refused:", ex)
        show(f"{tag} after {kind} k={k}", ix)


def host_rows(seed, longs):
    num, den = synth.rows_per_position(N)
    r0, r1 = synth.shard_rows(0, L, 64, num, den, L)
    s, e, o = synth.host_rows(r0, r1 - r0, num, den, N, seed)
    if longs:                                      # rows with end < start, spread over the chromosome
        e[7::len(e) // longs] = s[7::len(e) // longs] - 3
    return s, e, o


def ptr(a):
    return a.ctypes.data if a is not None and len(a) else None


def export_packed(tag, ix):
    inf = ix.info()
    rows, nb, nl, fmt = inf["rows"], inf["buckets"], inf["long_rows"], inf["packed_format"]
    pk, pa = np.empty(rows, np.uint32), np.empty(rows if fmt == 6 else 0, np.uint16)
    boff, longs = np.empty(nb, np.int64), np.empty(3 * nl, np.int64)
    rc = call(f"{tag} export_packed", ix, _lib.lib().memo_index_export_packed, ix._h, ptr(pk), ptr(pa), ptr(boff), ptr(longs))
    if rc:
        return None
    # (finalize collects the rows with end < start with an atomic counter: their order is not defined, their set is)
    print(tag, "exported", sha(pk), sha(pa), sha(boff), sha(np.sort(longs.reshape(3, nl).T.copy().view("i8,i8,i8"), axis=0)), nl)
    return pk, (pa if fmt == 6 else None), boff, longs, inf


def export_dense(tag, ix):
    inf = ix.info()
    rows3, nb, nl = inf["dense_row_count"], inf["buckets"], inf["long_rows"]
    p3, boff3, longs = np.empty(4 * ((rows3 + 4) // 5), np.uint32), np.empty(nb, np.int64), np.empty(3 * nl, np.int64)
    rc = call(f"{tag} export_dense", ix, _lib.lib().memo_index_export_dense, ix._h, ptr(p3), ptr(boff3), ptr(longs))
    if rc:
        return None
    print(tag, "exported", sha(p3), sha(boff3), sha(np.sort(longs.reshape(3, nl).T.copy().view("i8,i8,i8"), axis=0)), nl)
    return p3, boff3, longs, inf


def import_packed(tag, exported, b_lo, b_hi):
    pk, pa, boff, longs, inf = exported
    r0, r1 = int(boff[b_lo]), int(boff[b_hi])
    table = np.ascontiguousarray(boff[b_lo:b_hi + 1])
    shift = inf["bucket_shift"]
    h = C.c_void_p()
    rc = call(f"{tag} import_packed", None, _lib.lib().memo_index_import_packed, r1 - r0, 0, shift, b_lo, ptr(pk[r0:r1]),
              ptr(pa[r0:r1]) if pa is not None else None, ptr(table), len(table) + 1, r0, b_lo << shift, (b_hi << shift) - 1,
              inf["max_annot"], ptr(longs), len(longs) // 3, C.byref(h))
    return None if rc else DeviceIndex(r1 - r0, 0, _handle=h)


def import_dense(tag, exported, b_lo, b_hi):
    p3, boff3, longs, inf = exported
    d0, d1 = int(boff3[b_lo]), int(boff3[b_hi])
    base = d0 // 5 * 5
    table = np.ascontiguousarray(boff3[b_lo:b_hi + 1])
    shift = inf["bucket_shift"]
    h = C.c_void_p()
    rc = call(f"{tag} import_dense", None, _lib.lib().memo_index_import_dense, d1 - base, 0, shift, b_lo,
              ptr(p3[4 * (base // 5):4 * ((d1 + 4) // 5)]), ptr(table), len(table) + 1, base, b_lo << shift, (b_hi << shift) - 1,
              inf["max_annot"], ptr(longs), len(longs) // 3, C.byref(h))
    return None if rc else DeviceIndex(d1 - base, 0, _handle=h)


def build_up(tag, ix, keep_wide=True, keep_packed=True):
    call(f"{tag} pack", ix, _lib.lib().memo_index_pack, ix._h, int(keep_wide))
    call(f"{tag} pack_dense", ix, _lib.lib().memo_index_pack_dense, ix._h, int(keep_packed))
    taken = C.c_uint64(0)
    call(f"{tag} prepare", ix, _lib.lib().memo_index_prepare, ix._h, 31, N, 0, 0, None, C.byref(taken))
    print(tag, "prepare took", taken.value)


def columns_way():
    lib = _lib.lib()
    for longs in (0, 40):
        A, B = host_rows(synth.SEED, longs), host_rows(SEED_B, longs)
        m = len(A[0])
        tag = f"columns longs={longs}"
        with DeviceIndex(m) as ix:
            show(f"{tag} create", ix)
            call(f"{tag} upload A", ix, lib.memo_index_upload, ix._h, ptr(A[0]), ptr(A[1]), ptr(A[2]), m)
            call(f"{tag} finalize", ix, lib.memo_index_finalize, ix._h, 0, 0)
            queries(f"{tag} wide", ix)
            build_up(tag, ix)
            queries(f"{tag} all levels", ix)
            call(f"{tag} pack again", ix, lib.memo_index_pack, ix._h, 1)
            queries(f"{tag} repacked", ix)
            build_up(tag, ix)
            call(f"{tag} pack_dense again, words go", ix, lib.memo_index_pack_dense, ix._h, 0)
            queries(f"{tag} dense + wide", ix)
            build_up(tag, ix)
            call(f"{tag} upload B", ix, lib.memo_index_upload, ix._h, ptr(B[0]), ptr(B[1]), ptr(B[2]), m)
            call(f"{tag} query unfinalized", ix, lib.memo_query_conservation_dev, ix._h, 0, 16, 31, N, None, None)
            call(f"{tag} finalize", ix, lib.memo_index_finalize, ix._h, 0, 0)
            build_up(tag, ix)
            queries(f"{tag} B", ix)
            cut = slice(m // 3, m // 3 + 100_003)
            call(f"{tag} upload_rows", ix, lib.memo_index_upload_rows, ix._h, cut.start, ptr(A[0][cut]), ptr(A[1][cut]), ptr(A[2][cut]),
                 cut.stop - cut.start)
            call(f"{tag} finalize", ix, lib.memo_index_finalize, ix._h, 0, 0)
            build_up(tag, ix)
            queries(f"{tag} mixed", ix)
            call(f"{tag} truncate", ix, lib.memo_index_truncate, ix._h, m // 2)
            call(f"{tag} finalize", ix, lib.memo_index_finalize, ix._h, 0, 0)
            build_up(tag, ix)
            queries(f"{tag} half", ix)
            s, e, o = C.c_void_p(), C.c_void_p(), C.c_void_p()
            call(f"{tag} columns", ix, lib.memo_index_columns, ix._h, C.byref(s), C.byref(e), C.byref(o))
            call(f"{tag} finalize", ix, lib.memo_index_finalize, ix._h, 0, 0)
            build_up(tag, ix)
            num, den = synth.rows_per_position(N)
            call(f"{tag} synth_fill", ix, lib.memo_synth_fill, ix._h, 0, num, den, N, SEED_B)
            call(f"{tag} finalize", ix, lib.memo_index_finalize, ix._h, 0, 0)
            build_up(tag, ix)
            queries(f"{tag} synthetic", ix)
            call(f"{tag} finalize shift 6", ix, lib.memo_index_finalize, ix._h, 6, 0)
            build_up(tag, ix)
            queries(f"{tag} shift 6", ix)
            call(f"{tag} finalize shift 5", ix, lib.memo_index_finalize, ix._h, 5, 0)
            build_up(tag, ix, keep_wide=False, keep_packed=False)
            queries(f"{tag} dense only", ix)
            call(f"{tag} upload without columns", ix, lib.memo_index_upload, ix._h, ptr(B[0]), ptr(B[1]), ptr(B[2]), m // 2)
            call(f"{tag} finalize without columns", ix, lib.memo_index_finalize, ix._h, 0, 0)
            call(f"{tag} pack without columns", ix, lib.memo_index_pack, ix._h, 0)
    # a refused pack, and the 6-byte format
    s, e, o = host_rows(synth.SEED, 0)
    with DeviceIndex.from_host(s, e, np.where(np.arange(len(o)) == 12345, 70_000, o)) as ix:
        call("wild annot pack", ix, lib.memo_index_pack, ix._h, 1)
        call("wild annot pack again", ix, lib.memo_index_pack, ix._h, 1)
    with DeviceIndex.from_host(s, e, o * 50) as ix:
        call("format 6 pack", ix, lib.memo_index_pack, ix._h, 1)
        call("format 6 pack_dense", ix, lib.memo_index_pack_dense, ix._h, 1)
        queries("format 6", ix, n=5000)
        exported = export_packed("format 6", ix)
        call("format 6 finalize", ix, lib.memo_index_finalize, ix._h, 0, 0)
        lib.memo_index_upload(ix._h, ptr(s), ptr(e), ptr(o), len(s))
        ix.finalize()
        call("format 6 -> 4 pack", ix, lib.memo_index_pack, ix._h, 1)
    nb = len(exported[2])
    for b_lo, b_hi in ((0, nb - 1), (nb // 5, nb // 2)):
        with import_packed(f"format 6 [{b_lo}, {b_hi}]", exported, b_lo, b_hi) as ix:
            show("format 6 imported", ix)
            queries("format 6 imported", ix, n=5000)


def options():
    lib = _lib.lib()
    ix, _ = synth.device_index(0, L, 64, N, L, pack="keep")
    with ix:
        ix.pack_dense(keep_packed=True)
        for option in range(0, 9):
            for value in (-1, 0, 1, 2, 5, 6, 7, 1600, 1601, 100000, 100001):
                ix.prepare(31, N)
                ix.prepare(17, N)
                ix.prepare(31, N, membership=True)
                ix.conservation(-40, L // 2, 31, N)      # (a negative start: the dense rows without a tile table; then with one, of the rows themselves)
                ix.set_option(1, 0)
                ix.conservation(0, L, 31, N)
                ix.set_option(1, 1)
                ix.prepare(31, N)
                call(f"set_option({option}, {value})", ix, lib.memo_index_set_option, ix._h, option, value)
        for option, value in ((1, 1), (2, 200), (3, 100), (4, 0), (5, 1), (6, 1), (7, 1)):
            call(f"set_option({option}, {value})", ix, lib.memo_index_set_option, ix._h, option, value)
        queries("options restored", ix)


def builder_and_cache():
    lib = _lib.lib()
    for longs in (0, 40):
        s, e, o = host_rows(synth.SEED, longs)
        nb = None
        for dense in (False, True):
            tag = f"builder dense={dense} longs={longs}"
            with DeviceIndex.from_host_packed(s, e, o, dense=dense) as ix:
                show(f"{tag} finish", ix)
                queries(tag, ix)
                call(f"{tag} pack", ix, lib.memo_index_pack, ix._h, 0)
                taken = C.c_uint64(0)
                call(f"{tag} prepare", ix, lib.memo_index_prepare, ix._h, 31, N, 0, 0, None, C.byref(taken))
                call(f"{tag} prepare k=101", ix, lib.memo_index_prepare, ix._h, 101, N, 0, 0, None, C.byref(taken))
                queries(f"{tag} prepared", ix)
                call(f"{tag} pack_dense", ix, lib.memo_index_pack_dense, ix._h, 1)
                call(f"{tag} upload", ix, lib.memo_index_upload, ix._h, ptr(s), ptr(e), ptr(o), len(s))
                exported = export_dense(tag, ix) if dense else export_packed(tag, ix)
                exported3 = None if dense else export_dense(tag, ix)
            nb = len(exported[1] if dense else exported[2])
            for b_lo, b_hi in ((0, nb - 1), (nb // 4, nb // 2 + 3)):
                for which, ex in (("dense", exported if dense else exported3), ("packed", None if dense else exported)):
                    if ex is None:
                        continue
                    tag2 = f"{tag} import {which} [{b_lo}, {b_hi}]"
                    made = (import_dense if which == "dense" else import_packed)(tag2, ex, b_lo, b_hi)
                    with made as ix:
                        show(f"{tag2} imported", ix)
                        queries(tag2, ix)
                        call(f"{tag2} pack", ix, lib.memo_index_pack, ix._h, 0)
                        call(f"{tag2} pack_dense keep", ix, lib.memo_index_pack_dense, ix._h, 1)
                        call(f"{tag2} pack_dense drop", ix, lib.memo_index_pack_dense, ix._h, 0)
                        queries(f"{tag2} again", ix)
                        (export_dense if ix.info()["dense_rows"] else export_packed)(tag2, ix)


if __name__ == "__main__":
    print("library", os.path.basename(_lib.SO_PATH), _lib.lib().memo_version().decode())
    columns_way()
    options()
    builder_and_cache()
