"""`memo convert`: a conservation index (or the membership index in canonical form) from a membership index, without the genomes.

No counterpart in the reference.  A membership index holds, per non-pivot genome, the rows that bound how far the genome matches the
pivot from every position; `memo lengths` reads those lengths back, and they are the matching statistics the index was built from --
as far as the index says (a statistic of 0 leaves no row in the reference's membership index).  Per record of the
input, with its rows (s, e, a), N genomes and Lrec = max s (or the record's length in a .fai):

    ms[p][g - 1] = min( Lrec - p, len[g][p] )            0 <= p < Lrec, 1 <= g < N       len: memo_amd/lengths.py with qs = 0, qe = Lrec,
                                                                                        cap = min(Lrec, 2^31 - 1)
    rows out     = dap_to_bed.py --mem --overlap [--order] of ms                        (memo_amd/dap_to_bed.py, memo_dap.hip)

The lengths take their slices from the right (a slice needs, per genome, the smallest end right of it), the row builder takes positions
from the left (it needs the previous MEM of every column), and a record's planes do not fit on the device in general.  So a record of
more than one slice runs in two passes over its rows:
    pass A, right to left, carries only: before a slice's rows enter the carry (memo_lengths_carry_dev) the carry is saved as that
            slice's own: N int64 a slice, on the host
    pass B, left to right: begin with the slice's saved carry, rows, finish (memo_lengths_*_dev), then in batches of positions
            convert_dap_kernel (memo_amd/csrc/memo_convert.hip: genome-major planes to the position-major matrix, clipped at the
            record's end), memo_dap_push_dev and memo_dap_fetch
One memo_dap_t serves a whole file: the records follow one another without a gap, and a slice never straddles a record.  The result
depends neither on the slice nor on the batch length.  One device.  The flags are memo_amd/convert_cli.py.
"""
import contextlib
import ctypes as C
import os

import numpy as np

from ._lib import check, lib

N_MAX = 2048
L_MAX = 2 ** 31 - 1
BUILDER_L_MAX = 2 ** 30 - 1            # memo_dap_create takes records of 1 .. 2^30 - 1 positions
BATCH_BYTES = 128 << 20                # a push batch's matrix; the row builder holds three times that besides
_NO_CARRY = np.iinfo(np.int64).max


def tile():
    """positions per tile of convert_dap_kernel: the lengths a test wants to straddle"""
    return int(lib().memo_convert_tile())


def docs(n_docs):
    """n_docs as an integer of [2, N_MAX]"""
    n_docs = int(n_docs)
    if not 2 <= n_docs <= N_MAX:
        raise ValueError(f"n_docs must be in [2, {N_MAX}] (got {n_docs})")
    return n_docs


def default_batch_positions(n_docs):
    """the positions per push whose matrix, 4 (N - 1) batch bytes, is about 128 MiB"""
    return max(BATCH_BYTES // (4 * (int(n_docs) - 1)), 1)


def setting(value, env, what):
    """a slice or batch length: the argument, else the environment's (the tests force small ones; the result depends on neither), else None"""
    if value is None and os.environ.get(env):
        value = os.environ[env]
    if value is None:
        return None
    try:
        value = int(value)
    except ValueError:
        value = 0
    if not 1 <= value <= 2 ** 31:
        raise ValueError(f"{what} must be an integer in [1, 2^31]")
    return value


def check_rows(start, end, annot, n_docs, record="", offset=0):
    """What the promise does not cover is refused: the first row with end < start, the first annot outside [1, N - 1].  `offset`: the
    number of the columns' first row in its file."""
    where = f" of {record}" if record else ""
    bad = np.flatnonzero(end < start)
    if len(bad):
        i = int(bad[0])
        raise ValueError(f"row {offset + i}{where} ends before it starts ({int(start[i])}, {int(end[i])}, {int(annot[i])}): such an index answers "
                         "no query as a membership index does, and is not converted")
    bad = np.flatnonzero((annot < 1) | (annot > n_docs - 1))
    if len(bad):
        i = int(bad[0])
        raise ValueError(f"row {offset + i}{where} has annot {int(annot[i])} outside [1, {n_docs - 1}] ({int(start[i])}, {int(end[i])}, {int(annot[i])}): "
                         "the -n value is probably wrong")


def record_length(max_start, length=None, record=""):
    """Lrec: the largest start (an index that `memo index` wrote ends every record with rows at start = record length), or `length`"""
    where = f" of {record}" if record else ""
    L = int(max_start) if length is None else int(length)
    if L < int(max_start):
        raise ValueError(f"the length {L}{where} is below its largest row start {int(max_start)}")
    if L > L_MAX:
        raise ValueError(f"the length {L}{where} is above 2^31 - 1")
    if L > BUILDER_L_MAX:
        raise ValueError(f"the length {L}{where} is above 2^30 - 1, the longest record the row builder takes")
    return L


def slice_carries(start, end, annot, length, n_docs, step):
    """Pass A's bookkeeping on the host, for the tests: {(a, b): int64 [N]} -- for every slice [a, b) of [0, length) cut at multiples
    of `step`, the smallest end per genome among the rows with b < start (INT64_MAX: none), found from the right as the device finds
    it: the carry is saved, then the slice's rows a < start < b + 1 enter it."""
    from .lengths import window_slices
    start, end, annot = (np.asarray(c, np.int64) for c in (start, end, annot))
    known = (annot >= 0) & (annot < n_docs)
    carry = np.full(n_docs, _NO_CARRY, np.int64)

    def enter(lo, hi):
        take = known & (start > lo) & (start < hi)
        np.minimum.at(carry, annot[take], end[take])
    enter(length, length + min(length, L_MAX))
    out = {}
    for a, b in window_slices(0, length, n_docs, step):
        out[(a, b)] = carry.copy()
        enter(a, b + 1)
    return out


class _RowBuilder:
    """one memo_dap_t (--mem --overlap [--order]) that takes its matrix where it lies in device memory"""

    def __init__(self, columns, rec_begin, order, device):
        from .dap_to_bed import DapConverter
        self._conv = DapConverter(columns, rec_begin, order, True, device)

    def push_dev(self, d_dap, positions):
        n = C.c_uint64()
        check(lib().memo_dap_push_dev(self._conv._h, d_dap, positions, C.byref(n)))
        out = self._conv._bufs(n.value)
        if n.value:
            check(lib().memo_dap_fetch(self._conv._h, *[a.ctypes.data for a in out]))
        return out

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self._conv.close()


class Builders:
    """one row builder per requested output, all fed the same matrix"""

    def __init__(self, columns, rec_begin, orders, device):
        self._stack = contextlib.ExitStack()
        try:
            self._each = [self._stack.enter_context(_RowBuilder(columns, rec_begin, order, device)) for order in orders]
        except BaseException:
            self._stack.close()
            raise

    def push_dev(self, d_dap, positions):
        return [b.push_dev(d_dap, positions) for b in self._each]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self._stack.close()


def same_file(a, b):
    """whether two paths name one file, existing or not"""
    if os.path.exists(a) and os.path.exists(b):
        return os.path.samefile(a, b)
    return os.path.abspath(a) == os.path.abspath(b)


def record_rows(sources, length, builder, device, slice_positions, batch_positions, columns, matrix):
    """Yields what builder.push_dev(d_dap, positions) returns for one record of `length` positions, batch by batch, in the index's
    order.  sources = [(feed, n_docs), ...]: feed(lo, hi) yields (d_start, d_end, d_annot, rows) chunks of device columns that hold at
    least that source's rows with lo < start < hi.  The sources' planes lie stacked in one buffer with one pitch, source s in planes
    [base_s, base_s + N_s), each with its own carries; the slices are cut for the sum of the N_s.
    The step that makes a batch's matrix is the caller's: `columns`, the matrix's width, and matrix(d_cells, pitch, at, first,
    positions, remaining, d_dap), which writes int32 [positions][columns] at d_dap from positions [first, first + positions) of the
    slice's stack; `at` is the batch's first position in the record."""
    from ._device import DevBuffer
    from .lengths import pitch_of, window_slices
    L_ = lib()
    sizes = [n for _, n in sources]
    total = sum(sizes)
    bases = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    cap = min(length, L_MAX)
    reach = length + cap
    slices = window_slices(0, length, total, slice_positions)               # from the right; cut for the whole stack
    batch = default_batch_positions(columns + 1) if batch_positions is None else batch_positions
    longest = max(b - a for a, b in slices)
    with DevBuffer(device, 4 * total * pitch_of(longest)) as cells, DevBuffer(device, 8 * total if len(slices) > 1 else 0) as carry, \
            DevBuffer(device, 4 * columns * min(batch, longest)) as d_dap:
        saved = {}
        if len(slices) > 1:                                            # pass A: every slice's carry, from the right, source by source
            for s, (feed, n) in enumerate(sources):
                d_carry = carry.at(8 * bases[s])
                none = np.full(n, _NO_CARRY, np.int64)
                check(L_.memo_dev_upload(device, d_carry, none.ctypes.data, none.nbytes, None))
                for chunk in feed(length, reach):                      # (the rows right of the record: none in an index `memo index` wrote)
                    check(L_.memo_lengths_carry_dev(*chunk, length, reach, n, d_carry, device, None))
                for a, b in slices:
                    saved[s, a] = np.empty(n, np.int64)
                    check(L_.memo_dev_download(device, saved[s, a].ctypes.data, d_carry, saved[s, a].nbytes, None))
                    if a:                                              # (nothing lies left of the first slice)
                        for chunk in feed(a, b + 1):
                            check(L_.memo_lengths_carry_dev(*chunk, a, b + 1, n, d_carry, device, None))
        for a, b in slices[::-1]:                                      # pass B: the planes, left to right
            Ls, pitch = b - a, pitch_of(b - a)
            for s, (feed, n) in enumerate(sources):
                block = cells.at(4 * bases[s] * pitch)                 # (pitch % 4 == 0: every block is 16-byte aligned)
                if len(slices) > 1:
                    d_carry = carry.at(8 * bases[s])
                    check(L_.memo_dev_upload(device, d_carry, saved[s, a].ctypes.data, saved[s, a].nbytes, None))
                    check(L_.memo_lengths_begin_dev(block, Ls, pitch, n, cap, a, d_carry, device, None))
                    chunks = feed(a, b + 1)
                else:                                                  # the whole record: the row pass's own filter is the definition's
                    check(L_.memo_lengths_begin_dev(block, Ls, pitch, n, cap, a, None, device, None))
                    chunks = feed(0, reach)
                for chunk in chunks:
                    check(L_.memo_lengths_rows_dev(*chunk, a, Ls, pitch, n, cap, block, device, None))
                check(L_.memo_lengths_finish_dev(block, Ls, pitch, n, cap, device, None))
            for first in range(0, Ls, batch):
                positions = min(batch, Ls - first)
                matrix(cells.d, pitch, a + first, first, positions, length - a - first, d_dap.d)
                yield builder.push_dev(d_dap.d, positions)


def _converted_rows(feed, length, n_docs, builder, device, slice_positions, batch_positions):
    """record_rows of one source, its N - 1 columns as they lie (convert_dap_kernel)"""
    def matrix(d_cells, pitch, at, first, positions, remaining, d_dap):
        check(lib().memo_convert_dap_dev(d_cells, pitch, n_docs, first, positions, remaining, d_dap, device, None))
    return record_rows([(feed, n_docs)], length, builder, device, slice_positions, batch_positions, n_docs - 1, matrix)


def dap_of(call, width, planes, first, positions, remaining, device, pitch, side=None):
    """One planes-to-matrix kernel alone on host values: the uint32 planes [P, L], padded to `pitch` (default: L rounded up to 4), and
    the kernel's other host array `side` (or None) go up, call(d_cells, pitch, d_side, first, positions, remaining, d_out) runs, and
    int32 [positions, width] comes back."""
    from ._device import DevBuffer
    count, L = planes.shape
    pitch = (L + 3) & ~3 if pitch is None else int(pitch)
    if pitch < L:
        raise ValueError("pitch is below the planes' length")
    padded = np.zeros((count, pitch), np.uint32)
    padded[:, :L] = planes
    positions = int(positions)
    out = np.empty((max(positions, 0), width), np.int32)
    with DevBuffer(device, max(padded.nbytes, 16)) as cells, DevBuffer(device, 0 if side is None else max(side.nbytes, 16)) as d_side, \
            DevBuffer(device, max(out.nbytes, 16)) as d_out:
        for d, host in ((cells, padded), (d_side, side)):
            if host is not None and host.nbytes:
                check(lib().memo_dev_upload(device, d.d, host.ctypes.data, host.nbytes, None))
        check(call(cells.d, pitch, d_side.d, int(first), positions, int(remaining), d_out.d))
        if out.nbytes:
            check(lib().memo_dev_download(device, out.ctypes.data, d_out.d, out.nbytes, None))
    return out


def rows(start, end, annot, n_docs, *, length=None, order=True, device=0, slice_positions=None, batch_positions=None):
    """One record's host columns (any order), converted: the (start, end, annot) int64 columns of its conservation rows (order=True) or
    of its membership rows in canonical form (order=False).  length: the record's length where it is not the largest start.  The result
    depends neither on slice_positions nor on batch_positions."""
    n_docs = docs(n_docs)
    cols = [np.ascontiguousarray(c, np.int64) for c in (start, end, annot)]
    if len({len(c) for c in cols}) != 1:
        raise ValueError("start, end and annot differ in length")
    check_rows(*cols, n_docs)
    L = record_length(cols[0].max() if len(cols[0]) else 0, length)
    slice_positions = setting(slice_positions, "MEMO_CONVERT_SLICE", "slice_positions")
    batch_positions = setting(batch_positions, "MEMO_CONVERT_BATCH", "batch_positions")
    out = [[np.empty(0, np.int64)] for _ in range(3)]
    if L:
        from .lengths import host_feed
        feed, buf = host_feed(*cols, None, device, (0, L + min(L, L_MAX)))
        with buf, _RowBuilder(n_docs - 1, [0, L], order, device) as builder:
            for _rec, s, e, a in _converted_rows(feed, L, n_docs, builder, device, slice_positions, batch_positions):
                for column, part in zip(out, (s, e, a)):
                    column.append(part.astype(np.int64))
    return tuple(np.concatenate(column) for column in out)


def dap(planes, first, positions, remaining, device=0, pitch=None):
    """convert_dap_kernel alone on host values: planes uint32 [N, L] (plane 0 is not read) -> int32 [positions, N - 1],
    min(planes[g][first + i], remaining - i).  pitch: the planes' pitch on the device (default: L rounded up to 4)."""
    planes = np.asarray(planes, np.uint32)
    if planes.ndim != 2:
        raise ValueError("planes must be [n_docs, positions]")
    n_docs = docs(planes.shape[0])

    def call(d_cells, pitch, _d_side, first, positions, remaining, d_out):
        return lib().memo_convert_dap_dev(d_cells, pitch, n_docs, first, positions, remaining, d_out, device, None)
    return dap_of(call, n_docs - 1, planes, first, positions, remaining, device, pitch)


def scan_index(in_path, n_docs, fai=None):
    """The records of a Parquet index in order of first appearance with their lengths, after every row has passed check_rows:
    ([name, ...], [Lrec, ...]).  Host only."""
    import pyarrow.parquet as pq
    n_docs = docs(n_docs)
    lengths = None
    if fai is not None:
        from .dap_to_bed import parse_fai
        names, begin = parse_fai(fai)
        lengths = dict(zip(names, np.diff(begin).tolist()))
    pf = pq.ParquetFile(in_path)
    most, at = {}, 0
    for g in range(pf.metadata.num_row_groups):
        t = pf.read_row_group(g, columns=["f0", "f1", "f2", "f3"])
        s, e, a = (np.ascontiguousarray(t.column(c).to_numpy(), np.int64) for c in ("f1", "f2", "f3"))
        check_rows(s, e, a, n_docs, offset=at)
        at += len(s)
        f0 = t.column("f0").combine_chunks().dictionary_encode()
        codes = np.asarray(f0.indices.to_numpy(zero_copy_only=False), np.int64)
        seen = np.unique(codes, return_index=True)
        for code in seen[0][np.argsort(seen[1])]:                      # in order of first appearance
            name = f0.dictionary[int(code)].as_py()
            most[name] = max(most.get(name, 0), int(s[codes == code].max()))
    out = []
    for name, top in most.items():
        if lengths is not None and name not in lengths:
            raise ValueError(f"record {name!r} of {in_path} is not in {fai}")
        out.append(record_length(top, None if lengths is None else lengths[name], repr(name)))
    return list(most), out


def convert_index(in_path, out_path, n_docs, order=True, fai=None, device=0, log=print):
    """in_path, a Parquet membership index of n_docs genomes, as the conservation index of the same pangenome (order=False: as the
    membership index in canonical form) at out_path: the schema, codec and row-group statistics `memo index` writes.  fai: the pivot's
    .fai, for records longer than their largest row start.  Everything that is refused is refused before out_path is touched; the file
    is written beside its name and renamed.  Returns the number of rows written."""
    from . import dap_to_bed
    from ._cli import replace_into
    from .lengths import region_feed
    n_docs = docs(n_docs)
    if os.path.exists(out_path) and os.path.samefile(in_path, out_path):
        raise ValueError(f"{out_path} is the input file")
    slice_positions = setting(None, "MEMO_CONVERT_SLICE", "MEMO_CONVERT_SLICE")
    batch_positions = setting(None, "MEMO_CONVERT_BATCH", "MEMO_CONVERT_BATCH")
    names, lengths = scan_index(in_path, n_docs, fai)
    kept = [(name, L) for name, L in zip(names, lengths) if L]          # (a record whose rows all start at 0 has no position)
    names = [name for name, _ in kept]

    def batches(builder):
        for name, L in kept:
            feed, buf = region_feed(in_path, name, device)
            with buf:
                for part in _converted_rows(feed, L, n_docs, builder, device, slice_positions, batch_positions):
                    yield names, part
            log(f"{name}: {L} positions")

    def write(tmp):
        if not kept:
            return dap_to_bed.write_parquet(tmp, ())
        rec_begin = np.concatenate([[0], np.cumsum([L for _, L in kept])]).astype(np.int64)
        with _RowBuilder(n_docs - 1, rec_begin, order, device) as builder:
            return dap_to_bed.write_parquet(tmp, batches(builder))
    written = []
    replace_into(out_path, lambda tmp: written.append(write(tmp)))
    return written[0]
