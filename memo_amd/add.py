"""`memo add`: a membership index of N genomes grown by m new ones, without the old genomes.

No counterpart in the reference.  `memo index` spends almost all of its time on matching statistics, one suffix array, LCP array and walk
per genome; the membership index still holds the old genomes' (memo_amd/lengths.py reads them back, memo_amd/convert.py feeds them to the
row builder).  So only the new genomes' are computed (memo_amd/build_index.py's MatchingStatistics, memo_ms.hip as it stands), put beside
the columns read back, and the row builder runs once.  Per pivot record R of Lrec positions, with the input's rows of that record:

    old[p][g - 1] = min( Lrec - p, len[g][p] )                                  1 <= g < N       as memo_amd/convert.py defines ms
    new[p][j]     = MS of R at p against genome_text(new genome j)              0 <= j < m       build_index.genome_text
    rows out      = dap_to_bed.py --mem --overlap [--order] of [old | new]                       N - 1 + m columns; new genome j is annot N + j

Without --order the rows are the membership index of the N + m genomes in canonical form (`memo convert -m` writes that form), with
--order the conservation index; both come from the same matrix in the same run.  DESIGN.md 10.8's caveat carries over: a matching
statistic of 0 left no row in the input, so an old column is what the index answers with; where every pivot character occurs in every
old genome the output is the file `memo index` writes on the full list.  The new columns are the true matching statistics, zeros
included.  The index holds no sequence: a pivot FASTA with the right record names and lengths but other bases is not detected.

The records run as memo_amd/convert.py runs them (pass A for the carries, pass B for the planes, slices and batches); per batch
memo_ms_rows_dev hands over the new columns' rows where they lie, add_dap_kernel (memo_amd/csrc/memo_add.hip) writes the matrix from
both sources, and memo_dap_push_dev reads it -- once per requested output.  The result depends neither on the slice nor on the batch
length, nor on the layout, the piece cap or the walk budget of the matching statistics.  One device.  The flags are
memo_amd/add_cli.py.
"""
import contextlib
import ctypes as C
import os
import re

import numpy as np

from ._lib import MemoError, check, lib
from .convert import L_MAX, Builders, check_rows, dap_of, docs, record_length, record_rows, same_file, scan_index, setting

N_MAX = 2048                 # genomes after the addition, the pivot included
HOLD_BYTES = 2 << 30         # new genomes whose FASTA files are larger together are read twice: once to refuse, once to add


def tile():
    """positions per tile of add_dap_kernel: the lengths a test wants to straddle"""
    return int(lib().memo_add_tile())


def _sizes(n_docs, new):
    """(N, m) after the checks both the command and the functions make"""
    n_docs, new = int(n_docs), int(new)
    if not 2 <= n_docs <= N_MAX - 1:
        raise ValueError(f"n_docs must be in [2, {N_MAX - 1}] (got {n_docs})")
    if new < 1:
        raise ValueError("no new genome: needs the pivot and at least one new genome")
    if n_docs + new > N_MAX:
        raise ValueError(f"{n_docs} genomes and {new} new ones are {n_docs + new}: the limit is {N_MAX}")
    return docs(n_docs), new


def _add_genomes(ms, genomes, piece_bytes, label=lambda j: f"new genome {j}"):
    """genomes: an iterable of lists of (name, sequence); each becomes one column of `ms`"""
    for j, records in enumerate(genomes):
        try:
            ms.add_records([s for _, s in records], j, piece_bytes)
        except MemoError as exc:
            found = re.search(r"genome record (\d+) ", str(exc))
            if not found:
                raise
            from .build_index import FastaError
            raise FastaError(f"{label(j)}: record '{records[int(found.group(1))][0]}': {exc}") from None


def _grown_rows(ms, base, feed, length, n_docs, builders, device, slice_positions, batch_positions):
    """record_rows of one record whose first position is `base` in the pivot of `ms`, the new columns beside the old"""
    L_, new = lib(), ms.columns

    def matrix(d_cells, pitch, at, first, positions, remaining, d_dap):
        d_new = C.c_void_p()
        check(L_.memo_ms_rows_dev(ms._h, base + at, positions, C.byref(d_new)))
        check(L_.memo_add_dap_dev(d_cells, pitch, n_docs, first, positions, remaining, d_new, new, d_dap, device, None))
    return record_rows([(feed, n_docs)], length, builders, device, slice_positions, batch_positions, n_docs - 1 + new, matrix)


def rows(start, end, annot, n_docs, record, genomes, *, order=True, device=0, slice_positions=None, batch_positions=None,
         layout="auto", piece_bytes=0, walk_budget=None):
    """One pivot record grown: start, end, annot are the host columns (any order) of its rows in a membership index of n_docs
    genomes, `record` its sequence (bytes; only its length can be checked against the rows), `genomes` the new genomes, each a list
    of record sequences (bytes).  Returns the (start, end, annot) int64 columns of the record's rows in the index of n_docs +
    len(genomes) genomes: the conservation rows (order=True) or the membership rows in canonical form (order=False)."""
    from .build_index import MatchingStatistics, pivot_layout
    from .lengths import host_feed
    genomes = [[("", bytes(s)) for s in g] for g in genomes]
    n_docs, new = _sizes(n_docs, len(genomes))
    cols = [np.ascontiguousarray(c, np.int64) for c in (start, end, annot)]
    if len({len(c) for c in cols}) != 1:
        raise ValueError("start, end and annot differ in length")
    check_rows(*cols, n_docs)
    if not len(cols[0]):
        raise ValueError("the record has no rows in the index")
    L = record_length(cols[0].max())
    _names, pivot, rec_begin = pivot_layout([("record", bytes(record))])
    if L != len(pivot):
        raise ValueError(f"the largest row start is {L}, the record has {len(pivot)} positions")
    slice_positions = setting(slice_positions, "MEMO_ADD_SLICE", "slice_positions")
    batch_positions = setting(batch_positions, "MEMO_ADD_BATCH", "batch_positions")
    out = [[np.empty(0, np.int64)] for _ in range(3)]
    feed, buf = host_feed(*cols, None, device, (0, L + min(L, L_MAX)))
    with buf, MatchingStatistics(pivot, rec_begin, new, device, 0, layout, walk_budget) as ms:
        _add_genomes(ms, genomes, piece_bytes)
        with Builders(n_docs - 1 + new, rec_begin, [order], device) as builders:
            for ((_rec, s, e, a),) in _grown_rows(ms, 0, feed, L, n_docs, builders, device, slice_positions, batch_positions):
                for column, part in zip(out, (s, e, a)):
                    column.append(part.astype(np.int64))
    return tuple(np.concatenate(column) for column in out)


def dap(planes, new, first, positions, remaining, device=0, pitch=None):
    """add_dap_kernel alone on host values: planes uint32 [N, L] (plane 0 is not read) and new int32 [positions, m] -> int32
    [positions, N - 1 + m]: min(planes[g][first + i], remaining - i) beside min(uint32(new[i][j]), remaining - i).  pitch: the planes'
    pitch on the device (default: L rounded up to 4)."""
    planes = np.asarray(planes, np.uint32)
    positions = max(int(positions), 0)
    new = np.ascontiguousarray(new, np.int32)
    if planes.ndim != 2 or new.ndim != 2:
        raise ValueError("planes must be [n_docs, positions], new [positions, new genomes]")
    if new.shape[0] != positions:
        raise ValueError(f"new has {new.shape[0]} rows for {positions} positions")
    n_docs, m = _sizes(planes.shape[0], new.shape[1])

    def call(d_cells, pitch, d_new, first, positions, remaining, d_out):
        return lib().memo_add_dap_dev(d_cells, pitch, n_docs, first, positions, remaining, d_new, m, d_out, device, None)
    return dap_of(call, n_docs - 1 + m, planes, first, positions, remaining, device, pitch, new)


def _match_pivot(in_path, n_docs, pivot_path):
    """(names, pivot bytes, rec_begin) of the pivot FASTA after it has been held against the index: every record of the index is a
    pivot record, every pivot record has rows, and every record's largest row start is its length.  Host only."""
    from .build_index import FastaError, pivot_layout, read_fasta
    names, pivot, rec_begin = pivot_layout(read_fasta(pivot_path), pivot_path)
    if len(set(names)) != len(names):
        twice = next(n for i, n in enumerate(names) if n in names[:i])
        raise FastaError(f"{pivot_path}: record name '{twice}' occurs twice")
    found = dict(zip(*scan_index(in_path, n_docs)))
    for name in found:
        if name not in names:
            raise ValueError(f"record {name!r} of {in_path} is not a record of the pivot {pivot_path}: is this the pivot the index was built on?")
    for name, length in zip(names, np.diff(rec_begin).tolist()):
        if name not in found:
            raise ValueError(f"pivot record {name!r} of {pivot_path} has no rows in {in_path}: is this the pivot the index was built on?")
        if found[name] != length:
            raise ValueError(f"record {name!r}: the largest row start in {in_path} is {found[name]}, the record in {pivot_path} has "
                             f"{length} positions: is this the pivot the index was built on?")
    return names, pivot, rec_begin


def add_index(in_path, genome_list, n_docs, out_path=None, cons_path=None, device=0, log=print, piece_bytes=0, layout="auto",
              walk_budget=None):
    """in_path, a Parquet membership index of n_docs genomes, grown by the genomes of genome_list (`memo index`'s list format: the
    first line is the pivot FASTA the index was built on, the others are the new genomes, annot n_docs ... in list order): the
    membership index in canonical form at out_path and/or the conservation index at cons_path, with the schema, codec and row-group
    statistics `memo index` writes.  piece_bytes, layout and walk_budget are build_index.MatchingStatistics'.  Everything that is
    refused is refused before the device is touched and before anything is written; each file is written beside its name and renamed.
    Returns {"positions", "new", "rows": [per output, -o first]}."""
    from .build_index import MatchingStatistics, _layout_number, read_fasta, read_genome_list
    from .dap_to_bed import RowWriter
    from ._cli import replace_all_into
    from .lengths import region_feed
    outputs = [(path, order) for path, order in ((out_path, False), (cons_path, True)) if path]
    if not outputs:
        raise ValueError("no output: give the membership index's path, the conservation index's, or both")
    paths = read_genome_list(genome_list)
    n_docs, new = _sizes(n_docs, len(paths) - 1)
    _layout_number(layout)
    for path, _ in outputs:
        if same_file(in_path, path):
            raise ValueError(f"{path} is the input file")
    if len(outputs) == 2 and same_file(outputs[0][0], outputs[1][0]):
        raise ValueError(f"{outputs[0][0]} is named for both outputs")
    slice_positions = setting(None, "MEMO_ADD_SLICE", "MEMO_ADD_SLICE")
    batch_positions = setting(None, "MEMO_ADD_BATCH", "MEMO_ADD_BATCH")
    names, pivot, rec_begin = _match_pivot(in_path, n_docs, paths[0])
    hold = sum(os.path.getsize(p) for p in paths[1:]) <= HOLD_BYTES
    held = []
    for path in paths[1:]:                                             # what read_fasta refuses is refused here, before the device
        records = read_fasta(path)
        held.append(records if hold else None)

    def genomes():
        for j, path in enumerate(paths[1:]):
            log(f"Finding MS between pivot and {os.path.basename(path)}")
            yield held[j] if hold else read_fasta(path)
            held[j] = None

    def write(tmps):
        with contextlib.ExitStack() as stack:
            ms = stack.enter_context(MatchingStatistics(pivot, rec_begin, new, device, 0, layout, walk_budget))
            _add_genomes(ms, genomes(), piece_bytes, lambda j: paths[1 + j])
            writers = [stack.enter_context(RowWriter(tmp)) for tmp in tmps]
            builders = stack.enter_context(Builders(n_docs - 1 + new, rec_begin, [order for _, order in outputs], device))
            for r, name in enumerate(names):                           # in FASTA order
                feed, buf = region_feed(in_path, name, device)
                with buf:
                    for parts in _grown_rows(ms, int(rec_begin[r]), feed, int(rec_begin[r + 1] - rec_begin[r]), n_docs, builders, device,
                                             slice_positions, batch_positions):
                        for writer, part in zip(writers, parts):
                            writer.write(names, part)
                log(f"{name}: {int(rec_begin[r + 1] - rec_begin[r])} positions")
        return [w.rows for w in writers]

    written = []
    replace_all_into([path for path, _ in outputs], lambda tmps: written.extend(write(tmps)))
    return {"positions": int(rec_begin[-1]), "new": new, "rows": written}
