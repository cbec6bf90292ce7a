"""`memo merge`: the index of chosen genomes, in a chosen order, from one or more membership indexes on one pivot, without the genomes.

No counterpart in the reference.  A membership index holds every genome's matching statistics (memo_amd/lengths.py reads them back,
memo_amd/convert.py feeds them to the row builder, memo_amd/add.py puts new columns beside them).  Choosing among them -- a sub-cohort,
another order, the cohorts of two indexes together -- is the same run with a column map.  Per pivot record R of Lrec positions, with the
rows of that record in input s (N_s genomes) and the chosen (s, g) in output order:

    ms_s[p][g - 1] = min( Lrec - p, len_s[g][p] )                                1 <= g < N_s        as memo_amd/convert.py defines ms
    M[p][c]        = ms_s[p][g - 1]   for the c-th chosen (s, g)                 W columns; that genome is annot c + 1 of the output
    rows out       = dap_to_bed.py --mem --overlap [--order] of M

Without --order the rows are the membership index of the chosen genomes in canonical form (`memo convert -m` writes that form): the
canonical rows of the chosen genomes, renumbered.  With --order they are the conservation index, which no edit of the inputs'
conservation rows gives: it sorts every position's columns together.  Both come from the same matrix in the same run.  DESIGN.md 10.8's
caveat carries over: a matching statistic of 0 left no row in its input, so a column is what its index answers with.  The indexes hold no
sequence: two pivots with equal record names and lengths cannot be told apart.

The planes of all inputs lie stacked in one device buffer with one pitch, input s in planes [base_s, base_s + N_s); the slices are cut
for the sum of the N_s, so the stack keeps within the budget of memo_amd/lengths.py.  Every input runs memo_amd/convert.py's passes on
its own block, with its own feed and carries (pass A for the carries from the right, pass B for the planes from the left); per batch
merge_dap_kernel (memo_amd/csrc/memo_merge.hip) writes the matrix through the column map and memo_dap_push_dev reads it -- once per
requested output.  The result depends neither on the slice nor on the batch length.  One device.  The flags are memo_amd/merge_cli.py.
"""
import contextlib

import numpy as np

from ._lib import check, lib
from .convert import L_MAX, Builders, check_rows, dap_of, docs, record_length, record_rows, same_file, scan_index, setting

N_MAX = 2048                 # genomes of one input, and of the output, the pivot included
PLANES_MAX = 65536           # genomes of all inputs together, their pivots included


def tile():
    """positions per tile of merge_dap_kernel: the lengths a test wants to straddle"""
    return int(lib().memo_merge_tile())


def parse_selection(text, n_docs):
    """`-s`: annots and ranges of annots, comma-separated ("1-3,7,5"), in the order written; 1 .. n_docs - 1 are legal, none twice.
    None: all of them, ascending.  A list of integers passes the same checks."""
    if text is None:
        return list(range(1, n_docs))
    out = []
    if isinstance(text, str):
        for part in text.split(","):
            ends = part.split("-")
            if len(ends) > 2 or not all(e.isascii() and e.isdigit() for e in ends):
                raise ValueError(f"the selection {text!r} does not parse at {part!r}: write annots and ranges, as in 1-3,7,5")
            lo, hi = int(ends[0]), int(ends[-1])
            if hi < lo:
                raise ValueError(f"the selection {text!r} does not parse at {part!r}: a range runs upwards (write {lo},{lo - 1} ... for the other order)")
            if hi - lo >= N_MAX:
                raise ValueError(f"the selection {text!r} names annot {hi}, outside [1, {n_docs - 1}]")
            out.extend(range(lo, hi + 1))
    else:
        out = [int(g) for g in text]
    seen = set()
    for g in out:
        if not 1 <= g <= n_docs - 1:
            raise ValueError(f"the selection {_written(text)} names annot {g}, outside [1, {n_docs - 1}]")
        if g in seen:
            raise ValueError(f"the selection {_written(text)} names annot {g} twice")
        seen.add(g)
    return out


def _written(selection):
    return repr(selection) if isinstance(selection, str) else repr(",".join(str(int(g)) for g in selection))


def _plan(sizes, selections):
    """([N_s], [chosen annots of s], plane_of int32 [W]) after the checks both the command and the functions make"""
    if not sizes:
        raise ValueError("no input")
    sizes = [docs(n) for n in sizes]
    if sum(sizes) > PLANES_MAX:
        raise ValueError(f"the inputs hold {sum(sizes)} genomes together: the limit is {PLANES_MAX}")
    chosen = [parse_selection(sel, n) for sel, n in zip(selections, sizes)]
    width = sum(len(c) for c in chosen)
    if not width:
        raise ValueError("no genome is chosen")
    if width > N_MAX - 1:
        raise ValueError(f"{width} genomes are chosen: the limit is {N_MAX - 1}")
    bases = np.concatenate([[0], np.cumsum(sizes)])
    plane_of = np.asarray([bases[s] + g for s, picks in enumerate(chosen) for g in picks], np.int32)
    return sizes, chosen, plane_of


@contextlib.contextmanager
def _mapped(sizes, plane_of, device):
    """The column map on the device for a run: yields (columns, matrix), record_rows' batch step through merge_dap_kernel.  sizes: the
    N_s of the sources whose planes make the stack; plane_of names the plane of every output column in it."""
    from ._device import DevBuffer
    L_ = lib()
    total, width = int(sum(sizes)), len(plane_of)
    plane_of = np.ascontiguousarray(plane_of, np.int32)
    with DevBuffer(device, 4 * width) as d_map:
        check(L_.memo_dev_upload(device, d_map.d, plane_of.ctypes.data, plane_of.nbytes, None))

        def matrix(d_cells, pitch, at, first, positions, remaining, d_dap):
            check(L_.memo_merge_dap_dev(d_cells, pitch, total, d_map.d, width, first, positions, remaining, d_dap, device, None))
        yield width, matrix


def rows(sources, length=None, *, order=True, device=0, slice_positions=None, batch_positions=None):
    """One pivot record merged: sources = [(start, end, annot, n_docs, selection), ...], the host columns (any order) of the record's
    rows in every input, that input's number of genomes and its chosen annots (a list, a `-s` string, or None: all).  length: the
    record's length (default: the largest row start, which must then be the same in every input).  Returns the (start, end, annot)
    int64 columns of the record's rows in the index of the chosen genomes: the conservation rows (order=True) or the membership rows
    in canonical form (order=False).  The result depends neither on slice_positions nor on batch_positions."""
    from .lengths import host_feed
    sources = list(sources)
    sizes, _chosen, plane_of = _plan([src[3] for src in sources], [src[4] for src in sources])
    columns, lengths = [], []
    for s, src in enumerate(sources):
        cols = [np.ascontiguousarray(c, np.int64) for c in src[:3]]
        if len({len(c) for c in cols}) != 1:
            raise ValueError(f"input {s}: start, end and annot differ in length")
        check_rows(*cols, sizes[s], record=f"input {s}")
        columns.append(cols)
        lengths.append(record_length(cols[0].max() if len(cols[0]) else 0, length, f"input {s}"))
    if len(set(lengths)) != 1:
        raise ValueError(f"the record's largest row starts differ between the inputs ({', '.join(map(str, lengths))}): is this the same pivot?")
    L = lengths[0]
    slice_positions = setting(slice_positions, "MEMO_MERGE_SLICE", "slice_positions")
    batch_positions = setting(batch_positions, "MEMO_MERGE_BATCH", "batch_positions")
    out = [[np.empty(0, np.int64)] for _ in range(3)]
    if L:
        with contextlib.ExitStack() as stack:
            feeds = []
            for cols in columns:
                feed, buf = host_feed(*cols, None, device, (0, L + min(L, L_MAX)))
                stack.enter_context(buf)
                feeds.append(feed)
            builders = stack.enter_context(Builders(len(plane_of), [0, L], [order], device))
            mapped = stack.enter_context(_mapped(sizes, plane_of, device))
            for ((_rec, s, e, a),) in record_rows(list(zip(feeds, sizes)), L, builders, device, slice_positions, batch_positions, *mapped):
                for column, part in zip(out, (s, e, a)):
                    column.append(part.astype(np.int64))
    return tuple(np.concatenate(column) for column in out)


def dap(planes, plane_of, first, positions, remaining, device=0, pitch=None):
    """merge_dap_kernel alone on host values: planes uint32 [P, L] and plane_of, the plane of every column (an entry outside [0, P)
    gives a column of zeros) -> int32 [positions, len(plane_of)]: min(planes[plane_of[c]][first + i], remaining - i).  pitch: the
    planes' pitch on the device (default: L rounded up to 4)."""
    planes = np.asarray(planes, np.uint32)
    if planes.ndim != 2:
        raise ValueError("planes must be [planes, positions]")
    count = planes.shape[0]
    if not 1 <= count <= PLANES_MAX:
        raise ValueError(f"the planes must be 1 to {PLANES_MAX} (got {count})")
    plane_of = np.asarray(plane_of)
    if plane_of.ndim != 1 or not 1 <= len(plane_of) <= N_MAX - 1:
        raise ValueError(f"plane_of must name 1 to {N_MAX - 1} columns")
    if len(plane_of) and (plane_of.min() < -2 ** 31 or plane_of.max() > 2 ** 31 - 1):
        raise ValueError("plane_of must hold int32 values")
    plane_of = np.ascontiguousarray(plane_of, np.int32)

    def call(d_cells, pitch, d_map, first, positions, remaining, d_out):
        return lib().memo_merge_dap_dev(d_cells, pitch, count, d_map, len(plane_of), first, positions, remaining, d_out, device, None)
    return dap_of(call, len(plane_of), planes, first, max(int(positions), 0), remaining, device, pitch, plane_of)


def read_list(path, n_docs):
    """the lines of a genome list as memo_amd/_cli.py reads them (stripped, the empty ones dropped); there must be n_docs"""
    try:
        with open(path) as fh:
            lines = [ln.strip() for ln in fh if ln.strip()]
    except OSError as exc:
        raise ValueError(f"cannot read the genome list {path}: {exc.strerror}") from None
    if len(lines) != n_docs:
        raise ValueError(f"-g {path} names {len(lines)} genomes, -n says {n_docs}")
    return lines


def merged_list(lists, chosen):
    """the output's genome list: the first input's pivot line, then the line of every chosen genome in output order"""
    return [lists[0][0]] + [lists[s][g] for s, picks in enumerate(chosen) for g in picks]


def merge_index(inputs, out_path=None, cons_path=None, list_out=None, fai=None, device=0, log=print):
    """inputs = [(path, n_docs, selection, genome list), ...]: Parquet membership indexes on ONE pivot, each with its number of genomes,
    its chosen annots (a `-s` string, a list, or None: all, ascending) and its genome list (`memo index`'s format; None: none).  The
    output's genomes are annot 1, 2 ... in the order of the inputs and, within an input, of its selection; genome 0 is the pivot.
    Written: the membership index in canonical form at out_path and/or the conservation index at cons_path, with the schema, codec and
    row-group statistics `memo index` writes, and at list_out the output's genome list (needs every input's).  fai: the pivot's .fai,
    for records longer than their largest row start.  Everything that is refused is refused before the device is touched and before
    anything is written; each file is written beside its name and renamed.
    Returns {"positions", "genomes", "rows": [per output, -o first]}."""
    from .dap_to_bed import RowWriter
    from ._cli import replace_all_into
    from .lengths import region_feed
    inputs = [tuple(i) + (None,) * (4 - len(i)) for i in inputs]
    outputs = [(path, order) for path, order in ((out_path, False), (cons_path, True)) if path]
    if not outputs:
        raise ValueError("no output: give the membership index's path, the conservation index's, or both")
    sizes, chosen, plane_of = _plan([i[1] for i in inputs], [i[2] for i in inputs])
    paths = [i[0] for i in inputs]
    for at, path in enumerate(paths):
        if any(same_file(path, other) for other in paths[:at]):
            raise ValueError(f"{path} is given as two inputs")
    written_paths = [path for path, _ in outputs] + ([list_out] if list_out else [])
    for path in written_paths:
        if any(same_file(path, other) for other in paths) or any(i[3] and same_file(path, i[3]) for i in inputs):
            raise ValueError(f"{path} is an input file")
    for at, path in enumerate(written_paths):
        if any(same_file(path, other) for other in written_paths[:at]):
            raise ValueError(f"{path} is named for two outputs")
    if list_out and not all(i[3] for i in inputs):
        raise ValueError("-G needs the genome list (-g) of every input")
    slice_positions = setting(None, "MEMO_MERGE_SLICE", "MEMO_MERGE_SLICE")
    batch_positions = setting(None, "MEMO_MERGE_BATCH", "MEMO_MERGE_BATCH")
    lists = [read_list(i[3], n) if i[3] else None for i, n in zip(inputs, sizes)]
    found = [scan_index(path, n, fai) for path, n in zip(paths, sizes)]
    names, lengths = found[0]
    for path, (other_names, other_lengths) in zip(paths[1:], found[1:]):
        for name in names:
            if name not in other_names:
                raise ValueError(f"record {name!r} of {paths[0]} has no rows in {path}: is this the same pivot?")
        for name in other_names:
            if name not in names:
                raise ValueError(f"record {name!r} of {path} has no rows in {paths[0]}: is this the same pivot?")
        theirs = dict(zip(other_names, other_lengths))
        for name, L in zip(names, lengths):
            if theirs[name] != L:
                raise ValueError(f"record {name!r} has {L} positions in {paths[0]} and {theirs[name]} in {path}: is this the same pivot?")
    kept = [(name, L) for name, L in zip(names, lengths) if L]          # (a record whose rows all start at 0 has no position)
    names = [name for name, _ in kept]
    rec_begin = np.concatenate([[0], np.cumsum([L for _, L in kept])]).astype(np.int64)

    def write(tmps):
        with contextlib.ExitStack() as stack:
            writers = [stack.enter_context(RowWriter(tmp)) for tmp in tmps[:len(outputs)]]
            if kept:
                builders = stack.enter_context(Builders(len(plane_of), rec_begin, [order for _, order in outputs], device))
                mapped = stack.enter_context(_mapped(sizes, plane_of, device))
            for name, L in kept:
                with contextlib.ExitStack() as record:
                    feeds = []
                    for path in paths:
                        feed, buf = region_feed(path, name, device)
                        record.enter_context(buf)
                        feeds.append(feed)
                    for parts in record_rows(list(zip(feeds, sizes)), L, builders, device, slice_positions, batch_positions, *mapped):
                        for writer, part in zip(writers, parts):
                            writer.write(names, part)
                log(f"{name}: {L} positions")
        if list_out:
            with open(tmps[-1], "w") as fh:
                fh.write("".join(line + "\n" for line in merged_list(lists, chosen)))
        return [w.rows for w in writers]

    written = []
    replace_all_into(written_paths, lambda tmps: written.extend(write(tmps)))
    return {"positions": int(rec_begin[-1]), "genomes": len(plane_of) + 1, "rows": written}
