"""The definition `memo merge` is tested against, in NumPy, built on tests/convert_oracle.py and oracle/dap_oracle.py and
changing neither.

Per pivot record R of Lrec positions, with the rows (s, e, a) of the record in input s of N_s genomes and the chosen (s, g) in output order:

    ms_s   = convert_oracle.ms(s, e, a, N_s, length=Lrec)                           int64 [Lrec, N_s - 1]
    M      = [ ms_s[:, g - 1] for each chosen (s, g) ]                              W columns
    rows   = dap_oracle.dap_rows(M, [0, Lrec], overlap=True, order)                 order=False: -o, order=True: -c

A source is (start, end, annot, n_docs, selection); a selection is a list of annots, None: all, ascending.  Records keep the order of first
appearance in the first input; a record with Lrec = 0 is dropped."""
import numpy as np

from oracle import dap_oracle
from tests import convert_oracle


def selection(chosen, n_docs):
    return list(range(1, n_docs)) if chosen is None else [int(g) for g in chosen]


def matrix(sources, length):
    """int64 [Lrec, W]: the chosen columns in output order"""
    cols = []
    for s, e, a, n_docs, chosen in sources:
        ms = convert_oracle.ms(s, e, a, n_docs, length)
        cols += [ms[:, g - 1] for g in selection(chosen, n_docs)]
    return np.stack(cols, axis=1)


def rows(sources, length, order):
    """(start, end, annot) int64 of one record's rows in the index of the chosen genomes, in file order"""
    if not length:
        return tuple(np.empty(0, np.int64) for _ in range(3))
    _rec, start, end, annot = dap_oracle.dap_rows(matrix(sources, length), np.asarray([0, length], np.int64), overlap=True, order=order)
    return start.astype(np.int64), end.astype(np.int64), annot.astype(np.int64)


def index_rows(inputs, order, lengths=None):
    """(record names, start, end, annot) of a whole output.  inputs = [({record: (s, e, a)} in order of first appearance, n_docs,
    selection), ...]; lengths: {record: Lrec} (default: the largest row start in the first input)"""
    names, parts = [], []
    for name in inputs[0][0]:
        L = int(inputs[0][0][name][0].max()) if lengths is None else lengths[name]
        part = rows([(*index[name], n_docs, chosen) for index, n_docs, chosen in inputs], L, order)
        names += [name] * len(part[0])
        parts.append(part)
    return (names, *(np.concatenate([p[i] for p in parts]) for i in range(3)))


def renumbered(canonical):
    """The -o rows without the planes and without the matrix: canonical = [((s, e, a) of one record in canonical form, n_docs,
    selection), ...]; the rows whose annot is chosen, renumbered to the output's annots, in the order of (start, new annot)."""
    out = [[], [], []]
    base = 0
    for (s, e, a), n_docs, chosen in canonical:
        picks = selection(chosen, n_docs)
        new = np.zeros(n_docs, np.int64)
        new[picks] = base + 1 + np.arange(len(picks))
        keep = new[a] > 0
        for column, part in zip(out, (s[keep], e[keep], new[a[keep]])):
            column.append(part)
        base += len(picks)
    s, e, a = (np.concatenate(c).astype(np.int64) for c in out)
    at = np.lexsort((a, s))
    return s[at], e[at], a[at]


def by_record(names, s, e, a):
    """{record: (s, e, a)} in order of first appearance, from the columns of a whole index"""
    names = np.asarray(names, dtype=object)
    out = {}
    for name in dict.fromkeys(names.tolist()):
        sel = names == name
        out[name] = tuple(np.ascontiguousarray(c[sel], np.int64) for c in (s, e, a))
    return out
