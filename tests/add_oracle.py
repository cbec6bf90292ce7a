"""The definition `memo add` is tested against, in NumPy, built on oracle/ms_oracle.py, oracle/dap_oracle.py and
tests/convert_oracle.py and changing none of them.

Per pivot record R of Lrec positions with the rows (s, e, a) of the input index, N genomes in it and m new genomes:

    old[p][g - 1] = convert_oracle.ms(s, e, a, N)[p][g - 1]                             1 <= g < N: what the index says, clipped at the record's end
    new[p][j]     = ms_oracle.ms_records([R], genome_text(new genome j))[p]             0 <= j < m: the records, their reverse complements, NULs
    rows out      = dap_oracle.dap_rows([old | new], rec_begin, overlap=True, order)    order=False: -o, order=True: -c; records in FASTA order"""
import numpy as np

from oracle import dap_oracle, ms_oracle
from tests import convert_oracle

_COMPLEMENT = bytes.maketrans(b"ACGTRYKMBVDH", b"TGCAYRMKVBHD")


def genome_text(seqs):
    """S_1 $ ... S_s $ rc(S_1) $ ... rc(S_s) $ with $ = NUL: memo_amd.build_index.genome_text, restated"""
    seqs = [bytes(s) for s in seqs]
    if not seqs:
        return b""
    return b"\0".join(seqs + [s.translate(_COMPLEMENT)[::-1] for s in seqs]) + b"\0"


def new_ms(record, genomes):
    """int64 [Lrec, m]: the matching statistics of one pivot record against every new genome (a list of record sequences each)"""
    out = np.zeros((len(record), len(genomes)), np.int64)
    for j, seqs in enumerate(genomes):
        out[:, j] = ms_oracle.ms_records([bytes(record)], genome_text(seqs))
    return out


def matrix(s, e, a, n_docs, record, genomes):
    """int64 [Lrec, N - 1 + m]: the old columns as the index says them beside the new ones"""
    return np.hstack([convert_oracle.ms(s, e, a, n_docs, len(record)), new_ms(record, genomes)])


def rows(s, e, a, n_docs, record, genomes, order):
    """(start, end, annot) int64 of one record's rows in the index of N + m genomes, in file order"""
    L = len(record)
    _rec, start, end, annot = dap_oracle.dap_rows(matrix(s, e, a, n_docs, record, genomes), np.asarray([0, L], np.int64), overlap=True, order=order)
    return start.astype(np.int64), end.astype(np.int64), annot.astype(np.int64)


def index_rows(pivot, index, n_docs, genomes, order):
    """(record names, start, end, annot) of a whole index: pivot is [(name, sequence)] in FASTA order, index {name: (s, e, a)}"""
    names, parts = [], []
    for name, seq in pivot:
        part = rows(*index[name], n_docs, seq, genomes, order)
        names += [name] * len(part[0])
        parts.append(part)
    return (names, *(np.concatenate([p[i] for p in parts]) for i in range(3)))


def built_rows(pivot, genomes, order):
    """the rows `memo index` writes on the pivot [(name, sequence)] and all `genomes`, by the oracles alone: {name: (s, e, a)}"""
    out = {}
    for name, seq in pivot:
        L = len(seq)
        _rec, start, end, annot = dap_oracle.dap_rows(new_ms(seq, genomes), np.asarray([0, L], np.int64), overlap=True, order=order)
        out[name] = (start.astype(np.int64), end.astype(np.int64), annot.astype(np.int64))
    return out
