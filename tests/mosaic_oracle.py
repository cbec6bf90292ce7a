"""The definition `memo mosaic` is tested against, in NumPy and plain Python.

With best, ok and winner per position as `memo nearest` defines them (tests/nearest_oracle.py: per_position)

    step = best where ok, else 1            p_0 = 0;  p_{i+1} = p_i + max(step[p_i], 1)  while p_i < L            (the reached positions)

phrase i is [p_i, min(p_{i+1}, L)) of genome winner[p_i] (0: none).  A line is a phrase; consecutive none-phrases are one line; adjacent
phrases of one genome stay two.  greedy() walks one phrase at a time and merges through the PREVIOUS PHRASE, not through flags;
fewest() is the dynamic programme the greedy count is held against; bin_naive() cuts the lines at bin edges one base at a time."""
import numpy as np

from tests import nearest_oracle


def steps(v, cap, min_len=1, candidates=None):
    """(step uint32 [L], winner uint16 [L]) of cells [planes, L]"""
    best, ok, _, _, winner = nearest_oracle.per_position(v, cap, min_len, candidates)
    return np.where(ok, best, 1).astype(np.uint32), winner


def reached(step):
    """the reached positions, one hop at a time (a step of 0 counts as 1)"""
    step = np.asarray(step)
    out, p = [], 0
    while p < len(step):
        out.append(p)
        p += max(int(step[p]), 1)
    return out


def greedy(step, winner):
    """(starts int64 [R], genomes uint16 [R]): the lines"""
    winner = np.asarray(winner)
    starts, genomes = [], []
    previous = None                                   # the genome of the phrase before this one
    for p in reached(step):
        g = int(winner[p])
        if not (g == 0 and previous == 0):            # a none-phrase behind a none-phrase goes on with its line
            starts.append(p)
            genomes.append(g)
        previous = g
    return np.asarray(starts, np.int64), np.asarray(genomes, np.uint16)


def fewest(best):
    """the fewest pieces [p, p + l), 1 <= l <= max(best[p], 1), that cover [0, L) exactly: the dynamic programme, O(L x reach)"""
    best = [max(int(b), 1) for b in best]
    L = len(best)
    need = [0] + [L + 1] * L                         # need[q]: the fewest pieces that cover [0, q)
    for p in range(L):
        for q in range(p + 1, min(p + best[p], L) + 1):
            need[q] = min(need[q], need[p] + 1)
    return need[L]


def bin_naive(starts, genomes, L, edges, n_docs):
    """(bases uint64 [N, B], lines uint64 [B]), one base at a time"""
    starts, genomes, edges = [int(s) for s in starts], [int(g) for g in genomes], [int(e) for e in edges]
    bins = len(edges) - 1
    bases, lines = np.zeros((n_docs, bins), np.uint64), np.zeros(bins, np.uint64)
    ends = starts[1:] + [L]
    for s, e, g in zip(starts, ends, genomes):
        for p in range(s, e):
            hit = [b for b in range(bins) if edges[b] <= p < edges[b + 1]]
            assert len(hit) == 1, "every position lies in exactly one bin"
            bases[g, hit[0]] += np.uint64(1)
            if p == s:
                lines[hit[0]] += np.uint64(1)
    return bases, lines


def window_lines(s, e, a, qs, qe, cap, n_docs, *, min_len=1, candidates=None):
    """(starts from qs, genomes) of the window of a membership index's rows"""
    v = nearest_oracle.window_planes(s, e, a, qs, qe, cap, n_docs)
    return greedy(*steps(v, cap, min_len, candidates))


def intervals(starts, genomes, end, first=0):
    starts = [int(x) + first for x in starts]
    return list(zip(starts, starts[1:] + [end], [int(g) for g in genomes]))
