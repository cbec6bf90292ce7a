"""The oracle of `memo panel` (test infrastructure; the product never imports it): the greedy set cover of unpacked membership bits
B uint8 [L, N], by NumPy on whole columns, every candidate rescored at every step.

The state is two boolean masks over the positions, core (all True) and covered (all False); taking genome g does
core &= B[:, g], covered |= B[:, g].  The score of a candidate g is new = |B[:, g] & ~covered| and kept = |B[:, g] & core|; a step
takes the largest key, (new, kept, -g) under "covered", (kept, new, -g) under "core".  The seeds go first in the order written and
leave the candidates; steps go on until the candidates are used up, `most` genomes beyond the pivot are taken (seeds included), or
-- before a step that is no seed's -- covered has reached ceil(fraction x L), the fraction read as the decimal it is written as.
Every comparison against it is exact."""
import fractions
import math

import numpy as np


def greedy(B, objective="covered", candidates=None, seeds=(), most=None, fraction=None):
    """(order, core, covered) as lists, one entry per genome taken"""
    B = np.asarray(B).astype(bool)
    L, N = B.shape
    seeds = [int(g) for g in seeds]
    assert len(set(seeds)) == len(seeds) and all(1 <= g < N for g in seeds) and objective in ("covered", "core")
    remaining = [int(g) for g in (range(1, N) if candidates is None else candidates) if int(g) not in seeds]
    assert len(set(remaining)) == len(remaining) and all(1 <= g < N for g in remaining)
    most = len(seeds) + len(remaining) if most is None else most
    assert most >= len(seeds)
    stop_at = None if fraction is None else math.ceil(fractions.Fraction(str(fraction)) * L)
    core, covered = np.ones(L, bool), np.zeros(L, bool)
    order, n_core, n_covered = [], [], []

    def take(g):
        nonlocal core, covered
        core, covered = core & B[:, g], covered | B[:, g]
        order.append(g)
        n_core.append(int(core.sum()))
        n_covered.append(int(covered.sum()))
    for g in seeds:
        take(g)
    while remaining and len(order) < most and (stop_at is None or int(covered.sum()) < stop_at):
        scores = {g: (int((B[:, g] & ~covered).sum()), int((B[:, g] & core).sum())) for g in remaining}
        key = (lambda g: (scores[g][0], scores[g][1], -g)) if objective == "covered" else (lambda g: (scores[g][1], scores[g][0], -g))
        best = max(remaining, key=key)
        remaining.remove(best)
        take(best)
    return order, n_core, n_covered


def rows(result):
    """(added, core, covered) per genome taken, as the tables of the documents list them"""
    return list(zip(*result))
