"""The oracle of `memo cover` (test infrastructure; the product never imports it): the greedy cover of match lengths over every k of
[kmin, kmax], by NumPy on whole planes, every candidate rescored at every step.

With span = kmax - kmin + 1 and the weights w[g][p] = max(0, min(len[g][p], kmax) - (kmin - 1)) of the planes of `memo lengths`
(tests/lengths_oracle.planes), the state is two integer vectors over the positions, core (span everywhere) and covered (zeros);
taking genome g does core = min(core, w[g]), covered = max(covered, w[g]).  The score of a candidate g is
new = sum(max(0, w[g] - covered)) and kept = sum(min(w[g], core)); a step takes the largest key, (new, kept, -g) under "covered",
(kept, new, -g) under "core".  The seeds go first in the order written and leave the candidates; steps go on until the candidates
are used up, `most` genomes beyond the pivot are taken (seeds included), or -- before a step that is no seed's -- the sum of covered
has reached ceil(fraction x L x span), the fraction read as the decimal it is written as.  Every comparison against it is exact."""
import fractions
import math

import numpy as np


def weights(lengths, kmin, kmax):
    """int64 [N, L]: the number of k in [kmin, kmax] with k <= lengths[g][p]"""
    v = np.minimum(np.asarray(lengths).astype(np.int64), int(kmax))
    return np.maximum(v - (int(kmin) - 1), 0)


def scores(w, core, covered):
    """(new, kept) of one plane against the two vectors, as Python integers"""
    w = np.asarray(w, np.int64)
    return int(np.maximum(w - covered, 0).sum()), int(np.minimum(w, core).sum())


def greedy(W, span, objective="covered", candidates=None, seeds=(), most=None, fraction=None):
    """(order, core, covered) as lists, one entry per genome taken; W: weights [N, L], row 0 the pivot's (never read)"""
    W = np.asarray(W).astype(np.int64)
    N, L = W.shape
    seeds = [int(g) for g in seeds]
    assert len(set(seeds)) == len(seeds) and all(1 <= g < N for g in seeds) and objective in ("covered", "core")
    remaining = [int(g) for g in (range(1, N) if candidates is None else candidates) if int(g) not in seeds]
    assert len(set(remaining)) == len(remaining) and all(1 <= g < N for g in remaining)
    most = len(seeds) + len(remaining) if most is None else most
    assert most >= len(seeds)
    stop_at = None if fraction is None else math.ceil(fractions.Fraction(str(fraction)) * L * int(span))
    core, covered = np.full(L, int(span), np.int64), np.zeros(L, np.int64)
    order, s_core, s_covered = [], [], []

    def take(g):
        nonlocal core, covered
        core, covered = np.minimum(core, W[g]), np.maximum(covered, W[g])
        order.append(g)
        s_core.append(int(core.sum()))
        s_covered.append(int(covered.sum()))
    for g in seeds:
        take(g)
    while remaining and len(order) < most and (stop_at is None or int(covered.sum()) < stop_at):
        sc = {g: scores(W[g], core, covered) for g in remaining}
        key = (lambda g: (sc[g][0], sc[g][1], -g)) if objective == "covered" else (lambda g: (sc[g][1], sc[g][0], -g))
        best = max(remaining, key=key)
        remaining.remove(best)
        take(best)
    return order, s_core, s_covered


def rows(result):
    """(added, core, covered) per genome taken, as the tables of the documents list them"""
    return list(zip(*result))
