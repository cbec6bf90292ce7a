"""`memo panel`: which genomes give the collector's curve, in which order -- the greedy set cover of a window's membership bits.

No counterpart in the reference.  `memo collect` draws the curve of an order that is given; this driver chooses the order: the
state is two masks over the window's positions, core (all ones at first) and covered (all zeros); taking genome g does
core &= B[:, g], covered |= B[:, g]; the score of a candidate g is the pair

    new  = |B[:, g] & ~covered|        kept = |B[:, g] & core|

and a step takes the candidate with the largest key, (new, kept, -g) under the objective "covered", (kept, new, -g) under "core":
ties go to the lowest annot.  Every step depends on all the steps before it over the whole window, so the rows cannot be folded
slice by slice and forgotten as matrix, collect and tracks fold them: the window is swept in slices (_window.membership_slices), each
slice is packed into genome-major bit planes that stay in HBM (memo_panel_planes_dev, memo_amd/csrc/memo_panel.hip), and a step is a
stream over planes: memo_panel_score_dev for the candidates a step has to look at, the choice on the host, memo_panel_take_dev for
the winner.  Only the scores and two counts per step cross to the host.

Choosing is lazy and exact: new and kept never increase as genomes are taken, so the scores a candidate was last seen with are
upper bounds of its key.  A step scores the candidates in descending order of their bound keys, a few at a time, and stops as soon
as the best fresh key is at least the next bound key; it never scores more planes than rescoring every remaining candidate.  A
call of the library costs the host more than the device needs for a few hundred megabytes of planes, so a step is two calls at the
most: the largest bounds first (at least 8 planes, and as many as LAZY_BYTES hold), then everyone whose bound still beats the best
fresh key.  The flags are memo_amd/panel_cli.py.
"""
import fractions
import math

import numpy as np

from ._device import DevBuffer
from ._lib import check, lib
from ._window import membership_slices, parse_region
from .merge import parse_selection

OBJECTIVES = ("covered", "core")
N_MIN, N_MAX = 2, 2048
LAZY_BATCH = 8          # planes a lazy step's first call scores at least: one block of candidates of the score kernel
LAZY_BYTES = 256 << 20  # ... and as many more as this many bytes of planes hold: what the device reads in about the time a call costs
#                         on the host (profiles/panel_timing.txt), so that short planes are scored in one call a step

_scored = 0


def planes_scored():
    """planes the score kernel read during the last region_panel / greedy of this process"""
    return _scored


def tile():
    """positions per tile of memo_panel_planes_dev: the lengths a test wants to straddle"""
    return int(lib().memo_panel_tile())


def pass_words():
    """mask words a workgroup of the score and take kernels reads per pass"""
    return int(lib().memo_panel_pass_words())


def threshold(fraction, L):
    """ceil(FRACTION x L) of -f, exactly: the fraction is read as the decimal it is written as (0.7 x 20 is 14, not the 15 of binary
    floating point); None: no threshold"""
    if fraction is None:
        return None
    try:
        value = fractions.Fraction(fraction if isinstance(fraction, (str, int)) else repr(float(fraction)))
    except (ValueError, ZeroDivisionError):
        raise ValueError(f"the fraction {fraction!r} is not a number") from None
    if not 0 <= value <= 1:
        raise ValueError(f"the fraction must lie in [0, 1] (got {fraction})")
    return math.ceil(value * int(L))


def plan(n_docs, objective="covered", candidates=None, seeds=None, max_genomes=None):
    """(candidates without the seeds, seeds, the most genomes beyond the pivot) after every check that needs no window: what the
    command line and region_panel both refuse"""
    n_docs = int(n_docs)
    if not N_MIN <= n_docs <= N_MAX:
        raise ValueError(f"n_docs must be in [{N_MIN}, {N_MAX}]")
    if objective not in OBJECTIVES:
        raise ValueError(f"the objective must be one of {', '.join(OBJECTIVES)} (got {objective!r})")
    seeds = [] if seeds is None else parse_selection(seeds, n_docs)
    taken = set(seeds)
    cand = [g for g in parse_selection(candidates, n_docs) if g not in taken]
    most = len(seeds) + len(cand)
    if max_genomes is not None:
        if int(max_genomes) < len(seeds):
            raise ValueError(f"max_genomes = {int(max_genomes)} is below the {len(seeds)} seeds")
        most = min(most, int(max_genomes))
    return cand, seeds, most


def _key(objective, new, kept, g):
    return (new, kept, -g) if objective == "covered" else (kept, new, -g)


def greedy(score, take, L, candidates, seeds=(), objective="covered", most=None, stop_at=None, lazy=True, batch=None):
    """The steps, on any pair of functions score(list of genomes) -> [[new, kept], ...] and take(g) -> (core, covered) that keep the
    masks between them (the device's in region_panel, NumPy's in the tests).  Returns (order, core, covered) as lists, one entry per
    genome taken: the seeds first, in the order written, then the greedy's choices among `candidates` until they are used up, `most`
    genomes are taken, or -- before a step that is no seed's -- covered has reached `stop_at`."""
    global _scored
    _scored = 0
    L = int(L)
    batch = LAZY_BATCH if batch is None else max(1, int(batch))
    most = len(seeds) + len(candidates) if most is None else most
    order, core, covered = [], [], []

    def taking(g):
        a, o = take(g)
        order.append(int(g))
        core.append(int(a))
        covered.append(int(o))
    for g in list(seeds)[:most]:
        taking(g)
    bound = {int(g): (L, L) for g in candidates}          # the last scores seen: upper bounds of what a score would be now
    seen = covered[-1] if covered else 0
    while bound and len(order) < most and (stop_at is None or seen < stop_at):
        if lazy:
            queue = sorted(bound, key=lambda g: _key(objective, *bound[g], g), reverse=True)
            best, at = None, 0
            while at < len(queue) and (best is None or _key(objective, *bound[best], best) < _key(objective, *bound[queue[at]], queue[at])):
                # the first call of a step takes the `batch` largest bounds; a second one everyone whose bound still beats the best
                # fresh key, all of whom have to be looked at: a step is two calls at the most
                end = at + batch
                if best is not None:
                    end = at + 1
                    while end < len(queue) and _key(objective, *bound[best], best) < _key(objective, *bound[queue[end]], queue[end]):
                        end += 1
                chunk = queue[at:end]
                at += len(chunk)
                for g, (new, kept) in zip(chunk, score(chunk)):
                    bound[g] = (int(new), int(kept))
                _scored += len(chunk)
                fresh = max(chunk, key=lambda g: _key(objective, *bound[g], g))
                if best is None or _key(objective, *bound[best], best) < _key(objective, *bound[fresh], fresh):
                    best = fresh
        else:
            queue = sorted(bound)
            for g, (new, kept) in zip(queue, score(queue)):
                bound[g] = (int(new), int(kept))
            _scored += len(queue)
            best = max(queue, key=lambda g: _key(objective, *bound[g], g))
        del bound[best]
        taking(best)
        seen = covered[-1]
    return order, core, covered


def _result(order, core, covered):
    return np.array(order, np.uint16), np.array(core, np.uint64), np.array(covered, np.uint64)


class Planes:
    """a window's rows as genome-major bit planes on the device, and the two masks of the steps: what region_panel keeps between its
    calls of the library.  The planes are n_docs x words uint32, words = ceil(L / 32) rounded up to a multiple of 4."""

    def __init__(self, L, n_docs, device=0):
        self.L, self.n_docs, self.device = int(L), int(n_docs), device
        self.words = (-(-self.L // 32) + 3) // 4 * 4
        self.buffers = []
        try:
            self.planes = self._buffer(4 * self.words * self.n_docs)
            self.core, self.covered = self._buffer(4 * self.words), self._buffer(4 * self.words)
        except BaseException:
            self.close()
            raise

    def _buffer(self, nbytes):
        self.buffers.append(DevBuffer(self.device, max(nbytes, 16)))
        return self.buffers[-1]

    def pack(self, d_bits, positions, first):
        """a slice's rows (device pointer, uint32 [positions, W]) into the planes; `first`: the slice's first window position, a
        multiple of 32"""
        if first % 32:
            raise ValueError("a slice must begin at a multiple of 32 positions of its window")
        check(lib().memo_panel_planes_dev(d_bits, positions, self.n_docs, self.planes.d, self.words, first // 32, self.device, None))

    def begin(self):
        check(lib().memo_panel_begin_dev(self.planes.d, self.words, self.n_docs, self.L, self.core.d, self.covered.d, self.device, None))

    def score(self, genomes):
        ids = np.ascontiguousarray(genomes, np.uint16)
        out = np.zeros((len(ids), 2), np.uint64)
        check(lib().memo_panel_score_dev(self.planes.d, self.words, self.n_docs, self.words, self.core.d, self.covered.d, ids.ctypes.data, len(ids),
                                         out.ctypes.data, self.device, None))
        return out.tolist()

    def take(self, genome):
        out = np.zeros(2, np.uint64)
        check(lib().memo_panel_take_dev(self.planes.d, self.words, self.n_docs, self.words, int(genome), self.core.d, self.covered.d, out.ctypes.data,
                                        self.device, None))
        return int(out[0]), int(out[1])

    def close(self):
        for buf in self.buffers:
            buf.close()
        self.buffers = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _checked(L, n_docs, objective, candidates, seeds, max_genomes, fraction, slice_positions):
    """plan's triple and the threshold of a window of L positions, or the refusal"""
    if L < 0:
        raise ValueError("negative dimensions are not allowed")
    if int(slice_positions) < 32 or int(slice_positions) % 32:
        raise ValueError("slice_positions must be a positive multiple of 32")
    return (*plan(n_docs, objective, candidates, seeds, max_genomes), threshold(fraction, L))


def region_panel(index_path, region, k, n_docs, objective="covered", candidates=None, seeds=None, max_genomes=None, fraction=None, device=0,
                 slice_positions=1 << 24, lazy=True):
    """The greedy order of a window of a Parquet MEMBERSHIP index.  candidates / seeds: merge.parse_selection's syntax (a string, a
    list of annots, None: every genome but the pivot / no seed); max_genomes: the most genomes beyond the pivot, seeds included;
    fraction: stop before any step that is no seed's once covered >= ceil(fraction x L).  The window is swept in slices of at most
    slice_positions (a multiple of 32) into one reused buffer, each slice is packed into the resident planes, then the steps run.
    One device.  Returns (order uint16 [M], core uint64 [M], covered uint64 [M], L); an empty window touches no device and has no
    step.  planes_scored() then says how many planes the steps scored; lazy=False rescores every remaining candidate at every step."""
    record, qs, qe = parse_region(region)
    args = (k, n_docs, objective, candidates, seeds, max_genomes, fraction, device, slice_positions, lazy)
    _checked(qe - qs, n_docs, objective, candidates, seeds, max_genomes, fraction, slice_positions)      # before any file is opened
    if qe == qs:
        return index_panel(None, qs, qe, *args)
    from . import memo_query
    with memo_query.region_index(index_path, record, qs, qe + k, device=device, k=k, num_docs=n_docs, membership=True) as index:
        return index_panel(index, qs, qe, *args)


def index_panel(index, qs, qe, k, n_docs, objective="covered", candidates=None, seeds=None, max_genomes=None, fraction=None, device=0,
                slice_positions=1 << 24, lazy=True):
    """region_panel on the window [qs, qe) of a DeviceIndex that holds the window's membership rows (the index stays the caller's; an
    empty window never looks at it)"""
    global _scored
    L = qe - qs
    cand, seeds, most, stop_at = _checked(L, n_docs, objective, candidates, seeds, max_genomes, fraction, slice_positions)
    _scored = 0
    if L == 0:
        return (*_result([], [], []), 0)
    with Planes(L, n_docs, device) as planes:
        for d_bits, s, e in membership_slices(index, qs, qe, k, n_docs, slice_positions, device):
            planes.pack(d_bits, e - s, s - qs)
        planes.begin()
        batch = max(LAZY_BATCH, LAZY_BYTES // (4 * planes.words))
        return (*_result(*greedy(planes.score, planes.take, L, cand, seeds, objective, most, stop_at, lazy, batch)), L)


def format_panel(L, order, core, covered, labels=None):
    """the text of `memo panel`: collect's curve of the one order with the genome each line adds (labels: one per genome, the pivot
    first; None: the annots as decimal strings).  An empty window is an empty file."""
    from .collect import format_curves
    if int(L) == 0:
        return ""
    order = np.asarray(order, np.int64)
    if labels is None:
        labels = [str(g) for g in range(int(order.max()) + 1 if len(order) else 1)]
    return format_curves(L, np.asarray(core)[None], np.asarray(covered)[None], "curve", order[None], labels)
