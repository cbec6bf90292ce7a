"""`memo cover`: which genomes cover the pivot's matches, in which order, at every k -- `memo panel` summed over the k of [kmin, kmax].

No counterpart in the reference.  `memo panel` chooses at ONE k, and presence at one k saturates; the choice of k changes the order
more than it changes any other summary.  The lengths len[g][p] of `memo lengths` do not saturate: bit g of `memo query -m -k k` is
set exactly when k <= len[g][p] (index rows with end >= start), so with `memo pairs`' weights

    span    = kmax - kmin + 1
    w[g][p] = max(0, min(len[g][p], kmax) - (kmin - 1))        the number of k in [kmin, kmax] at which genome g holds the k-mer at p

`memo panel -k k`'s two masks, stacked over every k of [kmin, kmax], are two integer vectors over the positions: core[p], the smallest
weight taken so far (span at first), and covered[p], the largest (0 at first).  Taking genome g does core = min(core, w[g]),
covered = max(covered, w[g]); the score of a candidate g is the pair

    new  = sum over p of max(0, w[g][p] - covered[p])        kept = sum over p of min(w[g][p], core[p])

which are `memo panel -k k`'s new and kept summed over k = kmin .. kmax; the sums of core and covered are `memo collect`'s two
columns summed the same way, and with kmin = kmax = k everything is `memo panel -k k`, number for number.  Both scores never increase
as genomes are taken (a sum of maxima is monotone submodular), so panel.greedy's lazy, exact choice applies unchanged: this module
hands it the device's score and take.

The window comes through `memo lengths`' slices with cap = kmax, from the right; each finished slice is turned into weights where
it lies (memo_cover_weights_dev, memo_amd/csrc/memo_cover.hip) and written into resident planes -- of the genomes the candidates and
the seeds name, and of no other: the pivot has no plane, a genome outside both lists is never read.  A cell is 2 bytes while
span <= 65535 and 4 above, which halves every step's traffic for the caps people pass.  Only scores and two sums per step cross to the
host.  The flags are memo_amd/cover_cli.py.
"""
import numpy as np

from . import panel
from ._device import DevBuffer
from ._lib import MemoError, check, lib
from ._window import parse_region
from .lengths import default_slice_positions, finished_slices, region_feed
from .maxk import CAP_MAX

OBJECTIVES = panel.OBJECTIVES
N_MIN, N_MAX = panel.N_MIN, panel.N_MAX
L_MAX = 2 ** 31 - 1
NARROW_SPAN = 65535     # the largest span whose weights fit cells of 2 bytes

_scored = 0


def planes_scored():
    """planes the score kernel read during the last region_cover of this process"""
    return _scored


def pass_cells(cell_bytes):
    """cells a workgroup of the score and take kernels reads per pass: the lengths a test wants to straddle"""
    return int(lib().memo_cover_pass_cells(int(cell_bytes)))


def cell_bytes_of(span):
    return 2 if int(span) <= NARROW_SPAN else 4


def span_of(kmin=1, kmax=None):
    """(kmin, kmax, span), or the ValueError of limits outside 1 <= kmin <= kmax <= 2^31 - 1"""
    kmax = CAP_MAX if kmax is None else int(kmax)
    if not 1 <= kmax <= CAP_MAX:
        raise ValueError(f"kmax must be in [1, {CAP_MAX}]")
    if not 1 <= int(kmin) <= kmax:
        raise ValueError(f"kmin must be in [1, {kmax}]")
    return int(kmin), kmax, kmax - int(kmin) + 1


def slice_step(n_docs, slice_positions=None):
    """the positions per slice: a positive multiple of 8 (a slice begins at a quad of the planes in either cell width); None: what
    keeps `memo lengths`' cells within 2 GiB, rounded down to one"""
    if slice_positions is None:
        return max(default_slice_positions(n_docs) // 8 * 8, 8)
    if int(slice_positions) < 8 or int(slice_positions) % 8:
        raise ValueError("slice_positions must be a positive multiple of 8")
    return int(slice_positions)


class Weights:
    """the weight planes of the named genomes on the device, and the two vectors of the steps: what region_cover keeps between its
    calls of the library.  Plane i belongs to genomes[i]; the planes are len(genomes) x pitch cells of 2 or 4 bytes, pitch = L rounded
    up to 16 bytes of cells."""

    def __init__(self, L, genomes, kmin, kmax, device=0):
        self.kmin, self.kmax, self.span = span_of(kmin, kmax)
        self.L, self.device = int(L), device
        self.genomes = np.ascontiguousarray(genomes, np.uint16)
        self.cell_bytes = cell_bytes_of(self.span)
        quad = 16 // self.cell_bytes
        self.pitch = -(-self.L // quad) * quad
        self.plane_bytes = self.pitch * self.cell_bytes
        self.buffers = []
        try:
            self.weights = self._buffer(self.plane_bytes * len(self.genomes), f"the weight planes of {len(self.genomes)} genomes")
            self.core, self.covered = self._buffer(self.plane_bytes, "core"), self._buffer(self.plane_bytes, "covered")
        except BaseException:
            self.close()
            raise

    def _buffer(self, nbytes, what):
        nbytes = max(nbytes, 16)
        try:
            self.buffers.append(DevBuffer(self.device, nbytes))
        except MemoError as exc:
            raise MemoError(exc.code, f"{nbytes} bytes of device memory for {what} ({self.L} positions, cells of {self.cell_bytes} bytes): {exc}") from None
        return self.buffers[-1]

    def pack(self, d_lengths, positions, pitch_src, n_docs, first):
        """a finished slice of `memo lengths` (device pointer, uint32 [n_docs, pitch_src]) into the planes; `first`: the slice's
        first window position, a multiple of 8"""
        if first % 8:
            raise ValueError("a slice must begin at a multiple of 8 positions of its window")
        check(lib().memo_cover_weights_dev(d_lengths, positions, pitch_src, n_docs, self.kmin, self.kmax, self.genomes.ctypes.data, len(self.genomes),
                                           self.weights.d, self.pitch, self.cell_bytes, first, self.device, None))

    def begin(self):
        check(lib().memo_cover_begin_dev(self.weights.d, self.pitch, max(len(self.genomes), 1), self.cell_bytes, self.L, self.span, self.core.d, self.covered.d,
                                         self.device, None))

    def score(self, planes):
        ids = np.ascontiguousarray(planes, np.uint16)
        out = np.zeros((len(ids), 2), np.uint64)
        check(lib().memo_cover_score_dev(self.weights.d, self.pitch, len(self.genomes), self.cell_bytes, self.pitch, self.core.d, self.covered.d,
                                         ids.ctypes.data, len(ids), out.ctypes.data, self.device, None))
        return out.tolist()

    def take(self, plane):
        out = np.zeros(2, np.uint64)
        check(lib().memo_cover_take_dev(self.weights.d, self.pitch, len(self.genomes), self.cell_bytes, self.pitch, int(plane), self.core.d, self.covered.d,
                                        out.ctypes.data, self.device, None))
        return int(out[0]), int(out[1])

    def close(self):
        for buf in self.buffers:
            buf.close()
        self.buffers = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _checked(qs, qe, n_docs, kmin, kmax, objective, candidates, seeds, max_genomes, fraction, slice_positions):
    """(kmin, kmax, span, candidates, seeds, most, stop_at, step) of a window, or the refusal: everything that needs no file"""
    kmin, kmax, span = span_of(kmin, kmax)
    L = qe - qs
    if L < 0:
        raise ValueError("negative dimensions are not allowed")
    if qs < 0:
        raise ValueError("the window starts before position 0 of the record")
    if L > L_MAX:
        raise ValueError(f"a window of at most {L_MAX} positions")
    cand, seeds, most = panel.plan(n_docs, objective, candidates, seeds, max_genomes)
    return kmin, kmax, span, cand, seeds, most, panel.threshold(fraction, L * span), slice_step(n_docs, slice_positions)


def region_cover(index_path, region, n_docs, kmin=1, kmax=None, objective="covered", candidates=None, seeds=None, max_genomes=None, fraction=None,
                 device=0, slice_positions=None, lazy=True):
    """The greedy order of a window of a Parquet MEMBERSHIP index over every k of [kmin, kmax] (kmax=None: 2^31 - 1).  candidates /
    seeds / max_genomes: region_panel's; fraction: stop before any step that is no seed's once the sum of covered has reached
    ceil(fraction x L x span).  The window is taken in `memo lengths`' slices of slice_positions (a multiple of 8) from the right, each
    slice is turned into weights in the resident planes of the named genomes, then the steps run.  One device.  Returns (order uint16
    [M], core uint64 [M], covered uint64 [M], L, span); an empty window touches no device and has no step.  planes_scored() then says
    how many planes the steps scored; lazy=False rescores every remaining candidate at every step.  The result depends on no slicing."""
    global _scored
    record, qs, qe = parse_region(region)
    kmin, kmax, span, cand, seeds, most, stop_at, step = _checked(qs, qe, n_docs, kmin, kmax, objective, candidates, seeds, max_genomes, fraction,
                                                                  slice_positions)                     # before any file is opened
    _scored = 0
    L, n_docs = qe - qs, int(n_docs)
    empty = np.array([], np.uint16), np.array([], np.uint64), np.array([], np.uint64)
    if L == 0:
        return (*empty, 0, span)
    named = list(seeds) + list(cand)              # plane i is genome named[i]
    if not named:
        return (*empty, L, span)
    plane_of = {g: i for i, g in enumerate(named)}
    feed, buf = region_feed(index_path, record, device)
    with buf, Weights(L, named, kmin, kmax, device) as weights:
        for a, b, d_lengths, pitch_src in finished_slices(feed, qs, L, n_docs, kmax, device, step, halo=0):
            weights.pack(d_lengths, b - a, pitch_src, n_docs, a - qs)
        weights.begin()
        batch = max(panel.LAZY_BATCH, panel.LAZY_BYTES // weights.plane_bytes)
        try:
            order, core, covered = panel.greedy(lambda genomes: weights.score([plane_of[g] for g in genomes]), lambda g: weights.take(plane_of[g]), L * span,
                                                cand, seeds, objective, most, stop_at, lazy, batch)
        finally:
            _scored = panel.planes_scored()
    return np.array(order, np.uint16), np.array(core, np.uint64), np.array(covered, np.uint64), L, span


def format_cover(L, span, order, core, covered, labels=None):
    """the text of `memo cover`: collect's curve of the one order over L x span, with the genome each line adds (labels: one per
    genome, the pivot first; None: the annots as decimal strings).  An empty window is an empty file."""
    from .collect import format_curves
    if int(L) == 0:
        return ""
    order = np.asarray(order, np.int64)
    if labels is None:
        labels = [str(g) for g in range(int(order.max()) + 1 if len(order) else 1)]
    return format_curves(int(L) * int(span), np.asarray(core)[None], np.asarray(covered)[None], "curve", order[None], labels)
