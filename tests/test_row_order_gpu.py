"""The order of the 4-byte rows inside a start bucket (memo_amd/csrc/memo_interleave.hip), word for word.

The pass rewrites the rows of every packed index in place (memo_index_pack, mode 2), again out of place by the first query
that has paid for it (memo_view.hip: order_words_on), and on every packed k-class view.  Its header says the order is "a
function of the bucket's rows alone": so it has a closed form, written here in numpy from that description (`row_order_reference`,
two lexsorts over the whole index), and every export of the device's words is compared with it by np.array_equal.

    mode  class          order inside a class                  (s = start mod 2^bucket_shift, ov = the overlap byte)
    0     none           the bucket sorted by (s, ov, annot)
    1     s              (ov, annot)
    2     s              (ov mod 32, ov, annot)
    3     annot mod 32   (s + ov, annot, s)                    on bucket_shift 5 only: elsewhere it is mode 2
    modes 1-3: the row of rank r in its class is in chunk q = r >> 2; the bucket is laid out by (q, class, r & 3)
    buckets of 0, 1 or more than 8192 rows stay as they are

A bucket takes one of several routes through the file, decided by thresholds that are constants of this module (LANE_ROWS ...
TURN).  `predict_routes` names the route of every bucket from the words as they ARRIVE and the mode asked for; before a device
is touched, `_assert_route_coverage` checks that the recipes below reach every route, per format, per mode, from start order and
from a dealt order.  If the kernel's constants move, that assertion says which recipes to move.

Recipes (bucket_shift 5; a turn = eight consecutive buckets, the first at a multiple of eight; a wave takes buckets 2w, 2w + 1):

    turn "lane pairs"      pairs with 0 .. 8 rows per start; both buckets full (32 starts x 8 rows: 512 rows in the pair);
                           first bucket empty; second bucket empty                                  -> lane_pair
    turn "lane edges"      1 row beside 0 rows (skipped: untouched); 1 row beside 200 rows at <= 8 per start (lane_pair);
                           1 row beside 200 rows with a start of 20 (wave_bucket, the lone row untouched); a pair in which one
                           start has 9 rows (the whole pair falls to wave_bucket)
    turn "at most four"    eight buckets with at most 4 rows per start (a turn of eight small buckets): lane_pair on the way out,
                           wave mode-0 counted on the way back to start order
    turn "class lengths"   one start of 9, 63, 64, 65, 95, 96, 97, 200 rows beside a few short starts: chunk table (<= 64)
                           against counting loop, counted (<= 96) against sorted
    turn "bucket sizes"    a start of 256 rows that is its bucket; buckets of 2, 63, 64, 65, 127, 128, 129 rows
    turn "residues"        buckets of 255 and 256 rows; then buckets whose rows arrive grouped by annot mod 32 with one class of
                           9, 63, 64, 65, 95, 96 rows: the counted routes of mode 3 (rows in start order are not grouped by
                           residue unless built so)
    turn "residues 2"      the same with a class of 97 and of 200 rows (sorted), and small buckets
    turn "block sizes"     257, 511, 512, 513 rows (<= 40 per start: block counted); 4096, 4097, 8191, 8192 rows (block sorted)
    turn "block classes"   8193 rows (untouched); longest start 96 (block counted) and 97 (block sorted); one start holding 8192
                           rows; residue buckets of 700 rows with longest class 96 / 97 (mode 3: block counted / sorted)
    turn "one large"       a bucket of 257 rows; the others hold 0, 1, 2, 3, 0, 5, 1 rows and go through block_bucket with it
    turn "tail"            six buckets, so that the table leaves a last turn of seven buckets

The first three turns sit at low positions, the others straddle start 2^16 (format 4) / 2^12 (format 12), where the start field of
the word wraps: the bits above the bucket (high_of) are non-zero and differ between the buckets of a pair.  The "small" index holds
the small turns only (no large turn: the flag word lets the large kernel exit at once) and leaves a last turn of ONE bucket.  Bucket
shifts 1, 3, 6, 8 take block_bucket for everything and record a request for order 4 as row_order 2.  A seeded random part (sizes
log-uniform in 0 .. 600, clumps of 1 .. 120 rows on one start) runs both formats through orders 2, 3, 4.

Orders are the A/B switch's (memo_debug_row_order): order = mode + 1."""
import numpy as np
import pytest

# ---- thresholds of memo_amd/csrc/memo_interleave.hip (the route a bucket takes) ----
LANE_ROWS = 8        # lane_pair: rows of one start (`if (c > 8) ok = false`)
TABLE_ROWS = 64      # wave_bucket: chunk table up to 4 * kWaveQ rows in the longest class, else the counting loop
COUNTED_ROWS = 96    # kCountedClass: a longer class is sorted, not counted
WAVE_ROWS = 256      # kWaveRows: a larger bucket sends its turn to the large kernel
BLOCK_ROWS = 8192    # kMaxBucketRows: a larger bucket is left alone
TURN = 8             # kTurn

N_DOCS = {4: 256, 12: 4096}
MAX_ANNOT = {4: 255, 12: 4095}
WRAP_TURN = {4: (1 << 16) // (32 * TURN), 12: (1 << 12) // (32 * TURN)}     # the turn that begins where the start field wraps
OPT_BUILD_COST_PCT = 3


# =====================================================================================================================
# the reference
# =====================================================================================================================
def fields(words, fmt):
    """(start field, overlap byte, annot) of packed words (include/memo_amd.h at memo_index_pack)"""
    w = np.asarray(words, np.uint32).astype(np.int64)
    if fmt == 12:
        return (w >> 8) & 0xFFF, w & 0xFF, w >> 20
    return w & 0xFFFF, (w >> 16) & 0xFF, w >> 24


def pack_words(s, e, o, fmt):
    """host columns -> the words memo_index_pack writes, in the order of the columns (start order)"""
    ov = np.minimum(e - s, 255)
    if fmt == 12:
        return (ov | ((s & 0xFFF) << 8) | (o << 20)).astype(np.uint32)
    return ((s & 0xFFFF) | (ov << 16) | (o << 24)).astype(np.uint32)


def bucket_table(s, shift):
    """buckets 0 .. (max start >> shift) + 1, plus one entry pinned to the row count"""
    nb = (int(s[-1]) >> shift) + 3
    boff = np.searchsorted(s, np.arange(nb, dtype=np.int64) << shift, side="left").astype(np.int64)
    boff[-1] = len(s)
    return boff


def _bucket_of_rows(boff):
    sizes = np.diff(boff)
    return np.repeat(np.arange(len(sizes), dtype=np.int64), sizes), sizes


def row_order_reference(words, boff, shift, fmt, mode):
    """the words of an index after the ordering pass in `mode`, from the description in the module docstring"""
    words = np.asarray(words, np.uint32)
    if fmt not in (4, 12):
        return words.copy()
    if mode == 3 and shift != 5:
        mode = 2
    bucket, sizes = _bucket_of_rows(boff)
    assert len(bucket) == len(words)
    start, ov, annot = fields(words, fmt)
    s = start & ((1 << shift) - 1)
    if mode == 0:
        cls, keys = np.zeros_like(s), (s, ov, annot)
    elif mode == 1:
        cls, keys = s, (ov, annot)
    elif mode == 2:
        cls, keys = s, (ov & 31, ov, annot)
    else:
        cls, keys = annot & 31, (s + ov, annot, s)
    first = np.lexsort(keys[::-1] + (cls, bucket))                     # by bucket, class, order inside the class
    b1, c1 = bucket[first], cls[first]
    n = len(words)
    idx = np.arange(n, dtype=np.int64)
    head = np.ones(n, bool)
    head[1:] = (b1[1:] != b1[:-1]) | (c1[1:] != c1[:-1])
    rank = idx - np.maximum.accumulate(np.where(head, idx, 0))         # a row's rank inside its class
    out = words[first]
    if mode:
        out = out[np.lexsort((rank & 3, c1, rank >> 2, b1))]           # by bucket, chunk, class, place in the chunk
    alone = ((sizes < 2) | (sizes > BLOCK_ROWS))[bucket]
    out[alone] = words[alone]
    return out


# =====================================================================================================================
# the route a bucket takes, from the thresholds
# =====================================================================================================================
def predict_routes(words, boff, shift, fmt, mode):
    """one route name per bucket, from the words as they arrive and the mode asked for"""
    if mode == 3 and shift != 5:
        mode = 2
    bucket, sizes = _bucket_of_rows(boff)
    nb = len(sizes)
    start, ov, annot = fields(words, fmt)
    s = start & ((1 << shift) - 1)
    cls = (annot & 31) if mode == 3 else s
    same = bucket[1:] == bucket[:-1]
    grouped, by_start = np.ones(nb, bool), np.ones(nb, bool)
    grouped[bucket[1:][same & (cls[1:] < cls[:-1])]] = False           # the classes do not come in rising order
    by_start[bucket[1:][same & (s[1:] < s[:-1])]] = False
    longest = np.bincount(bucket * 256 + cls, minlength=nb * 256).reshape(nb, 256).max(axis=1)
    longest_start = np.bincount(bucket * 256 + s, minlength=nb * 256).reshape(nb, 256).max(axis=1)
    padded = np.zeros((nb + TURN - 1) // TURN * TURN, np.int64)
    padded[:nb] = sizes
    small_turn = (padded.reshape(-1, TURN).max(axis=1) <= WAVE_ROWS) & (shift == 5)
    routes = ["untouched"] * nb
    for b in range(nb):
        rows = int(sizes[b])
        counted = bool(grouped[b]) and longest[b] <= COUNTED_ROWS
        if not small_turn[b // TURN]:
            if 2 <= rows <= BLOCK_ROWS:
                routes[b] = "block counted" if counted else "block sorted"
            continue
        a = b & ~1
        pair = [x for x in (a, a + 1) if x < nb]
        if sum(int(sizes[x]) for x in pair) < 2:
            continue
        if mode in (1, 2) and all(by_start[x] and longest_start[x] <= LANE_ROWS for x in pair):
            if rows:
                routes[b] = "lane_pair"
            continue
        if rows < 2:
            continue
        if mode == 0:
            routes[b] = "wave mode-0 counted" if counted else "wave sorted"
        else:
            how = "table" if longest[b] <= TABLE_ROWS else "loop"
            routes[b] = f"wave {how}/counted" if counted else f"wave sorted ({how})"
    return routes


def _describe_mismatch(got, want, arriving, boff, shift, fmt, mode, label):
    bad = int(np.flatnonzero(got != want)[0])
    b = int(np.searchsorted(boff, bad, side="right")) - 1
    a, z = int(boff[b]), int(boff[b + 1])
    s = fields(arriving[a:z], fmt)[0] & ((1 << shift) - 1)
    kind = "a permutation in the wrong order" if np.array_equal(np.sort(got[a:z]), np.sort(want[a:z])) else "NOT a permutation"
    return (f"{label}: format {fmt}, bucket_shift {shift}, mode {mode}: first difference in bucket {b} (rows {a} .. {z}, {z - a} rows, "
            f"turn {b // TURN}), {kind}; predicted route: {predict_routes(arriving, boff, shift, fmt, mode)[b]}; rows per start: "
            f"{np.bincount(s, minlength=1 << shift).tolist()}")


def assert_words(got, want, arriving, boff, shift, fmt, mode, label):
    if not np.array_equal(got, want):
        msg = _describe_mismatch(got, want, arriving, boff, shift, fmt, mode, label)
        print(msg)
        pytest.fail(msg)


# =====================================================================================================================
# recipes
# =====================================================================================================================
class _Rows:
    """host rows bucket by bucket; the rows of a bucket keep the order they are given in (sorted by start, stable)"""

    def __init__(self, fmt, shift, seed):
        self.fmt, self.shift, self.rng = fmt, shift, np.random.default_rng(seed)
        self.parts = {}

    def _lens(self, n):
        rng = self.rng
        lens = rng.integers(0, 70, n)
        wide = rng.random(n) < 0.25
        lens[wide] = rng.integers(0, 256, int(wide.sum()))
        far = rng.random(n) < 0.08
        lens[far] = rng.integers(255, 600, int(far.sum()))             # end - start >= 255: the overlap byte saturates
        return lens

    def _annots(self, n):
        return self.rng.integers(1, MAX_ANNOT[self.fmt] + 1, n)

    def _put(self, bucket, s, lens, annots):
        assert bucket not in self.parts, bucket
        self.parts[bucket] = ((bucket << self.shift) + np.asarray(s, np.int64), np.asarray(lens, np.int64), np.asarray(annots, np.int64))

    def by_start(self, bucket, counts):
        """counts[s] rows on start s, their (overlap, annot) in random order"""
        counts = np.asarray(counts, np.int64)
        assert len(counts) == 1 << self.shift
        n = int(counts.sum())
        if n:
            self._put(bucket, np.repeat(np.arange(len(counts)), counts), self._lens(n), self._annots(n))

    def by_residue(self, bucket, class_counts):
        """class_counts[c] rows of annot mod 32 == c, arriving grouped by c (starts rising along them), shuffled inside a class"""
        class_counts = np.asarray(class_counts, np.int64)
        n = int(class_counts.sum())
        res = np.repeat(np.arange(32), class_counts)
        annots = res + 32 * self.rng.integers(1 if self.fmt == 12 else 0, (MAX_ANNOT[self.fmt] + 1) // 32, n)
        annots[annots == 0] = 32
        self._put(bucket, np.sort(self.rng.integers(0, 1 << self.shift, n)), self._lens(n), annots)

    def columns(self):
        order = sorted(self.parts)
        s = np.concatenate([self.parts[b][0] for b in order])
        lens = np.concatenate([self.parts[b][1] for b in order])
        o = np.concatenate([self.parts[b][2] for b in order])
        o[0], o[-1] = MAX_ANNOT[self.fmt], 1 + MAX_ANNOT[self.fmt] // 2       # (the format follows from the largest annot)
        assert np.all(np.diff(s) >= 0)
        return s, s + lens, o


def _spread(rng, total, cap, starts=32, skip=()):
    """`total` rows over the starts at random, at most `cap` on one"""
    free = np.array([x for x in range(starts) if x not in skip])
    assert total <= cap * len(free), (total, cap)
    c = np.zeros(starts, np.int64)
    c[free] = rng.multinomial(total, np.full(len(free), 1.0 / len(free)))
    while c.max() > cap:
        i = int(c.argmax())
        j = free[int(c[free].argmin())]
        c[i] -= 1
        c[j] += 1
    return c


def _one_long(rng, longest, total=None, cap=5, starts=32):
    """one start of `longest` rows beside short ones (`total` rows in all; default: a few starts of 1 .. 5)"""
    at = int(rng.integers(0, starts))
    if total is None:
        c = np.zeros(starts, np.int64)
        others = [x for x in rng.permutation(starts) if x != at][:5]
        c[others] = rng.integers(1, 6, len(others))
    else:
        c = _spread(rng, total - longest, cap, starts, skip=(at,))
    c[at] = longest
    return c


def _turns(rng, which):
    """[(name, [eight bucket specs])]: a spec is None (empty), ("s", per-start counts) or ("r", counts per annot mod 32: _one_long
    serves for both, a class being a start or a residue)"""
    S = lambda c: ("s", c)
    lane = lambda: S(rng.integers(0, LANE_ROWS + 1, 32))
    one = lambda: S(np.bincount([int(rng.integers(0, 32))], minlength=32))
    full = S(np.full(32, LANE_ROWS))
    low4 = lambda total: S(_spread(rng, total, 4))
    nine = rng.integers(0, LANE_ROWS + 1, 32)
    nine[int(rng.integers(0, 32))] = LANE_ROWS + 1
    small = [
        ("lane pairs", [lane(), lane(), full, full, None, lane(), lane(), None]),
        ("lane edges", [one(), None, one(), S(_spread(rng, 200, LANE_ROWS)), one(), S(_one_long(rng, 20, 200, LANE_ROWS)), S(nine), lane()]),
        ("at most four", [low4(100), low4(128), low4(37), low4(2), low4(64), low4(5), low4(90), low4(120)]),
        ("class lengths", [S(_one_long(rng, n)) for n in (9, 63, 64, 65, 95, 96, 97, 200)]),
        ("bucket sizes", [S(_one_long(rng, 256, 256))] + [S(_one_long(rng, min(12, n // 2 + 1) if n > 2 else 1, n, LANE_ROWS))
                                                          for n in (2, 63, 64, 65, 127, 128, 129)]),
        ("residues", [S(_one_long(rng, 16, 255, LANE_ROWS)), S(_one_long(rng, 16, 256, LANE_ROWS))] +
         [("r", _one_long(rng, n)) for n in (9, 63, 64, 65, 95, 96)]),
        ("residues 2", [("r", _one_long(rng, 97)), ("r", _one_long(rng, 200)), lane(), low4(50), S(_one_long(rng, 30)), one(), None,
                        S(_one_long(rng, 70))]),
    ]
    if which == "small":
        return small
    large = [
        ("block sizes", [S(_spread(rng, n, 40)) for n in (257, 511, 512, 513)] + [S(_spread(rng, n, 400)) for n in (4096, 4097, 8191, 8192)]),
        ("block classes", [S(_spread(rng, BLOCK_ROWS + 1, 400)), S(_one_long(rng, COUNTED_ROWS, 600, 60)), S(_one_long(rng, COUNTED_ROWS + 1, 600, 60)),
                           S(_one_long(rng, BLOCK_ROWS, BLOCK_ROWS)), ("r", _one_long(rng, COUNTED_ROWS, 700, 60)),
                           ("r", _one_long(rng, COUNTED_ROWS + 1, 700, 60)), None, low4(2)]),
        ("one large", [S(_spread(rng, WAVE_ROWS + 1, 20)), None, one(), low4(2), low4(3), None, low4(5), one()]),
    ]
    return small + large


class _Index:
    """one recipe index on the host: columns, the words and table memo_index_pack must write, who sits where"""


_INDEXES = {}


def recipe_index(fmt, which="full"):
    key = (fmt, which)
    if key in _INDEXES:
        return _INDEXES[key]
    seed = 1000 * fmt + (7 if which == "small" else 0)
    R = _Rows(fmt, 5, seed)
    rng = R.rng
    turns = _turns(rng, which)
    ix = _Index()
    ix.fmt, ix.shift, ix.n_docs, ix.where = fmt, 5, N_DOCS[fmt], {}
    turn = 1
    for i, (name, specs) in enumerate(turns):
        if i == 3:
            turn = WRAP_TURN[fmt] - 3                                   # three turns below the wrap of the start field, the rest past it
        assert len(specs) == TURN
        for j, spec in enumerate(specs):
            ix.where[turn * TURN + j] = name
            if spec is not None:
                (R.by_start if spec[0] == "s" else R.by_residue)(turn * TURN + j, spec[1])
        turn += 1
    # the tail: the table has (last bucket + 2) buckets -- six buckets here leave a last turn of seven; the small index ends on
    # the eighth bucket of its turn, so that the empty bucket behind it is a turn of one
    tail = 6 if which == "full" else TURN
    for j in range(tail):
        ix.where[turn * TURN + j] = "tail"
        R.by_start(turn * TURN + j, rng.integers(1, LANE_ROWS + 1, 32) if j % 3 else _one_long(rng, 30))
    ix.s, ix.e, ix.o = R.columns()
    ix.words0 = pack_words(ix.s, ix.e, ix.o, fmt)
    ix.boff = bucket_table(ix.s, 5)
    assert (len(ix.boff) - 1) % TURN == (7 if which == "full" else 1)
    assert len(ix.s) < 100_000
    _INDEXES[key] = ix
    return ix


WALK = (2, 1, 3, 1, 4, 2, 3, 2, 4, 3, 4, 1)          # from order 1: all twelve ordered pairs of the four orders

FROM_START = {1: {"lane_pair", "wave table/counted", "wave loop/counted", "wave sorted (loop)", "block counted", "block sorted", "untouched"},
              3: {"wave table/counted", "wave loop/counted", "wave sorted (table)", "wave sorted (loop)", "block counted", "block sorted",
                  "untouched"}}
FROM_START[2] = FROM_START[1]
# arriving dealt: chunks of four dealt over the classes come grouped by another class only where there is a single pass (at most four
# rows per start: lane_pair again between modes 1 and 2, mode 0's counted route on the way back), else they are sorted
DEALT = {0: {"wave mode-0 counted", "wave sorted", "block sorted", "untouched"},
         1: {"lane_pair", "wave sorted (table)", "wave sorted (loop)", "block sorted", "untouched"},
         2: {"lane_pair", "wave sorted (table)", "wave sorted (loop)", "block sorted", "untouched"},
         3: {"wave sorted (table)", "wave sorted (loop)", "block sorted", "untouched"}}

_COVERED = []


def _assert_route_coverage():
    """every named route is predicted for at least one recipe bucket, per format, per mode, from start order and from a dealt order"""
    if _COVERED:
        return
    for fmt in (4, 12):
        ix = recipe_index(fmt)
        for mode in (1, 2, 3):
            seen = set(predict_routes(ix.words0, ix.boff, 5, fmt, mode))
            assert FROM_START[mode] <= seen, (fmt, mode, sorted(FROM_START[mode] - seen))
        dealt = {m: set() for m in range(4)}
        have = 0
        for order in WALK:
            arriving = row_order_reference(ix.words0, ix.boff, 5, fmt, have)
            if have:
                dealt[order - 1] |= set(predict_routes(arriving, ix.boff, 5, fmt, order - 1))
            have = order - 1
        for mode in range(4):
            assert DEALT[mode] <= dealt[mode], (fmt, mode, sorted(DEALT[mode] - dealt[mode]))
        small = recipe_index(fmt, "small")
        for mode in (1, 2, 3):
            seen = set(predict_routes(small.words0, small.boff, 5, fmt, mode))
            assert not any(r.startswith("block") for r in seen) and (mode == 3 or "lane_pair" in seen), (fmt, mode)
    _COVERED.append(True)


def random_index(seed, fmt, shift, n_buckets, sizes=None):
    """buckets of random sizes (log-uniform in 0 .. 600 unless a list is given) with clumps of 1 .. 120 rows on single starts"""
    R = _Rows(fmt, shift, seed)
    rng = R.rng
    width = 1 << shift
    first = int(rng.integers(1, 200))
    for b in range(first, first + n_buckets):
        n = int(np.exp(rng.uniform(0, np.log(601)))) - 1 if sizes is None else int(sizes[int(rng.integers(0, len(sizes)))])
        counts = np.bincount(rng.integers(0, width, n), minlength=width)
        if rng.random() < 0.3:
            counts[int(rng.integers(0, width))] += int(rng.integers(1, 121))
        R.by_start(b, counts)
    ix = _Index()
    ix.fmt, ix.shift, ix.n_docs = fmt, shift, N_DOCS[fmt]
    ix.s, ix.e, ix.o = R.columns()
    ix.words0 = pack_words(ix.s, ix.e, ix.o, fmt)
    ix.boff = bucket_table(ix.s, shift)
    assert len(ix.s) < 100_000
    return ix


# =====================================================================================================================
# the reference and the recipes, on the CPU
# =====================================================================================================================
def _word(fmt, start, ov, annot):
    s = np.array([start]), np.array([start + ov]), np.array([annot])
    return int(pack_words(*s, fmt)[0])


@pytest.mark.parametrize("fmt", [4, 12])
@pytest.mark.parametrize("mode", [1, 2])
def test_reference_on_a_bucket_written_out(fmt, mode):
    """starts a < b < c with 6, 1 and 5 rows: a0 a1 a2 a3 b0 c0 c1 c2 c3 a4 a5 c4"""
    base = 7 * 32 + (1 << 16)                          # bucket 2055: the start field of both formats has wrapped
    a, b, c = base + 3, base + 4, base + 31
    rows = {"a": [_word(fmt, a, ov, 9) for ov in (0, 1, 2, 3, 4, 5)], "b": [_word(fmt, b, 7, 200)],
            "c": [_word(fmt, c, ov, 77) for ov in (0, 1, 2, 3, 4)]}
    want = [rows[x[0]][int(x[1])] for x in "a0 a1 a2 a3 b0 c0 c1 c2 c3 a4 a5 c4".split()]
    arriving = rows["a"][::-1] + rows["b"] + [rows["c"][i] for i in (3, 0, 4, 1, 2)]
    boff = np.zeros((base >> 5) + 3, np.int64)
    boff[(base >> 5) + 1:] = 12
    got = row_order_reference(np.array(arriving, np.uint32), boff, 5, fmt, mode)
    assert got.tolist() == want
    back = row_order_reference(got, boff, 5, fmt, 0)
    assert back.tolist() == rows["a"] + rows["b"] + rows["c"]


@pytest.mark.parametrize("fmt", [4, 12])
def test_reference_on_a_membership_bucket_written_out(fmt):
    """mode 3: classes of annot mod 32, inside a class by the row's end in the bucket (s + ov), then annot, then s"""
    base = 64
    x = [_word(fmt, base + s, ov, annot) for s, ov, annot in ((9, 0, 33), (1, 9, 1), (0, 10, 65), (2, 8, 1), (0, 200, 1), (30, 255, 97))]
    #   residue 1, by (s + ov, annot, s): (1,9,1)=10,1,1  (2,8,1)=10,1,2  (9,0,33)=9 first ...
    cls1 = [x[0], x[1], x[3], x[2], x[4], x[5]]        # ends 9, 10 (annot 1, s 1), 10 (annot 1, s 2), 10 (annot 65), 200, 285
    y = [_word(fmt, base + s, ov, annot) for s, ov, annot in ((5, 5, 64), (31, 0, 32))]     # residue 0: ends 10, 31
    z = [_word(fmt, base + 4, 1, 31)]                                                       # residue 31
    arriving = [x[2], x[4], x[1], x[3], z[0], y[0], x[0], x[5], y[1]]
    boff = np.array([0, 0, 0, 9, 9], np.int64)
    got = row_order_reference(np.array(arriving, np.uint32), boff, 5, fmt, 3)
    #   chunk 0: residue 0 (two rows), residue 1 (four), residue 31 (one); chunk 1: residue 1's last two
    assert got.tolist() == y + cls1[:4] + z + cls1[4:]
    # on another bucket width the membership order is mode 2
    boff6 = np.array([0, 0, 9, 9], np.int64)
    assert np.array_equal(row_order_reference(np.array(arriving, np.uint32), boff6, 6, fmt, 3),
                          row_order_reference(np.array(arriving, np.uint32), boff6, 6, fmt, 2))


@pytest.mark.parametrize("fmt", [4, 12])
def test_reference_mode_2_on_overlaps_that_differ_above_bit_5(fmt):
    """one start: overlaps 40, 5, 37, 69, 8 -- mode 1 by overlap; mode 2 by overlap mod 32 first (5, 37, 69 | 8, 40)"""
    base = 32 * 3
    w = {ov: _word(fmt, base + 2, ov, 3) for ov in (40, 5, 37, 69, 8)}
    other = _word(fmt, base + 1, 255, 4)
    arriving = np.array([other] + [w[ov] for ov in (40, 5, 37, 69, 8)], np.uint32)
    boff = np.array([0, 0, 0, 0, 6, 6], np.int64)
    assert row_order_reference(arriving, boff, 5, fmt, 1).tolist() == [other] + [w[ov] for ov in (5, 8, 37, 40)] + [w[69]]
    assert row_order_reference(arriving, boff, 5, fmt, 2).tolist() == [other] + [w[ov] for ov in (5, 37, 69, 8)] + [w[40]]


@pytest.mark.parametrize("fmt,shift", [(4, 5), (12, 5), (4, 3), (12, 6), (4, 8), (12, 1)])
def test_reference_is_a_permutation_idempotent_and_comes_back_sorted(fmt, shift):
    ix = random_index(77 + shift, fmt, shift, 60, sizes=None if shift == 5 else (0, 1, 2, 3, 20, 100, 300))
    bucket, sizes = _bucket_of_rows(ix.boff)
    start, ov, annot = fields(ix.words0, fmt)
    key0 = (bucket << 40) | ((start & ((1 << shift) - 1)) << 20) | (ov << 12) | annot
    for mode in range(4):
        out = row_order_reference(ix.words0, ix.boff, shift, fmt, mode)
        for b in np.flatnonzero(sizes)[::7]:                                                     # a permutation, bucket by bucket
            assert np.array_equal(np.sort(out[ix.boff[b]:ix.boff[b + 1]]), np.sort(ix.words0[ix.boff[b]:ix.boff[b + 1]]))
        assert np.array_equal(np.sort(out.astype(np.int64) | (bucket << 40)), np.sort(ix.words0.astype(np.int64) | (bucket << 40)))
        assert np.array_equal(row_order_reference(out, ix.boff, shift, fmt, mode), out)          # idempotent
        for other in range(4):                                                                   # a function of the bucket's rows alone
            assert np.array_equal(row_order_reference(row_order_reference(ix.words0, ix.boff, shift, fmt, other), ix.boff, shift, fmt, mode), out)
        back = row_order_reference(out, ix.boff, shift, fmt, 0)
        assert np.array_equal(back, ix.words0[np.argsort(key0, kind="stable")])                 # mode 0 after any mode: sorted


def test_recipes_reach_every_route_and_cover_every_value():
    _assert_route_coverage()
    for fmt in (4, 12):
        for which in ("full", "small"):
            ix = recipe_index(fmt, which)
            start, ov, annot = fields(ix.words0, fmt)
            assert which == "small" or set(ov.tolist()) == set(range(256))                        # every overlap byte, 255 included
            assert set((ov & 31).tolist()) == set(range(32)) and set((annot & 31).tolist()) == set(range(32))
            assert int((ix.e - ix.s).max()) > 255 and int(annot.max()) == MAX_ANNOT[fmt]
            assert (int(annot.max()) > 255) == (fmt == 12)
            buckets = np.flatnonzero(np.diff(ix.boff))
            wrap = (1 << 16 if fmt == 4 else 1 << 12) >> 5
            assert buckets.min() < wrap - 8 and (buckets >= wrap).sum() > 8                       # on both sides of the wrap, and past it
            sizes = np.diff(ix.boff)
            if which == "full":
                assert {257, 511, 512, 513, 4096, 4097, 8191, 8192, 8193} <= set(sizes.tolist())
            assert {2, 63, 64, 65, 127, 128, 129, 255, 256} <= set(sizes.tolist())
            # a turn of eight small buckets; a turn with one bucket of 257 rows beside 0, 1, 2 and 3
            per_turn = np.pad(sizes, (0, -len(sizes) % TURN)).reshape(-1, TURN)
            assert any(0 < r.min() and r.max() <= WAVE_ROWS for r in per_turn)
            if which == "full":
                assert any(r.max() == WAVE_ROWS + 1 and {0, 1, 2, 3} <= set(r.tolist()) for r in per_turn)
    # the small index has no large turn at all, the full one both kinds
    assert np.diff(recipe_index(4, "small").boff).max() <= WAVE_ROWS < np.diff(recipe_index(4).boff).max()


def test_route_prediction_on_buckets_written_out():
    """the thresholds, one bucket each side of each"""
    rng = np.random.default_rng(5)

    def route(counts, mode, neighbour=None, turn_mate=None):
        R = _Rows(4, 5, 11)
        R.by_start(8, counts)
        if neighbour is not None:
            R.by_start(9, neighbour)
        if turn_mate is not None:
            R.by_start(12, turn_mate)
        s, e, o = R.columns()
        return predict_routes(pack_words(s, e, o, 4), bucket_table(s, 5), 5, 4, mode)[8]

    eight, nine = np.full(32, 8), np.r_[np.full(31, 7), 9]
    assert route(eight, 2) == "lane_pair" and route(nine, 2) == "wave table/counted" and route(eight, 2, neighbour=nine) == "wave table/counted"
    assert route(eight, 3) == "wave sorted (table)" and route(eight, 0) == "wave mode-0 counted"
    assert route(_one_long(rng, 64), 1) == "wave table/counted" and route(_one_long(rng, 65), 1) == "wave loop/counted"
    assert route(_one_long(rng, 96), 1) == "wave loop/counted" and route(_one_long(rng, 97), 1) == "wave sorted (loop)"
    assert route(_one_long(rng, 256, 256), 2) == "wave sorted (loop)" and route(_spread(rng, 257, 20), 2) == "block counted"
    assert route(eight, 2, turn_mate=_spread(rng, 257, 20)) == "block counted"
    assert route(_one_long(rng, 97, 300, 20), 2) == "block sorted" and route(_one_long(rng, 96, 300, 20), 2) == "block counted"
    assert route(_spread(rng, 8192, 400), 2) == "block sorted" and route(_spread(rng, 8193, 400), 2) == "untouched"
    assert route(np.bincount([3], minlength=32), 2) == "untouched"
    assert route(np.bincount([3], minlength=32), 2, neighbour=np.bincount([3], minlength=32)) == "lane_pair"


# =====================================================================================================================
# on the GPU
# =====================================================================================================================
@pytest.fixture(scope="module")
def memo():
    _assert_route_coverage()                            # before any device call
    import memo_amd
    from memo_amd import _lib
    memo_amd.build()
    assert _lib.lib().memo_device_count() > 0, "no HIP device: the product has no CPU fallback"
    return memo_amd


@pytest.fixture
def ab(memo):
    """the A/B library (product objects + memo_debug.o): memo_debug_row_order"""
    from memo_amd import _lib
    _lib.use_ab(True)
    yield _lib
    _lib.use_ab(False)


def _export(ix):
    """(packed words, 16-bit annots, bucket table) of a packed index (memo_index_export_packed)"""
    from memo_amd import _lib
    inf = ix.info()
    assert inf["long_rows"] == 0
    pk = np.empty(inf["rows"], np.uint32)
    pa = np.empty(inf["rows"] if inf["packed_format"] == 6 else 0, np.uint16)
    boff = np.empty(inf["buckets"], np.int64)
    _lib.check(_lib.lib().memo_index_export_packed(ix._h, pk.ctypes.data, pa.ctypes.data if pa.size else None, boff.ctypes.data, None))
    return pk, pa, boff


def _packed_in_start_order(memo, h):
    """the host index on the device, packed under order 1; its words and table are the host's own"""
    ix = memo.DeviceIndex.from_host(h.s, h.e, h.o, bucket_shift=h.shift)
    try:
        ix.debug_row_order(1)
        ix.pack(keep_wide=False)
        inf = ix.info()
        assert inf["packed_format"] == h.fmt and inf["row_order"] == 0 and inf["bucket_shift"] == h.shift
        words, _, boff = _export(ix)
        assert np.array_equal(boff, h.boff)
        assert np.array_equal(words, h.words0)
    except BaseException:
        ix.close()
        raise
    return ix


def _recorded(h, order):
    return 2 if order == 4 and h.shift != 5 else order - 1


_WANT = {}


def _oracle_windows(oracle, h, key):
    """[(kind, qs, qe, k, expected)]: one conservation and one membership window over the recipe buckets, k = 31 and 101; computed once"""
    if key not in _WANT:
        used = np.flatnonzero(np.diff(h.boff))
        lo = int(used[used >= (WRAP_TURN[h.fmt] - 3) * TURN].min()) << h.shift
        hi = (int(used.max()) + 1) << h.shift
        out = []
        for k in (31, 101):
            qs, qe = max(int(h.s[0]) - 40, 0), hi + 300
            out.append(("c", qs, qe, k, oracle.conservation(*oracle.filter_rows(h.s, h.e, h.o, qs, qe, k), qs, qe, k, h.n_docs, literal=False)))
            qs, qe = lo - 50, hi + 120
            out.append(("m", qs, qe, k, oracle.membership(*oracle.filter_rows(h.s, h.e, h.o, qs, qe, k), qs, qe, k, h.n_docs, literal=False)))
        _WANT[key] = out
    return _WANT[key]


def _check_windows(ix, h, windows, label):
    for kind, qs, qe, k, want in windows:
        got = ix.conservation(qs, qe, k, h.n_docs) if kind == "c" else ix.membership(qs, qe, k, h.n_docs)
        assert np.array_equal(got, want), (label, kind, qs, qe, k)


@pytest.mark.gpu
@pytest.mark.parametrize("order", [2, 3, 4])
@pytest.mark.parametrize("which", ["full", "small"])
@pytest.mark.parametrize("fmt", [4, 12])
def test_from_start_order(fmt, which, order, memo, ab):
    """rows grouped by start, as memo_index_pack writes them, into each dealt order: lane_pair and the counted routes"""
    h = recipe_index(fmt, which)
    with _packed_in_start_order(memo, h) as ix:
        ix.debug_row_order(order)
        assert ix.info()["row_order"] == order - 1
        words, _, boff = _export(ix)
        assert np.array_equal(boff, h.boff)
        assert_words(words, row_order_reference(h.words0, h.boff, 5, fmt, order - 1), h.words0, h.boff, 5, fmt, order - 1,
                     f"{which} index, start order -> order {order}")


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [4, 12])
def test_from_every_order_to_every_other(fmt, memo, ab):
    """1 -> 2 -> 1 -> 3 -> 1 -> 4 -> 2 -> 3 -> 2 -> 4 -> 3 -> 4 -> 1: after every step the words are the reference of the ORIGINAL words"""
    h = recipe_index(fmt)
    with _packed_in_start_order(memo, h) as ix:
        have = h.words0
        was = 1
        for order in WALK:
            ix.debug_row_order(order)
            assert ix.info()["row_order"] == order - 1
            words, _, boff = _export(ix)
            assert np.array_equal(boff, h.boff)
            assert_words(words, row_order_reference(h.words0, h.boff, 5, fmt, order - 1), have, h.boff, 5, fmt, order - 1,
                         f"order {was} -> {order}")
            ix.debug_row_order(order)                                   # asking twice changes nothing
            again, _, boff = _export(ix)
            assert np.array_equal(again, words) and np.array_equal(boff, h.boff) and ix.info()["row_order"] == order - 1
            have, was = words, order
        # back in start order: every bucket the pass touches is sorted by (start, overlap, annot)
        bucket, sizes = _bucket_of_rows(h.boff)
        start, ov, annot = fields(have, fmt)
        key = ((start & 31) << 20) | (ov << 12) | annot
        falls = (bucket[1:] == bucket[:-1]) & (key[1:] < key[:-1])
        assert set(sizes[bucket[1:][falls]].tolist()) <= {BLOCK_ROWS + 1}
        assert np.array_equal(np.sort(have.astype(np.int64) | (bucket << 40)), np.sort(h.words0.astype(np.int64) | (bucket << 40)))


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [4, 12])
def test_results_in_every_order(fmt, memo, oracle, ab):
    """one conservation and one membership window over the recipe buckets, k = 31 and 101, in each of the four orders -- with views (the first
    query of a class builds its view, ordered like the rows; the second reads it)"""
    h = recipe_index(fmt)
    windows = _oracle_windows(oracle, h, fmt)
    with _packed_in_start_order(memo, h) as ix:
        ix.set_option(OPT_BUILD_COST_PCT, 0)
        _check_windows(ix, h, windows, (fmt, "as packed"))
        assert np.array_equal(_export(ix)[0], h.words0)
        for order in (2, 3, 4, 1):                                     # (start order last: sorted by the pass, not as packed)
            ix.debug_row_order(order)
            assert ix.info()["row_order"] == order - 1
            for rep in range(2):
                _check_windows(ix, h, windows, (fmt, order, rep))
            assert ix.info()["row_order"] == order - 1                  # (an order asked for by name stays)
            assert_words(_export(ix)[0], row_order_reference(h.words0, h.boff, 5, fmt, order - 1), h.words0, h.boff, 5, fmt, order - 1,
                         f"after the queries in order {order}")


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [4, 12])
def test_plain_pack_leaves_the_conservation_order(fmt, memo):
    """the product's own route: memo_index_pack runs the pass in mode 2 on the pack's stream"""
    h = recipe_index(fmt)
    with memo.DeviceIndex.from_host(h.s, h.e, h.o) as ix:
        ix.pack(keep_wide=True)
        inf = ix.info()
        assert inf["packed_format"] == fmt and inf["row_order"] == 2 and inf["bucket_shift"] == 5
        words, _, boff = _export(ix)
        assert np.array_equal(boff, h.boff)
        assert_words(words, row_order_reference(h.words0, h.boff, 5, fmt, 2), h.words0, h.boff, 5, fmt, 2, "memo_index_pack")


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [4, 12])
def test_builder_rows_are_ordered_by_the_queries_that_pay(fmt, memo, oracle):
    """memo_builder_* leaves start order; with MEMO_OPT_BUILD_COST_PCT 0 the first conservation query orders a COPY of the rows for
    conservation (order_words_on, mode 2), a later membership query for membership (mode 3)"""
    h = recipe_index(fmt)
    windows = _oracle_windows(oracle, h, fmt)
    with memo.IndexBuilder(len(h.s) + 100) as b:
        b.push(h.s, h.e, h.o)
        with b.finish() as ix:
            inf = ix.info()
            assert inf["packed_format"] == fmt and inf["row_order"] == 0 and inf["has_wide"] == 0
            before, _, boff = _export(ix)
            assert np.array_equal(boff, h.boff) and np.array_equal(before, h.words0)
            ix.set_option(OPT_BUILD_COST_PCT, 0)
            _check_windows(ix, h, [w for w in windows if w[0] == "c"][:1], (fmt, "first conservation query"))
            assert ix.info()["row_order"] == 2
            words, _, boff = _export(ix)
            assert np.array_equal(boff, h.boff)
            assert_words(words, row_order_reference(before, h.boff, 5, fmt, 2), before, h.boff, 5, fmt, 2, "builder, conservation query")
            _check_windows(ix, h, [w for w in windows if w[0] == "m"][:1], (fmt, "membership query"))
            assert ix.info()["row_order"] == 3
            arriving = words
            words, _, boff = _export(ix)
            assert np.array_equal(boff, h.boff)
            assert_words(words, row_order_reference(before, h.boff, 5, fmt, 3), arriving, h.boff, 5, fmt, 3, "builder, membership query")
            _check_windows(ix, h, windows, (fmt, "every window, membership order"))


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [1, 3, 6, 8])
@pytest.mark.parametrize("fmt", [4, 12])
def test_other_bucket_widths_take_the_block_route(fmt, shift, memo, ab):
    """bucket widths other than 32: block_bucket for every bucket; the membership order is recorded, and is, mode 2"""
    h = random_index(300 + 10 * shift + fmt, fmt, shift, 48, sizes=(0, 1, 2, 3, 20, 100, 257, 300, 1000, 3000, BLOCK_ROWS + 7))
    for mode in range(4):
        assert {r.split()[0] for r in predict_routes(h.words0, h.boff, shift, fmt, mode)} == {"block", "untouched"}
    with _packed_in_start_order(memo, h) as ix:
        have = h.words0
        for order in (2, 1, 3, 1, 4, 3, 4, 2, 1):
            ix.debug_row_order(order)
            mode = _recorded(h, order)
            assert ix.info()["row_order"] == mode
            words, _, boff = _export(ix)
            assert np.array_equal(boff, h.boff)
            assert_words(words, row_order_reference(h.words0, h.boff, shift, fmt, order - 1), have, h.boff, shift, fmt, mode, f"-> order {order}")
            have = words


@pytest.mark.gpu
@pytest.mark.parametrize("fmt,shift", [(4, 3), (12, 8), (4, 5), (12, 5)])
def test_pack_under_the_membership_order(fmt, shift, memo, ab):
    """memo_index_pack with order 4 asked for beforehand: the pass runs inside the pack; on a bucket width other than 32 the words are in
    mode 2 and row_order says so (it said 3 until this test: memo_index_pack recorded the order asked for, not the one applied)"""
    h = recipe_index(fmt, "small") if shift == 5 else random_index(500 + shift, fmt, shift, 30, sizes=(0, 1, 2, 3, 20, 100, 300, 1000))
    mode = 3 if shift == 5 else 2
    with memo.DeviceIndex.from_host(h.s, h.e, h.o, bucket_shift=shift) as ix:
        ix.debug_row_order(4)
        ix.pack(keep_wide=False)
        assert ix.info()["packed_format"] == fmt
        words, _, boff = _export(ix)
        assert np.array_equal(boff, h.boff)
        assert_words(words, row_order_reference(h.words0, h.boff, shift, fmt, mode), h.words0, h.boff, shift, fmt, mode, "packed under order 4")
        assert ix.info()["row_order"] == mode
        ix.debug_row_order(4)                                           # already there: nothing moves
        assert np.array_equal(_export(ix)[0], words) and ix.info()["row_order"] == mode


@pytest.mark.gpu
def test_six_byte_rows_are_left_alone(memo, ab):
    """format 6 (one annot above 4095): every order asked for leaves the words, the annots and row_order 0"""
    h = random_index(66, 12, 5, 40)
    o = h.o.copy()
    o[len(o) // 2] = 5000
    with memo.DeviceIndex.from_host(h.s, h.e, o) as ix:
        ix.debug_row_order(1)
        ix.pack(keep_wide=False)
        assert ix.info()["packed_format"] == 6 and ix.info()["row_order"] == 0
        words0, annots0, boff0 = _export(ix)
        assert np.array_equal(annots0, o.astype(np.uint16)) and np.array_equal(boff0, h.boff)
        for order in (2, 3, 4, 0, 1):
            ix.debug_row_order(order)
            assert ix.info()["row_order"] == 0
            words, annots, boff = _export(ix)
            assert np.array_equal(words, words0) and np.array_equal(annots, annots0) and np.array_equal(boff, boff0)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [4, 12])
def test_random_buckets(fmt, memo, ab):
    """a few hundred buckets, sizes log-uniform in 0 .. 600, clumps of 1 .. 120 rows on single starts: orders 2, 3, 4, each from start order
    and from the order before"""
    h = random_index(4242 + fmt, fmt, 5, 300)
    with _packed_in_start_order(memo, h) as ix:
        have = h.words0
        for order in (2, 1, 3, 1, 4, 2, 4, 3):
            ix.debug_row_order(order)
            assert ix.info()["row_order"] == order - 1
            words, _, boff = _export(ix)
            assert np.array_equal(boff, h.boff)
            assert_words(words, row_order_reference(h.words0, h.boff, 5, fmt, order - 1), have, h.boff, 5, fmt, order - 1, f"random, -> order {order}")
            have = words
