"""Lives of an index, drawn from a seed: the case generator of the sweep fuzz (tests/fuzz_gpu.py: time-boxed, clock seed;
tests/test_sweep_lives_gpu.py: fixed seed, fixed count, inside the suite; tests/test_sweep_lives_cpu.py: the generator itself).

A LIFE is an index description plus a list of steps.  life(rng) draws one WITHOUT touching a GPU: random indexes (density, clumping,
annots, overlaps incl. end < start), the way in (int64 columns, the packed builder in ragged pieces, dense rows alone), row formats,
row orders, memo_index_prepare, and then between twelve and some twenty-five queries -- conservation as uint16 or uint8, membership,
membership slices, the one-shot host forms -- with random windows, k, tile shapes, membership algorithms, row sources, scatters (incl.
the chain and pair bits of the wide tiles), options (memo_index_set_option 1 and 3 .. 7) and up to three changes of the rows in
between (upload_rows, truncate, finalize on other buckets, pack again, pack_dense without the words, another row order).  The rows the
oracle reads are the ones the Python side holds after each change: desc["rows"][version].

run_life(memo, oracle, L) plays a life on the GPU and compares every answer with the oracle's, exactly.

Steps (tuples; every argument a plain int / bool / str / tuple of them, arrays by their number in desc):
    ("pack", keep_wide) ("pack_dense", keep_packed) ("row_order", order) ("switches", colouring, six_views)
    ("prepare", k, n_docs, membership, window_hint, may_refuse)
    ("option", option, value, previous)            previous: what memo_index_set_option must return
    ("tuning", tile_w, waves, membership_algo, row_source, scatter)
    ("query", form, version, qs, qe, k, n_docs, extra, may_refuse)
        form: "cons16" "cons8" "memb" | "slice" (extra = (slice_qs, slice_qe)) | "oneshot_cons" "oneshot_memb" (extra = the way)
    ("upload_rows", offset, fresh, version) ("truncate", rows, version) ("finalize", bucket_shift)
may_refuse: the index holds the dense rows alone and memo_dense_rows_can_answer says 0 for this query -- the only queries the library
may refuse (with one of REFUSALS), and the generator keeps them under 5 % of all queries."""
import hashlib

import numpy as np

SEED = 20261019
OPT_VIEWS, OPT_BUILD_COST_PCT, OPT_VIEW_ROWS, OPT_VIEW_PLACES, OPT_VIEW_LIVE, OPT_WIDE_TILES = 1, 3, 4, 5, 6, 7
OPTION_DEFAULTS = {OPT_VIEWS: 1, OPT_BUILD_COST_PCT: 100, OPT_VIEW_ROWS: 0, OPT_VIEW_PLACES: 1, OPT_VIEW_LIVE: 1, OPT_WIDE_TILES: 1}
OPTION_VALUES = {OPT_VIEWS: (0, 1, 1, 1), OPT_BUILD_COST_PCT: (0, 0, 0, 1, 100, 1000), OPT_VIEW_ROWS: (0, 5, 6, 6),
                 OPT_VIEW_PLACES: (0, 1), OPT_VIEW_LIVE: (0, 1), OPT_WIDE_TILES: (0, 1, 1)}
CHAIN_BITS = (256, 512, 1024, 2048)       # memo_debug_set_tuning, scatter: parts of the wide tiles' chain off; the pair kernel off
REFUSALS = ("this query needs the 4-byte rows or the int64 columns, which this index dropped",
            "this membership query needs the 4-byte rows or the int64 columns, which this index dropped")
MEMB_CELLS = 30_000_000                   # positions x genomes of a membership window, at most
# Directed modes: the conditions the launchers put on a pick (memo_sweep_cons.hip: query_conservation; memo_sweep_cons3t.hip:
# launch_halo3t; memo_view.hip: dense_rows_for), met on purpose where a uniform draw meets them by luck or never:
#   six      six-row views: bucket shift 5, k - 1 <= 31, annots and n_docs <= 255, a view that spares a fifth of the rows
#   r4       the wide tiles: k - 1 in 16 .. 31, a six-row view without flags, fewer than kR4MaxGroups = 543 groups per wide tile
#            (1568 positions: a view of under two rows per position), the chain bits drawn
#   pairs    fewer than kPairMaxGroups = 418 groups per pair of wide tiles (a view of under 0.8 rows per position), no chain bit
#   live     a placed view with a dead share of kLiveMinShare = 0.25 or more: few genomes, many rows per position
#   a9       256 .. 511 genomes on the dense rows
#   checked  an annot outside the matrix on the 4-byte rows
#   annot16  annots past 4095: the rows with a 16-bit order column (format 6), in and outside the matrix
#   shapes   the int64 columns / the 4-byte rows / the dense rows without a table under every forced tile width and wave count
DIRECTED = ("six", "r4", "pairs", "live", "a9", "checked", "annot16", "shapes")


def mode_of(i):
    """the directed mode of life i of a seeded run (None: the uniform draw): every third life, the modes in turn"""
    return DIRECTED[(i // 3) % len(DIRECTED)] if i % 3 == 2 else None


def seeded_life(seed, i, can_answer=None):
    return life(np.random.default_rng([seed, i]), mode_of(i), can_answer)


def _can_answer(rows, min_start, max_start, max_annot, k, n_docs, membership):
    from memo_amd.index import dense_rows_can_answer      # memo_dense_rows_can_answer: pure host arithmetic, no device
    return dense_rows_can_answer(rows, min_start, max_start, max_annot, k, n_docs, membership)


def _draw_rows(rng, length, m, mode, span):
    if mode == 0:
        s = rng.integers(1, length, m)
    elif mode == 1:
        s = rng.choice(rng.integers(1, length, max(int(rng.integers(1, 40)), 1)), m)
    elif mode == 2:
        s = rng.integers(-100, length + 1000, m)
    elif mode == 3:
        s = (rng.integers(1, max(length // 64, 2), m) * 64 + rng.integers(-1, 2, m))
    else:
        s = np.abs(rng.normal(length / 2, length / 20 + 1, m)).astype(np.int64) + 1
    s = np.sort(s).astype(np.int64)
    e = s + rng.integers(0, span, m)
    return s, e


def life(rng, directed=None, can_answer=None):
    """one life: (desc, steps).  Pure: the same rng state gives the same life; no GPU is touched (can_answer: memo_dense_rows_can_answer)"""
    can_answer = can_answer or _can_answer
    d = directed
    dense_family = d in ("six", "r4", "pairs", "live")
    n_docs = int(rng.choice([2, 5, 31, 32, 33, 64, 100, 255, 256, 257, 500, 511, 512, 1000]))
    length = int(rng.choice([100, 3000, 50_000, 400_000]))
    m = int(rng.integers(0, int(rng.choice([50, 5000, 200_000]))))
    mode = int(rng.integers(0, 5))
    span = int(rng.choice([2, 30, 70, 300, 3000]))
    if dense_family:
        n_docs = int(rng.choice([2, 2, 5] if d == "live" else [5, 31, 100, 255]))
        length = int(rng.choice([3000, 50_000]))
        lo, hi = {"six": (1.2, 6.0), "r4": (1.0, 1.6), "pairs": (1.0, 1.3), "live": (2.0, 4.0)}[d]
        m = min(int(length * rng.uniform(lo, hi)), 200_000)
        mode, span = 0, 70                                  # (overlaps below 70: a view of k - 1 <= 32 spares more than half the rows)
    elif d == "a9":
        n_docs = int(rng.choice([256, 257, 500, 511]))
        length = int(rng.choice([3000, 50_000]))
        m = min(int(length * rng.uniform(1.0, 5.0)), 200_000)
        mode, span = 0, int(rng.choice([30, 70]))
    elif d == "annot16":
        n_docs = int(rng.choice([70, 4096, 5000, 5000]))
        m = max(m, 40)
    elif d == "checked":
        m = max(m, 40)
    elif d == "shapes":
        n_docs = int(rng.choice([5, 100, 255, 256]))
        length = int(rng.choice([3000, 50_000]))
        m = min(int(length * rng.uniform(1.0, 4.0)), 200_000)
        mode = 0
    if d in ("checked", "annot16") and mode == 2:
        mode = 0                                            # (rows that can be packed: no negative start)
    s, e = _draw_rows(rng, length, m, mode, span)
    if rng.random() < 0.25 and m and not dense_family:
        neg = rng.random(m) < 0.02
        e[neg] = s[neg] - rng.integers(1, 2000, int(neg.sum()))
    hi_annot = n_docs if rng.random() < 0.9 else n_docs + 3          # sometimes outside the matrix
    if d == "checked":
        hi_annot = n_docs + 3
    elif d == "annot16":
        hi_annot = n_docs + int(rng.choice([0, 0, 3]))
    elif d in ("six", "r4", "pairs", "live", "a9", "shapes"):
        hi_annot = n_docs
    lo_annot = 0 if rng.random() < 0.1 else 1

    def draw_annots(count):
        return rng.integers(lo_annot, max(hi_annot, 2), count).astype(np.int64)
    o = draw_annots(m)
    if d in ("checked", "annot16") and m:
        o[int(rng.integers(0, m))] = hi_annot - 1                   # (the largest annot really occurs)
        if n_docs == 70:                                            # (a few annots of more than twelve bits, far outside the matrix)
            big = rng.random(m) < 0.03
            big[int(rng.integers(0, m))] = True
            o[big] = rng.integers(4096, 5003, int(big.sum()))
    bshift = int(rng.choice([0, 0, 0, 1, 3, 5, 6, 8]))
    if dense_family:
        bshift = 5
    packable = not (m and s.min() < 0)
    # a third of the packable indexes come in the packed, pinned way (memo_builder_*: host packer + bucket table
    # built on the host), in ragged pieces; the rest as int64 columns
    via_builder = packable and m > 0 and int(o.max()) <= 4095 and int(o.min()) >= 0 and rng.random() < 0.4
    # ... a third of those as DENSE rows straight from the host packer (five rows per 16 bytes; such an index answers k <= 64
    # only, may leave out the rows that can never write, and builds k-class views and tile tables behind its queries)
    dense_only = via_builder and int(o.max()) <= 511 and n_docs <= 511 and rng.random() < 0.35      # (annots of up to nine bits)
    if d in ("checked", "annot16", "shapes"):
        via_builder = dense_only = False
    if dense_family:
        dense_only = False
    cuts = ([0] + sorted(int(x) for x in rng.integers(0, m, int(rng.integers(0, 4)))) + [m]) if via_builder else []
    desc = dict(directed=d, n_docs=n_docs, length=length, m=m, mode=mode, bshift=bshift, via_builder=bool(via_builder),
                dense_only=bool(dense_only), cuts=cuts, extra=int(rng.integers(0, 100)) if via_builder else 0,
                rows=[(s, e, o)], fresh=[])
    steps = []
    # ---- what the generator knows of the index: enough to keep every step legal
    st = dict(ver=0, has_wide=not via_builder, words=bool(via_builder and not dense_only), dense=bool(dense_only), bshift=bshift,
              want_words=False, want_dense=False, opts=dict(OPTION_DEFAULTS))

    def cur():
        return desc["rows"][st["ver"]]

    def max_annot():
        return int(cur()[2].max()) if len(cur()[2]) else 0

    def can_pack():
        cs = cur()[0]
        return not (len(cs) and cs.min() < 0) and max_annot() <= 65535

    def dense_fits():                                       # (memo_index_pack_dense: format 4, or 12 with annots of nine bits)
        return st["words"] and max_annot() <= 511

    def build_up():                                         # the formats the life wants, as far as its rows allow
        if st["want_words"] and st["has_wide"] and can_pack():
            steps.append(("pack", True))
            st["words"], st["dense"] = True, False
        if st["want_dense"] and not st["dense"] and dense_fits():
            steps.append(("pack_dense", True))
            st["dense"] = True

    def set_option(opt, val):
        steps.append(("option", opt, int(val), st["opts"][opt]))
        st["opts"][opt] = int(val)

    if via_builder and not dense_only:
        st["want_words"] = True
        st["want_dense"] = dense_family or d == "a9" or rng.random() < 0.5
    elif not via_builder and (packable and rng.random() < 0.7 or d in ("checked", "annot16", "a9", "shapes") or dense_family):
        st["want_words"] = True
        st["want_dense"] = dense_family or d == "a9" or rng.random() < 0.6
    build_up()
    if rng.random() < 0.5:                                     # the order of the 4-byte rows inside their buckets (memo_interleave.hip):
        steps.append(("row_order", int(rng.integers(1, 5))))   #   start order, the two dealt orders, the membership order
    # the places of a dense view's rows inside their groups; which kind of dense view: the library's choice, five rows per group, six
    steps.append(("switches", int(rng.choice([0, 1, 1])) if d != "live" else 1,
                  int(rng.choice([-1, -1, 0, 1])) if not dense_family else int(rng.choice([-1, 1]))))
    k_pet = int(rng.choice([5, 9, 17, 31, 33, 101]))           # (asked often enough for its class's view to be built)
    if d in ("r4", "pairs"):
        k_pet = int(rng.choice([17, 21, 31, 32]))
    elif d in ("six", "live"):
        k_pet = int(rng.choice([3, 5, 9, 17, 31]))
    elif d == "a9" or dense_only:
        k_pet = int(rng.choice([5, 9, 17, 31, 33]))
    if rng.random() < 0.5 or dense_family:                     # views, placings and live copies really get built inside a life
        set_option(OPT_BUILD_COST_PCT, 0)
    if dense_family:
        set_option(OPT_VIEW_ROWS, 6)
        set_option(OPT_VIEW_PLACES, 0 if d in ("r4", "pairs") and rng.random() < 0.5 else 1)
        if d == "live":
            set_option(OPT_VIEW_LIVE, int(rng.choice([0, 0, 1])))

    def refusable(k, nd, memb):
        if not (st["dense"] and not st["words"] and not st["has_wide"]):
            return False
        cs, _, co = cur()
        return not can_answer(len(cs), int(cs[0]) if len(cs) else 0, int(cs[-1]) if len(cs) else -1, max_annot(), k, nd, memb)

    if rng.random() < 0.3 or d == "live":                      # memo_index_prepare: the view / tile table / row order before the first query
        memb = bool(rng.random() < 0.3) and d != "live"
        steps.append(("prepare", k_pet, n_docs, memb, int(rng.choice([0, 1000, length])), refusable(k_pet, n_docs, memb)))

    def draw_tuning():
        if dense_only or (dense_family and rng.random() < (0.9 if d == "r4" else 0.6)):
            # (dense rows alone: the tile shape and the scatter are the library's, so that its own predicate decides)
            scatter = 0
            if d == "r4" and rng.random() < 0.85:              # (every combination of the chain's parts and the pair kernel, evenly)
                scatter = 256 * int(rng.integers(0, 16))
            return (0, 0, 0, 0, scatter)
        t = (int(rng.choice([0, 256, 512, 1024, 2048, 4096, 1472, 1728])), int(rng.choice([0, 1, 4, 8])),
             int(rng.choice([0, 2, 3, 4])), int(rng.choice([0, 0, 0, 1, 2, 3, 5, 8, 9, 10, 13])), int(rng.integers(0, 6)))
        if d == "shapes":                                      # the row source and the scatter that keep one family under every shape
            src, sc = ((1, 1), (3, 1), (5, 0), (10, 2), (3, 2), (3, 3), (3, 5))[int(rng.integers(0, 7))]
            t = (int(rng.choice([0, 256, 512, 1024, 2048, 4096])), int(rng.choice([0, 1, 4, 8])), t[2], src, sc)
        if d == "a9" and rng.random() < 0.3:                   # (the dense rows without a tile table, under every wave count)
            t = (int(rng.choice([0, 0, 256, 512])), t[1], t[2], int(rng.choice([5, 10])), 0)
        if rng.random() < 0.3:
            t = t[:4] + (t[4] + int(sum(b for b in CHAIN_BITS if rng.random() < 0.4)),)
        return t

    def draw_query(k_classes):
        n = len(cur()[0])
        for attempt in range(64):
            kk = [1, 2, 3, 5, 8, 9, 16, 17, 21, 31, 32, 33, 64]
            only_dense = st["dense"] and not st["words"] and not st["has_wide"]
            if not only_dense:
                kk += [65, 80, 101, 128, 129, 255, 256]        # (a packed-only index answers k <= 256, dense rows k <= 64)
            if st["has_wide"]:
                kk += [257, 1000]
            k = k_classes if rng.random() < 0.45 or d in ("r4", "pairs", "live") and rng.random() < 0.7 else int(rng.choice(kk))
            qs = int(rng.integers(0, length))
            if rng.random() < 0.5:
                qs &= ~3                                       # (windows on the 4-position raster: aligned result stores)
            qe = int(rng.integers(qs, length + 200))
            if dense_family and rng.random() < 0.5:
                qs, qe = int(rng.integers(0, 64)), length + int(rng.integers(0, 64))     # (many tiles: the whole sequence)
            u = rng.random()
            extra = None
            # (a slice and its window agree on IndexError only where none can be raised: the membership matrix has n_docs columns)
            inside = max_annot() < n_docs
            if u < 0.35:
                form = "memb"
            elif u < 0.43 and inside:
                form = "slice"
            elif u < 0.50 and n:
                form = "oneshot_memb" if rng.random() < 0.4 else "oneshot_cons"
            else:
                form = "cons8" if n_docs <= 255 and rng.random() < 0.5 else "cons16"
            if d in ("r4", "pairs", "live", "six") and rng.random() < 0.6:
                form = "cons8" if rng.random() < 0.5 else "cons16"
            if form.startswith("oneshot"):                     # (its own index, whatever this one holds: any k)
                extra = int(rng.integers(0, 3))                # memo_debug_one_shot_way
                k = int(rng.choice([2, 9, 17, 31, 33, 64, 101, 256, 300])) if rng.random() < 0.5 else k
            if form in ("memb", "slice", "oneshot_memb") and (qe - qs) * n_docs > MEMB_CELLS:
                qe = qs + MEMB_CELLS // n_docs
            if form == "slice":
                if qe - qs < 3:
                    form = "memb"
                else:
                    way = int(rng.integers(0, 3))              # strictly inside, at the left edge, at the right edge
                    a = qs if way == 1 else int(rng.integers(qs + 1, qe - 1))
                    b = qe if way == 2 else int(rng.integers(a + 1, qe))
                    extra = (a, b)
            may = not form.startswith("oneshot") and refusable(k, n_docs, form in ("memb", "slice"))
            if may and attempt < 63 and rng.random() < 0.75:
                continue                                       # (three times out of four: drawn again)
            return ("query", form, st["ver"], qs, qe, k, n_docs, extra, bool(may))

    def change():
        cs, ce, co = cur()
        n = len(cs)
        legal = ["row_order"]
        if st["has_wide"] and n:
            legal += ["upload_rows", "truncate", "finalize"]
            if can_pack():
                legal.append("pack")
            if st["dense"] or dense_fits():
                legal.append("pack_dense")
        what = str(rng.choice(legal))
        if what == "row_order":
            steps.append(("row_order", int(rng.integers(1, 5))))
        elif what == "upload_rows":
            off = int(rng.integers(0, n))
            cnt = int(rng.integers(1, min(n - off, int(rng.choice([8, 1000, 200_000]))) + 1))
            fs = np.sort(rng.integers(cs[off], cs[off + cnt - 1] + 1, cnt)).astype(np.int64)
            fe = fs + rng.integers(0, span, cnt)
            fo = draw_annots(cnt)
            desc["fresh"].append((fs, fe, fo))
            desc["rows"].append(tuple(np.concatenate((old[:off], new, old[off + cnt:])) for old, new in zip(cur(), (fs, fe, fo))))
            st["ver"] = len(desc["rows"]) - 1
            steps.append(("upload_rows", off, len(desc["fresh"]) - 1, st["ver"]))
        elif what == "truncate":
            keep = int(rng.integers(max(1, n // 2), n + 1))
            desc["rows"].append(tuple(a[:keep].copy() for a in cur()))
            st["ver"] = len(desc["rows"]) - 1
            steps.append(("truncate", keep, st["ver"]))
        elif what == "finalize":
            st["bshift"] = int(rng.choice([b for b in (0, 1, 3, 5, 6, 8) if b != st["bshift"]]))
        elif what == "pack":
            st["want_words"] = True
        elif what == "pack_dense":
            if not st["dense"]:
                steps.append(("pack_dense", True))
            steps.append(("pack_dense", False))                # the words go; the int64 columns answer what the dense rows cannot
            st["dense"], st["words"] = True, False
            return
        if what in ("upload_rows", "truncate", "finalize"):    # (the rows changed: no words, no dense rows, no views; not finalized)
            steps.append(("finalize", st["bshift"]))
            st["words"] = st["dense"] = False
        if what != "row_order":
            build_up()

    n_changes = int(rng.choice([0, 0, 1, 2, 3])) if not dense_only else int(rng.choice([0, 1]))
    change_at = sorted(int(x) for x in rng.integers(1, 12, n_changes))
    for q in range(12):
        while change_at and change_at[0] == q:
            change_at.pop(0)
            change()
            for _ in range(3):                                 # ... then queries at a k class the index already had a view of
                steps.append(("tuning",) + draw_tuning())
                steps.append(draw_query(k_pet))
        if rng.random() < 0.25 and not dense_family:
            opt = int(rng.choice(list(OPTION_VALUES)))
            set_option(opt, rng.choice(OPTION_VALUES[opt]))
        if rng.random() < 0.15:
            steps.append(("switches", int(rng.choice([0, 1, 1])), int(rng.choice([-1, -1, 0, 1]))))
        steps.append(("tuning",) + draw_tuning())
        steps.append(draw_query(k_pet))
    return desc, steps


def queries(steps):
    return [s for s in steps if s[0] == "query"]


def digest(lives):
    """sha256 over the step lists and the rows of lives: what "the seeded lives are deterministic" pins"""
    h = hashlib.sha256()
    for desc, steps in lives:
        h.update(repr([(k, v) for k, v in sorted(desc.items()) if k not in ("rows", "fresh")]).encode())
        for cols in desc["rows"] + desc["fresh"]:
            for a in cols:
                h.update(np.ascontiguousarray(a, np.int64).tobytes())
        h.update(repr(steps).encode())
    return h.hexdigest()


def oracle_answer(oracle, desc, step):
    """(want, error) of a query step: the oracle's array, or IndexError where the reference raises it.  A slice: its part of the
    whole window's answer; uint8: the uint16 answer narrowed (num_docs <= 255: nothing is lost)."""
    _, form, ver, qs, qe, k, n_docs, extra, _ = step
    memb = form in ("memb", "slice", "oneshot_memb")
    rows = oracle.filter_rows(*desc["rows"][ver], qs, qe, k)
    try:
        want = (oracle.membership if memb else oracle.conservation)(*rows, qs, qe, k, n_docs, literal=False)
    except IndexError:
        return None, IndexError
    if form == "slice":
        want = want[extra[0] - qs:extra[1] - qs]
    if form == "cons8":
        assert n_docs <= 255
        want = want.astype(np.uint8)
    return want, None


class LifeFailure(AssertionError):
    """a step of a life that did not do what the oracle or the API's contract says; .context: what fuzz_gpu.py prints"""

    def __init__(self, msg, context):
        super().__init__(msg + "\n" + "\n".join(f"  {k}: {v}" for k, v in context.items()))
        self.context = context


def _build(memo, desc):
    s, e, o = desc["rows"][0]
    if desc["via_builder"]:
        with memo.IndexBuilder(desc["m"] + desc["extra"], bucket_shift=desc["bshift"], dense=desc["dense_only"]) as b:
            for a_, z_ in zip(desc["cuts"][:-1], desc["cuts"][1:]):
                b.push(s[a_:z_], e[a_:z_], o[a_:z_])
            return b.finish()
    return memo.DeviceIndex.from_host(s, e, o, bucket_shift=desc["bshift"])


def _device_query(memo, ix, fn, args, out):
    """one device-pointer query, memo_query_check behind it, the result on the host"""
    import ctypes as C
    from memo_amd import _lib
    d = C.c_void_p()
    _lib.check(_lib.lib().memo_dev_malloc(ix.device, max(out.nbytes, 16), C.byref(d)))
    try:
        fn(*args, d.value)
        ix.check()
        _lib.check(_lib.lib().memo_dev_download(ix.device, out.ctypes.data, d, out.nbytes, None))
    finally:
        _lib.lib().memo_dev_free(ix.device, d)
    return out


def run_life(memo, oracle, L, ledger=None, name="life", wants=None):
    """play the life L = (desc, steps) on the GPU (memo: the package on the A/B library).  Every answer must equal the oracle's; an
    IndexError must be the oracle's; a refusal (MemoError with one of REFUSALS) passes only on a step the generator marked may_refuse;
    nothing else may be raised.  ledger: a list that receives one (form, pick) per answered query -- debug_last_pick() for
    conservation, debug_last_membership() for membership.  wants: {step number: oracle_answer} computed before.  Returns the number of
    queries played; raises LifeFailure."""
    from memo_amd import _lib, index as memo_index
    lib = _lib.lib()
    desc, steps = L
    played = 0
    ix = _build(memo, desc)

    def context(i, step, **more):
        ctx = dict(life=name, step=i, doing=step, desc={k: v for k, v in desc.items() if k not in ("rows", "fresh")},
                   steps_before=[s for s in steps[:i] if s[0] != "query"][-12:])
        for what, get in (("info", ix.info), ("last_pick", ix.debug_last_pick), ("last_membership", ix.debug_last_membership),
                          ("last_tiles_per_group", ix.debug_last_tiles_per_group)):
            try:
                ctx[what] = get()
            except Exception as exc:                           # (the report must not hide the failure it reports)
                ctx[what] = repr(exc)
        ctx.update(more)
        return ctx

    try:
        if desc["dense_only"]:                                 # (the predicate is asked with what the index says of itself)
            inf, (s0, _, o0) = ix.info(), desc["rows"][0]
            seen = (inf["rows"], inf["min_start"], inf["max_start"], inf["max_annot"])
            if seen != (len(s0), int(s0[0]), int(s0[-1]), int(o0.max())):
                raise LifeFailure("the dense index's rows / starts / largest annot are not its rows'", context(0, "build", seen=seen))
        for i, step in enumerate(steps):
            op = step[0]
            try:
                if op == "pack":
                    ix.pack(keep_wide=step[1])
                elif op == "pack_dense":
                    ix.pack_dense(keep_packed=step[1])
                elif op == "row_order":
                    ix.debug_row_order(step[1])
                elif op == "switches":
                    lib.memo_debug_view_colouring(step[1])
                    lib.memo_debug_six_views(step[2])
                elif op == "option":
                    before = ix.set_option(step[1], step[2])
                    if before != step[3]:
                        raise LifeFailure(f"memo_index_set_option returned {before} as the previous value", context(i, step))
                elif op == "tuning":
                    ix.debug_set_tuning(*step[1:])
                elif op == "upload_rows":
                    ix.upload_rows(step[1], *desc["fresh"][step[2]])
                elif op == "truncate":
                    ix.truncate(step[1])
                elif op == "finalize":
                    ix.finalize(step[1], True)
                elif op == "prepare":
                    try:
                        ix.prepare(step[1], step[2], membership=step[3], window_hint=step[4])
                    except memo.MemoError as exc:
                        if not (step[5] and any(t in str(exc) for t in REFUSALS)):
                            raise
                elif op == "query":
                    played += 1
                    _, form, ver, qs, qe, k, n_docs, extra, may_refuse = step
                    want, werr = wants[i] if wants is not None and i in wants else oracle_answer(oracle, desc, step)
                    got = gerr = None
                    try:
                        if form == "cons16":
                            got = ix.conservation(qs, qe, k, n_docs, np.uint16)
                        elif form == "cons8":
                            got = ix.conservation(qs, qe, k, n_docs, np.uint8)
                        elif form == "memb":
                            got = ix.membership(qs, qe, k, n_docs)
                        elif form == "slice":
                            a, b = extra
                            out = np.empty((b - a, memo_index.words(n_docs)), np.uint32)
                            got = _device_query(memo, ix, lambda *args: ix.membership_slice_dev(*args), (qs, qe, a, b, k, n_docs), out)
                        else:
                            lib.memo_debug_one_shot_way(extra)
                            try:
                                fn = memo_index.membership if form == "oneshot_memb" else memo_index.conservation
                                got = fn(*desc["rows"][ver], qs, qe, k, n_docs)
                            finally:
                                lib.memo_debug_one_shot_way(0)
                    except IndexError:
                        gerr = IndexError
                    except memo.MemoError as exc:
                        if may_refuse and any(t in str(exc) for t in REFUSALS):
                            if ledger is not None:
                                ledger.append(("refused", {"form": form}))
                            continue
                        raise
                    if werr != gerr or (werr is None and not (got.dtype == want.dtype and np.array_equal(got, want))):
                        first = None
                        if werr is None and gerr is None and got.shape == want.shape:
                            first = int(np.argmax((got != want).reshape(len(got), -1).any(axis=1))) if len(got) else None
                        raise LifeFailure("the library's answer is not the oracle's",
                                          context(i, step, oracle_raises=str(werr), library_raises=str(gerr), first_differing_position=first,
                                                  got=None if got is None or first is None else got[first].tolist(),
                                                  want=None if want is None or first is None else want[first].tolist()))
                    if ledger is not None:                     # (an IndexError comes from memo_query_check: the sweep was launched)
                        if form.startswith("oneshot"):
                            if gerr is None:
                                ledger.append((form, {"way": extra, "sweep": int(lib.memo_debug_last_one_shot_sweep())}))
                        elif form in ("cons16", "cons8"):
                            ledger.append(("cons", ix.debug_last_pick()))
                        else:
                            ledger.append((form, ix.debug_last_membership()))
                else:
                    raise ValueError(f"unknown step {step!r}")
            except LifeFailure:
                raise
            except Exception as exc:                           # no other exception is tolerated anywhere
                raise LifeFailure(f"{type(exc).__name__}: {exc}", context(i, step)) from exc
    finally:
        lib.memo_debug_view_colouring(1)
        lib.memo_debug_six_views(-1)
        ix.close()
    return played
