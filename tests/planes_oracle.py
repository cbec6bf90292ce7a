"""References for the three plane kernels (`memo matrix`, `memo collect`, `memo tracks`) that work on the PACKED membership rows
uint32 [L, W] (bit g & 31 of word g >> 5 is genome g), for the sizes at which the definitions on the unpacked bits B uint8 [L, N] --
test_matrix_gpu.oracle, collect_oracle.curves, tracks_oracle.tracks -- cost gigabytes and tens of seconds.  Test infrastructure; the
product never imports it.  tests/test_planes_oracle_cpu.py holds each of them against its definition: they are trusted on the GPU only
because they agree there.

    cooccurrence(bits, N)            int64 [N, N]         B.T @ B, in float32 blocks of at most 2^15 rows summed in float64: exact
    tracks(bits, N, edges, first)    int64 [N, bins]      np.add.reduceat over the non-empty bins, a few genome words at a time
    curves(bits, N, orders)          2 x int64 [P, M]     per-genome planes of 64 positions a word, &= and |= along each order

Bits at or above N of the last word never count.  And the rows themselves: density_rows (per-genome densities from ANDs and ORs of
random words) and structure (columns a kernel can get wrong in ways that random ones hide)."""
import numpy as np

BLOCK_ROWS = 1 << 15


def unpack(bits, N):
    """membership rows uint32 [L, W] -> uint8 [L, N]"""
    bits = np.ascontiguousarray(bits, np.uint32)
    return np.unpackbits(bits.view(np.uint8), axis=1, bitorder="little")[:, :N]


def _rows(bits, N):
    bits = np.asarray(bits, np.uint32)
    assert bits.ndim == 2 and bits.shape[1] == (N + 31) // 32, (bits.shape, N)
    return bits


# ---------------------------------------------------------------------------------------
# the references
# ---------------------------------------------------------------------------------------
def cooccurrence(bits, N):
    bits = _rows(bits, N)
    L = len(bits)
    assert BLOCK_ROWS < 2 ** 24 and L < 2 ** 53           # a block's entries are exact in float32, the totals in float64
    total = np.zeros((N, N), np.float64)
    for lo in range(0, L, BLOCK_ROWS):
        B = unpack(bits[lo:lo + BLOCK_ROWS], N).astype(np.float32)
        assert len(B) <= BLOCK_ROWS
        total += B.T @ B
    assert total.max(initial=0) <= L
    return total.astype(np.int64)


def tracks(bits, N, edges, first=0, words_at_a_time=4):
    bits = _rows(bits, N)
    L, W = bits.shape
    rel = np.clip(np.asarray(edges, np.int64) - int(first), 0, L)
    assert rel.ndim == 1 and len(rel) >= 1 and (np.diff(rel) >= 0).all() and L < 2 ** 32
    out = np.zeros((N, len(rel) - 1), np.int64)
    full = np.flatnonzero(rel[1:] > rel[:-1])               # the non-empty bins: consecutive runs of [rel[0], rel[-1])
    if not len(full):
        return out
    lo, hi = int(rel[0]), int(rel[-1])
    starts = rel[full] - lo
    for w0 in range(0, W, words_at_a_time):
        w1 = min(w0 + words_at_a_time, W)
        g0, g1 = 32 * w0, min(32 * w1, N)
        B = unpack(bits[lo:hi, w0:w1], g1 - g0)
        out[g0:g1, full] = np.add.reduceat(B, starts, axis=0, dtype=np.uint32).T     # (a bin's sum is at most L < 2^32)
    return out


def planes(bits, N):
    """uint64 [N, ceil(L / 64)]: bit p & 63 of word p >> 6 of row g is bit g of position p; the pad bits of the last word are 0"""
    bits = _rows(bits, N)
    L, W = bits.shape
    nw = (L + 63) // 64
    out = np.zeros((N, 8 * nw), np.uint8)
    for w in range(W):
        n = min(32, N - 32 * w)
        out[32 * w:32 * w + n, :(L + 7) // 8] = np.packbits(unpack(bits[:, w:w + 1], n).T, axis=1, bitorder="little")
    return out.view(np.uint64)


def curves(bits, N, orders):
    """(core, covered), int64 [P, M]"""
    orders = np.asarray(orders, np.int64)
    assert orders.ndim == 2 and (not orders.size or (orders.min() >= 0 and orders.max() < N))
    P, M = orders.shape
    pl = planes(bits, N)
    L, nw = len(bits), pl.shape[1]
    core, covered = np.zeros((P, M), np.int64), np.zeros((P, M), np.int64)
    if not nw:
        return core, covered
    ones = np.full(nw, ~np.uint64(0))
    if L % 64:
        ones[-1] = np.uint64((1 << (L % 64)) - 1)           # the running AND starts without the pad bits
    block = max(1, BLOCK_ROWS // nw)                        # orders taken together: many short ones, or one long one
    for q0 in range(0, P, block):
        rows = orders[q0:q0 + block]
        a = np.tile(ones, (len(rows), 1))
        o = np.zeros_like(a)
        for j in range(M):
            x = pl[rows[:, j]]
            a &= x
            o |= x
            core[q0:q0 + block, j] = np.bitwise_count(a).sum(axis=1, dtype=np.int64)
            covered[q0:q0 + block, j] = np.bitwise_count(o).sum(axis=1, dtype=np.int64)
    return core, covered


def column_counts(bits, N):
    """int64 [N]: the popcount of each genome's column"""
    bits = _rows(bits, N)
    total = np.zeros(N, np.int64)
    for lo in range(0, len(bits), BLOCK_ROWS):
        total += unpack(bits[lo:lo + BLOCK_ROWS], N).sum(axis=0, dtype=np.int64)
    return total


# ---------------------------------------------------------------------------------------
# the rows
# ---------------------------------------------------------------------------------------
def density_rows(L, N, levels, seed=0, conserved=0):
    """Packed rows uint32 [L, W] whose genome g is present at a share of 1 - 2^-k of the positions for levels[g] = k >= 1 (the OR
    of k random words) and of 2^k for k <= -1 (the AND of -k random words); levels is one number or one per genome, |k| <= 6.
    conserved: every 2^conserved-th position or so (0: none) holds every genome, so that a long order's core does not die out."""
    levels = np.broadcast_to(np.asarray(levels, np.int64), (N,))
    assert ((np.abs(levels) >= 1) & (np.abs(levels) <= 6)).all()
    W = (N + 31) // 32
    rng = np.random.default_rng([seed, L, N])
    draw = lambda: rng.integers(0, 2 ** 32, (L, W), dtype=np.uint32)

    def class_mask(k):                                      # uint32 [W]: the bits of the genomes at level k
        m = np.zeros(32 * W, np.uint8)
        m[:N] = levels == k
        return np.packbits(m, bitorder="little").view(np.uint32)
    out = np.zeros((L, W), np.uint32)
    ands = draw()
    ors = ands.copy()
    for k in range(1, 7):
        if k > 1 and (np.abs(levels) >= k).any():
            r = draw()
            ands &= r
            ors |= r
        for level, source in ((k, ors), (-k, ands)):
            m = class_mask(level)
            if m.any():
                out |= source & m
    if conserved:
        every = np.ones(L, bool)
        for _ in range(conserved):
            every &= rng.integers(0, 2, L).astype(bool)
        out[every] = 0xFFFFFFFF
    last = N & 31
    if last:
        out[:, -1] &= np.uint32((1 << last) - 1)
    return out


def set_column(bits, g, present):
    """genome g's column of packed rows, in place: present is bool [L] or one bool"""
    bit = np.uint32(1 << (g & 31))
    col = bits[:, g >> 5]
    col &= ~bit
    col |= np.where(present, bit, np.uint32(0))


def get_column(bits, g):
    return (bits[:, g >> 5] >> np.uint32(g & 31)) & np.uint32(1) != 0


def structure(bits, N, T, seed=0):
    """Overwrites eight columns of packed rows (N >= 8) in place and returns {name: genome}: `everywhere`; `absent`; `tile_ends`,
    present only at the last position of every whole tile of T positions; `tail`, present only in the ragged tail behind the last
    whole tile; `twin_a` = `twin_b`; `mirror_a` = not `mirror_b`.  The genomes are drawn from all the words, genomes 0, 31, 32 and
    N - 1 among them."""
    L = len(bits)
    assert N >= 8 and L % T, "a ragged tail is part of the structure"
    rng = np.random.default_rng([seed, N, 8])
    fixed = [g for g in (0, 31, 32, N - 1) if g < N]
    fixed = list(dict.fromkeys(fixed))
    rest = [int(g) for g in rng.permutation(N) if g not in fixed]
    chosen = (fixed + rest)[:8]
    rng.shuffle(chosen)
    names = ("everywhere", "absent", "tile_ends", "tail", "twin_a", "twin_b", "mirror_a", "mirror_b")
    at = dict(zip(names, (int(g) for g in chosen)))
    p = np.arange(L)
    set_column(bits, at["everywhere"], True)
    set_column(bits, at["absent"], False)
    set_column(bits, at["tile_ends"], (p % T == T - 1))
    set_column(bits, at["tail"], p >= L - L % T)
    set_column(bits, at["twin_b"], get_column(bits, at["twin_a"]))
    set_column(bits, at["mirror_b"], ~get_column(bits, at["mirror_a"]))
    return at
