"""Dead rows of placed six-row views (memo_view_build.hip: view_live_kernel) and the sweep that skips the groups holding none that live
(memo_sweep_cons3t.hip: LIVE).  A view row (s, ov, order) covers [s + ov - (k - 1), s) at every k; a row of strictly lower order
with s_a >= s_b and s_a + ov_a <= s_b + ov_b contains it at every k, so it never decides a minimum.  The view keeps every row (the
bytes a sweep reads do not change); a group of six slots without a live row carries kDeadGroup (bit 20 of its first dword)."""
import numpy as np
import pytest

DEAD_GROUP = 1 << 20


@pytest.fixture(scope="module")
def memo():
    import memo_amd
    from memo_amd import _lib
    memo_amd.build()
    assert _lib.lib().memo_device_count() > 0, "no HIP device: the product has no CPU fallback"
    return memo_amd


@pytest.fixture
def ab(memo):
    """the A/B library (product objects + memo_debug.o): the switches between views with and without places"""
    from memo_amd import _lib
    _lib.use_ab(True)
    yield _lib
    _lib.use_ab(False)


def _dead_brute(s, ov, order, bucket):
    """dead[i]: some row j of bucket(i) or bucket(i) + 1 with order_j < order_i, s_j >= s_i, s_j + ov_j <= s_i + ov_i"""
    dead = np.zeros(len(s), bool)
    edges = np.flatnonzero(np.diff(bucket)) + 1
    lo = np.concatenate(([0], edges))
    hi = np.concatenate((edges, [len(s)]))
    nxt = {int(bucket[a]): (a, b) for a, b in zip(lo, hi)}
    for a, b in zip(lo, hi):
        c0, c1 = a, b
        if int(bucket[a]) + 1 in nxt:
            c1 = nxt[int(bucket[a]) + 1][1]
        S, O, A = s[c0:c1], ov[c0:c1], order[c0:c1]
        for i in range(a, b):
            dead[i] = np.any((A < order[i]) & (S >= s[i]) & (S + O <= s[i] + ov[i]))
    return dead


def _dead_prefix_min(s, ov, order, bucket):
    """the kernel's rule: M[t][j] = least order of the rows of buckets b, b + 1 at position t (0 .. 63) with overlap <= j; row i of
    b is dead iff min over d = 0 .. ov of M[s + d][ov - d] < order"""
    dead = np.zeros(len(s), bool)
    for b in np.unique(bucket):
        M = np.full((64, 32), 1 << 30, np.int64)
        for bb, off in ((b, 0), (b + 1, 32)):
            sel = bucket == bb
            np.minimum.at(M, (s[sel] - 32 * bb + off, ov[sel]), order[sel])
        M = np.minimum.accumulate(M, axis=1)
        for i in np.flatnonzero(bucket == b):
            t, o = s[i] - 32 * b, ov[i]
            dead[i] = min(M[t + d, o - d] for d in range(o + 1)) < order[i]
    return dead


def _rows(seed, n=6000, length=4000, n_docs=12):
    """rows with many ties (few orders), exact duplicates, and starts at both edges of 32-position buckets"""
    rng = np.random.default_rng(seed)
    s = rng.integers(1, length, n)
    s[: n // 4] = (rng.integers(1, length // 32, n // 4) * 32 + rng.choice([-1, 0, 31], n // 4)).clip(1, length - 1)
    ov = rng.integers(0, 40, n)
    o = rng.integers(1, n_docs, n)
    dup = rng.integers(0, n, n // 10)
    s, ov, o = np.concatenate((s, s[dup])), np.concatenate((ov, ov[dup])), np.concatenate((o, o[dup]))
    idx = np.argsort(s, kind="stable")
    return s[idx].astype(np.int64), ov[idx].astype(np.int64), o[idx].astype(np.int64)


def test_prefix_min_rule_is_the_containment_rule():
    for seed in range(3):
        s, ov, o = _rows(seed)
        keep = ov < 30
        s, ov, o = s[keep], ov[keep], o[keep]
        bucket = s >> 5
        brute = _dead_brute(s, ov, o, bucket)
        assert np.array_equal(_dead_prefix_min(s, ov, o, bucket), brute)
        assert 0.2 < brute.mean() < 0.95, brute.mean()


def _decode(view):
    """(slots of every group: start mod 32, overlap, annot), group flags, bucket of every group"""
    g = view[0].reshape(-1, 4).astype(np.int64)
    lo = np.stack([g[:, 0] & 0x3FF, g[:, 1] & 0x3FF, g[:, 2] & 0x3FF, g[:, 3] & 0x3FF, (g[:, 0] >> 10) & 0x3FF, (g[:, 3] >> 10) & 0x3FF], 1)
    an = np.stack([g[:, 0] >> 24, g[:, 1] >> 24, g[:, 2] >> 24, g[:, 3] >> 24, (g[:, 1] >> 10) & 0xFF, (g[:, 2] >> 10) & 0xFF], 1)
    table = view[1]
    ng = int(table[-1]) // 6
    bucket = np.searchsorted(table[1:] // 6, np.arange(ng), side="right")
    return lo[:ng] & 31, lo[:ng] >> 5, an[:ng], (g[:ng, 0] & DEAD_GROUP) != 0, bucket


@pytest.mark.gpu
def test_dead_group_flags_against_brute_force(memo, ab):
    s, ov, o = _rows(11, n=40_000, length=30_000, n_docs=20)
    e = s + ov
    try:
        ab.check(ab.lib().memo_debug_six_views(1))
        for k in (9, 21, 31):
            views = {}
            for placed in (0, 1):
                ab.check(ab.lib().memo_debug_view_colouring(placed))
                with memo.DeviceIndex.from_host(s, e, o) as ix:
                    ix.pack(keep_wide=False)
                    ix.pack_dense(keep_packed=False)
                    ix.prepare(k, 20)
                    views[placed] = ix.export_view(k, 6)
                    assert ix.info()["view_placings"] == placed
            plain, placed = views[0], views[1]
            assert np.array_equal(plain[1], placed[1]) and plain[2] == placed[2], k   # rows per bucket, the table: unchanged
            ps, pov, pan, pflag, pb = _decode(plain)
            assert not pflag.any()                                                   # the view without places: no flags
            gs, gov, gan, flag, gb = _decode(placed)
            for a, b in ((ps, gs), (pov, gov), (pan, gan)):                          # every bucket holds the same slots
                key_a = np.lexsort((a.reshape(-1), np.repeat(pb, 6)))
                key_b = np.lexsort((b.reshape(-1), np.repeat(gb, 6)))
                assert np.array_equal(a.reshape(-1)[key_a], b.reshape(-1)[key_b])
            slot_b = np.repeat(gb, 6)
            S = slot_b * 32 + gs.reshape(-1)
            dead = _dead_brute(S, gov.reshape(-1), gan.reshape(-1), slot_b).reshape(-1, 6)
            assert dead[flag].all(), k                                               # a flagged group holds dead rows only
            assert np.array_equal(flag, dead.all(axis=1)), k                         # ... and every group of dead rows is flagged
            # live rows first: a bucket's live slots fill ceil(live / 6) groups -- plus those the copies of its last row land in, when
            # that row is live (the places no row took hold copies of it, as in the view without places: up to five)
            need = extra = 0
            for b in np.unique(gb):
                sel = gb == b
                nl = int((~dead[sel]).sum())
                live_groups = int((~flag[sel]).sum())
                assert live_groups <= (nl + 5) // 6 + 5, (k, b, nl, live_groups)
                need += (nl + 5) // 6
                extra += live_groups - (nl + 5) // 6
            assert extra <= 0.25 * need, (k, need, extra)
            assert flag.mean() > 0.05, (k, flag.mean())                                  # (there are flags to skip)
    finally:
        ab.check(ab.lib().memo_debug_view_colouring(1))
        ab.check(ab.lib().memo_debug_six_views(-1))


@pytest.mark.gpu
def test_live_sweep_equals_oracle_every_k_class(memo, oracle):
    from memo_amd import synth
    n, L = 40, 400_000
    ix, (r0, r1) = synth.device_index(0, L, 33, n, L, pack="dense")
    num, den = synth.rows_per_position(n)
    s, e, o = oracle.synth_rows(r0, r1 - r0, num, den, n)
    rng = np.random.default_rng(5)
    with ix:
        ix.set_option(4, 6)
        ix.set_option(5, 1)
        for k in range(2, 33):
            ix.prepare(k, n)
            for _ in range(2):
                qs = int(rng.integers(1, 40_000)) * 4 + int(rng.integers(1, 4)) + 300   # mid-tile, off the 4-position raster
                qe = min(qs + int(rng.integers(50_000, 300_000)), L - 100)
                got = ix.conservation(qs, qe, k, n)
                inf = ix.info()
                assert inf["last_variant"] == 3 and inf["last_view_placed"] == 1 and inf["last_view_rows_per_group"] == 6, (k, inf)
                want = oracle.conservation(*oracle.filter_rows(s, e, o, qs, qe, k), qs, qe, k, n, literal=False)
                assert np.array_equal(got, want), (k, qs, qe, int(np.argmax(got != want)))
