"""The oracle of `memo tracks`: NumPy on the unpacked bits B [L, N] of a membership result that holds the positions first .. first + L,

    counts[g][b] = B[edges[b] : edges[b + 1], g].sum()          int64 [N, bins], the edges clipped to the slice

and the packing of such bits into membership rows (as tests/test_matrix_gpu.py packs them)."""
import numpy as np


def tracks(B, edges, first=0):
    B = np.asarray(B)
    L, N = B.shape
    rel = np.clip(np.asarray(edges, np.int64) - int(first), 0, L)
    out = np.zeros((N, len(rel) - 1), np.int64)
    for b in range(len(rel) - 1):
        out[:, b] = B[rel[b]:rel[b + 1]].sum(axis=0, dtype=np.int64)
    return out


def tracks_fast(B, edges, first=0):
    """the same through one prefix sum: for tables of many bins"""
    B = np.asarray(B)
    L, N = B.shape
    rel = np.clip(np.asarray(edges, np.int64) - int(first), 0, L)
    cum = np.zeros((L + 1, N), np.int64)
    np.cumsum(B, axis=0, dtype=np.int64, out=cum[1:])
    return np.ascontiguousarray((cum[rel[1:]] - cum[rel[:-1]]).T)


def pack(B, garbage=None):
    """B uint8 [L, N] as membership rows uint32 [L, W]: bit g & 31 of word g >> 5.  garbage: the bits at or above N of the last word"""
    B = np.asarray(B, np.uint8)
    L, N = B.shape
    W = (N + 31) // 32
    full = np.zeros((L, 32 * W), np.uint8)
    full[:, :N] = B
    if garbage is not None:
        full[:, N:] = garbage
    return np.ascontiguousarray(np.packbits(full, axis=1, bitorder="little")).view(np.uint32).reshape(L, W)


def random_bits(L, N, density, seed=0):
    return (np.random.default_rng([seed, L, N]).random((L, N)) < density).astype(np.uint8)
