"""The oracle of `memo collect` (test infrastructure; the product never imports it): the collector's curves of unpacked membership
bits B uint8 [L, N] over orders [P, M] of genome ids, by NumPy's accumulate along the order:

    core   [q] = np.logical_and.accumulate(B[:, orders[q]], axis=1).sum(0)
    covered[q] = np.logical_or .accumulate(B[:, orders[q]], axis=1).sum(0)

Both int64 [P, M].  Every comparison against it is exact."""
import numpy as np


def curves(B, orders):
    B = np.asarray(B).astype(bool)
    orders = np.asarray(orders, np.int64)
    assert B.ndim == 2 and orders.ndim == 2
    core = np.zeros(orders.shape, np.int64)
    covered = np.zeros(orders.shape, np.int64)
    for q, order in enumerate(orders):
        if len(order):
            cols = B[:, order]
            core[q] = np.logical_and.accumulate(cols, axis=1).sum(0)
            covered[q] = np.logical_or.accumulate(cols, axis=1).sum(0)
    return core, covered


def unpack(bits, num_docs):
    """membership rows uint32 [L, W] (bit g & 31 of word g >> 5) -> uint8 [L, N]"""
    bits = np.ascontiguousarray(bits, np.uint32)
    return np.unpackbits(bits.view(np.uint8), axis=1, bitorder="little")[:, :num_docs]
