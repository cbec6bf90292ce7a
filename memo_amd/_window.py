"""How the drivers read a window string, and how they sweep a membership window in slices.

`-r CHR:START-END` is read in one place, parse_region, and raises there what `memo query` raises for the same string.  A driver
that reduces a membership window (matrix, collect, tracks) never holds its result as a whole: membership_slices sweeps it slice
by slice into one reused device buffer, and the driver accumulates each slice where it lies.
"""
from ._device import DevBuffer
from .index import words


def parse_region(region):
    """(record, start, end) of CHR:START-END as `memo query -r` takes it; what is wrong with it raises what memo_query.main raises"""
    record, start_end = region.split(':')                  # exactly one ':' and one '-'
    qs, qe = map(int, start_end.split('-'))
    if qe < qs:
        raise ValueError("negative dimensions are not allowed")          # np.zeros of memo_init, as `memo query` raises it
    return record, qs, qe


def membership_slices(index, qs, qe, k, n_docs, slice_positions, device):
    """Yields (d_bits, s, e) for every slice [s, e) of at most slice_positions positions of the window [qs, qe), from the left:
    the slice's membership rows, uint32 [e - s, W], lie at d_bits until the consumer comes back.  A slice is swept as part of its
    window (membership_slice_dev), so what is accumulated over the slices does not depend on them.  The one buffer is this
    generator's and is freed when it ends or is closed."""
    if slice_positions < 1:
        raise ValueError("slice_positions must be at least 1")
    step = min(int(slice_positions), max(qe - qs, 1))
    with DevBuffer(device, step * 4 * words(n_docs)) as bits:
        for s in range(qs, qe, step):
            e = min(s + step, qe)
            index.membership_slice_dev(qs, qe, s, e, k, n_docs, bits.d.value)
            index.check()
            yield bits.d, s, e
