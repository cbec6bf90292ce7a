"""What every driver needs from the device besides its own kernels: who owns an allocation, and how text comes out of the library.

A driver never calls memo_dev_malloc / memo_dev_free itself.  It holds a DevBuffer (its own allocation, an uploaded host array, or
a pointer the library allocated and handed over) in a `with`, reads results back through to_host, and takes an argument that may
be a host array or a (device pointer, L) pair through on_device.  The text writers of memo_amd/csrc/memo_emit.cpp are called
through emit_text.  (The benchmarked query path -- index.py, cache.py, _fastquery.py -- keeps its own handles: DESIGN.md.)
"""
import contextlib
import ctypes as C

import numpy as np

from ._lib import check, lib


class DevBuffer:
    """one device allocation; none for 0 bytes (d is NULL then)"""

    def __init__(self, device, nbytes):
        self.device, self.d = device, C.c_void_p()
        if nbytes:
            check(lib().memo_dev_malloc(device, nbytes, C.byref(self.d)))

    @classmethod
    def of(cls, host, device):
        """a buffer that holds a C-contiguous host array; of at least 8 bytes, so that an empty array has an address too"""
        buf = cls(device, max(host.nbytes, 8))
        try:
            if host.nbytes:
                check(lib().memo_dev_upload(device, buf.d, host.ctypes.data, host.nbytes, None))
        except BaseException:
            buf.close()
            raise
        return buf

    @classmethod
    def adopt(cls, ptr, device):
        """the owner of a pointer the library allocated (a c_void_p or an integer; NULL owns nothing)"""
        buf = cls(device, 0)
        buf.d = C.c_void_p(getattr(ptr, "value", ptr))
        return buf

    def at(self, offset):
        return C.c_void_p((self.d.value or 0) + offset)

    def to_host(self, shape, dtype):
        """the first bytes of the buffer as a host array of that shape; nothing is downloaded for 0 bytes"""
        out = np.empty(shape, dtype)
        if out.nbytes:
            check(lib().memo_dev_download(self.device, out.ctypes.data, self.d, out.nbytes, None))
        return out

    def close(self):
        if self.d:
            lib().memo_dev_free(self.device, self.d)
            self.d = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


@contextlib.contextmanager
def on_device(host_or_pair, dtype, device):
    """(device pointer, L) of a host array, uploaded for the length of the block, or of a (device pointer, L) pair as it is: the
    pair's memory is its owner's and is not freed"""
    if isinstance(host_or_pair, tuple):
        yield C.c_void_p(int(host_or_pair[0])), int(host_or_pair[1])
        return
    host = np.ascontiguousarray(host_or_pair, dtype)
    with DevBuffer.of(host, device) as buf:
        yield buf.d, len(host)


class RowBuffer:
    """one reused device buffer for a chunk's three int64 columns, each at a 16-byte aligned offset; it grows with the largest chunk"""

    def __init__(self, device):
        self.device, self.d, self.capacity = device, C.c_void_p(), 0

    def upload(self, start, end, annot):
        """(d_start, d_end, d_annot, rows) of host columns"""
        cols = [np.ascontiguousarray(c, np.int64) for c in (start, end, annot)]
        n = len(cols[0])
        if len(cols[1]) != n or len(cols[2]) != n:
            raise ValueError("start, end and annot differ in length")
        if n > self.capacity:
            self.close()
            self.capacity = (n + 1) & ~1
            check(lib().memo_dev_malloc(self.device, 24 * self.capacity, C.byref(self.d)))
        ptrs = [C.c_void_p((self.d.value or 0) + 8 * self.capacity * i) for i in range(3)]
        for p, c in zip(ptrs, cols):
            if n:
                check(lib().memo_dev_upload_pipelined(self.device, p, c.ctypes.data, c.nbytes))
        return (*ptrs, n)

    def close(self):
        if self.d:
            lib().memo_dev_free(self.device, self.d)
        self.d, self.capacity = C.c_void_p(), 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def emit_text(call):
    """The text of a writer of the library as a uint8 array (write it with fh.write(memoryview(buf))): call(buffer, capacity)
    returns the bytes the text needs; a first call sizes the buffer, a second writes it.  Empty text is not written."""
    need = call(None, 0)
    buf = np.empty(need, np.uint8)
    if need:
        got = call(buf.ctypes.data, need)
        assert got == need
    return buf
