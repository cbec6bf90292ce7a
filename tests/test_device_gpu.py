"""memo_amd._device on the GPU: the owner of the drivers' device memory (DevBuffer: its own allocation, an uploaded array, an adopted
pointer), on_device's two kinds of argument, and emit_text on an empty result."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def memo():
    import memo_amd
    from memo_amd import _lib
    memo_amd.build()                     # make: a no-op when libmemo_amd.so is up to date
    assert _lib.lib().memo_device_count() > 0, "no HIP device: the product has no CPU fallback"
    return memo_amd


@pytest.mark.parametrize("nbytes", (0, 1, 4099))
def test_an_uploaded_array_comes_back(memo, nbytes):
    from memo_amd._device import DevBuffer
    host = np.random.default_rng(nbytes).integers(0, 256, nbytes, dtype=np.uint8)
    with DevBuffer.of(host, 0) as buf:
        assert buf.d.value                                   # an empty array has an address too
        back = buf.to_host(nbytes, np.uint8)
        assert back.dtype == np.uint8 and np.array_equal(back, host)
        if nbytes > 1:                                       # a shorter read, as another type and shape
            assert np.array_equal(buf.to_host((2, 1024), np.uint16), host[:4096].view(np.uint16).reshape(2, 1024))
    assert not buf.d


def test_nothing_is_allocated_for_no_bytes(memo):
    from memo_amd._device import DevBuffer
    with DevBuffer(0, 0) as buf:
        assert not buf.d and buf.at(0).value is None and buf.at(12).value == 12
        assert buf.to_host(0, np.uint32).shape == (0,)       # nothing to download, no call
    buf.close()


def test_offsets_and_a_second_close(memo):
    from memo_amd._device import DevBuffer
    from memo_amd._lib import check, lib
    host = np.arange(1000, dtype=np.uint32)
    buf = DevBuffer.of(host, 0)
    base = buf.d.value
    assert buf.at(0).value == base and buf.at(4 * 333).value == base + 4 * 333
    part = np.empty(5, np.uint32)
    check(lib().memo_dev_download(0, part.ctypes.data, buf.at(4 * 333), part.nbytes, None))
    assert part.tolist() == [333, 334, 335, 336, 337]
    buf.close()
    assert not buf.d
    buf.close()                                              # (nothing left to free: no call)
    assert not buf.d


def test_an_adopted_pointer_is_freed_once(memo, monkeypatch):
    from memo_amd import _device
    from memo_amd._lib import check, lib
    raw = C.c_void_p()
    check(lib().memo_dev_malloc(0, 64, C.byref(raw)))
    freed = []

    class Counting:
        """the library, its memo_dev_free counted"""
        def __getattr__(self, name):
            return getattr(lib(), name)

        def memo_dev_free(self, device, d):
            freed.append(d.value)
            return lib().memo_dev_free(device, d)
    monkeypatch.setattr(_device, "lib", lambda: Counting())
    host = np.arange(16, dtype=np.uint32)
    check(lib().memo_dev_upload(0, raw, host.ctypes.data, host.nbytes, None))
    with _device.DevBuffer.adopt(raw, 0) as buf:
        assert buf.d.value == raw.value
        assert np.array_equal(buf.to_host(16, np.uint32), host)
    buf.close()
    assert freed == [raw.value] and not buf.d
    with _device.DevBuffer.adopt(C.c_void_p(), 0) as none, _device.DevBuffer.adopt(raw.value, 0) as by_number:
        assert not none.d and by_number.d.value == raw.value
        by_number.d = C.c_void_p()                           # (freed above: this owner must not free it again)
    assert freed == [raw.value]


def test_on_device_uploads_an_array_and_leaves_a_pair_alone(memo):
    from memo_amd._device import DevBuffer, on_device
    from memo_amd._lib import check, lib

    def read(d, n):
        out = np.empty(n, np.uint16)
        check(lib().memo_dev_download(0, out.ctypes.data, d, out.nbytes, None))
        return out
    host = np.arange(777, dtype=np.int64)                    # (converted to the asked type on the way)
    with on_device(host, np.uint16, 0) as (d, L):
        assert L == 777 and np.array_equal(read(d, L), host.astype(np.uint16))
    with DevBuffer.of(host.astype(np.uint16), 0) as mine:
        with on_device((mine.d.value, 700), np.uint16, 0) as (d, L):
            assert d.value == mine.d.value and L == 700
        assert mine.d and np.array_equal(read(mine.d, 777), host.astype(np.uint16))        # still there, still readable
    with on_device(np.zeros(0, np.uint16), np.uint16, 0) as (d, L):
        assert L == 0 and d.value


def test_emit_text_of_an_empty_result(memo):
    from memo_amd import maxk
    from memo_amd._device import emit_text
    calls = []

    def call(buf, cap):
        calls.append((buf, cap))
        return 0
    text = emit_text(call)
    assert text.dtype == np.uint8 and text.shape == (0,) and calls == [(None, 0)]          # sized, and not written
    empty = maxk.emit(np.zeros(0))
    assert empty.dtype == np.uint8 and empty.shape == (0,) and bytes(memoryview(empty)) == b""
    assert bytes(memoryview(maxk.emit(np.array([7, 0, 2 ** 31 - 1])))) == b"7\n0\n2147483647\n"
