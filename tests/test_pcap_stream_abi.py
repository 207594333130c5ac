"""The window calls of pkt_pcap_stream_* (include/pktgpu.h: release, room, released, batch) as the
library exports them: the four symbols load with the signatures pktgpu/_lib.py declares, and each
refuses a NULL stream or a NULL required pointer with PKT_ERR_INVALID_ARG before it looks at either.
No device is touched: no stream is opened (the stand-in for a stream below is never dereferenced)."""
import ctypes

import pytest

from pktgpu import _lib

INVALID_ARG = -1  # PKT_ERR_INVALID_ARG
_P = ctypes.c_void_p
U64P = ctypes.POINTER(ctypes.c_uint64)
WANT = {
    "pkt_pcap_stream_release": (ctypes.c_int, [_P, ctypes.c_uint64]),
    "pkt_pcap_stream_room": (ctypes.c_int, [_P, U64P]),
    "pkt_pcap_stream_released": (ctypes.c_int, [_P, U64P, U64P]),
    "pkt_pcap_stream_batch": (ctypes.c_int, [_P, ctypes.POINTER(_lib.PktBatch)]),
}


@pytest.fixture(scope="module")
def L():
    return _lib.load()


def test_symbols_load_with_the_declared_signatures(L):
    for name, (res, args) in WANT.items():
        assert _lib.SIGNATURES[name] == (res, args), name
        f = getattr(L, name)
        assert f.restype is res and list(f.argtypes) == args, name


def test_null_stream_is_refused(L):
    v, w = ctypes.c_uint64(7), ctypes.c_uint64(9)
    b = _lib.PktBatch()
    b.n = 5
    assert L.pkt_pcap_stream_release(None, 0) == INVALID_ARG
    assert L.pkt_pcap_stream_release(None, 3) == INVALID_ARG
    assert L.pkt_pcap_stream_room(None, ctypes.byref(v)) == INVALID_ARG
    assert L.pkt_pcap_stream_released(None, ctypes.byref(v), ctypes.byref(w)) == INVALID_ARG
    assert L.pkt_pcap_stream_released(None, None, None) == INVALID_ARG
    assert L.pkt_pcap_stream_batch(None, ctypes.byref(b)) == INVALID_ARG
    assert (v.value, w.value, b.n) == (7, 9, 5)  # nothing written
    assert L.pkt_pcap_stream_last_error(None) == b"null stream"


def test_null_required_pointer_is_refused(L):
    """room's `bytes` and batch's `batch` are required (released's two are optional): NULL is refused
    before the stream is read, so a block of zeroed host memory stands in for one."""
    stand_in = ctypes.create_string_buffer(4096)
    st = ctypes.cast(stand_in, _P)
    assert L.pkt_pcap_stream_room(st, None) == INVALID_ARG
    assert L.pkt_pcap_stream_batch(st, None) == INVALID_ARG
    assert stand_in.raw == bytes(4096)
