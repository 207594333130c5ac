"""pkt_pcap_write_host (the CPU model of pkt_pcap_write, through pktgpu.pcap_write): a batch written
out as a tests/pcap.rs:7-37 capture.  Every expected capture is built record by record with
struct.pack in pcap_write_cases.expect, and the index of every result is checked against
gen.pcap_index_py of the result."""
import ctypes

import numpy as np
import pytest

import pktgpu
from pktgpu import gen

import pcap_write_cases as C

CASES = C.host_cases()


def write(c, dst=None):
    return pktgpu.pcap_write(c["slab"], offsets=c["offsets"], lens=c["lens"], stride=c["stride"], n=c["n"],
                             select=c["select"], snaplen=c["snaplen"], ts=c["ts"], dst=dst)


def check(c, label):
    want, w_off, w_len, w_src = C.expect(c)
    cap, n, offs, lens, src = write(c)
    assert cap.tobytes() == want, label
    assert n == len(w_src) and cap.size == len(want), label
    assert np.array_equal(offs, w_off) and np.array_equal(lens, w_len) and np.array_equal(src, w_src), label
    i_off, i_len = gen.pcap_index_py(cap.tobytes())
    assert np.array_equal(offs, i_off) and np.array_equal(lens, i_len), label
    return cap, n, offs, lens, src


def test_golden_round_trip():
    buf, c = C.golden()
    cap, n, offs, lens, src = check(c, "golden")
    assert cap.tobytes() == buf  # byte-equal to the file
    assert n == 22 and np.array_equal(src, np.arange(22))
    assert np.array_equal(offs, c["offsets"]) and np.array_equal(lens, c["lens"])


@pytest.mark.parametrize("per_packet_ts", [False, True])
def test_length_edges(per_packet_ts):
    c = C.edges(per_packet_ts)
    cap, n, offs, lens, src = check(c, "edges")
    assert n == len(C.EDGE_LENS) and np.array_equal(lens, C.EDGE_LENS)


@pytest.mark.parametrize("mask", list(C.select_masks()))
def test_select(mask):
    c = C.select_case(mask)
    cap, n, offs, lens, src = check(c, mask)
    keep = np.flatnonzero(c["select"])
    assert n == keep.size and np.array_equal(src, keep)
    assert cap.size == 24 + keep.size * (16 + 64)


@pytest.mark.parametrize("snaplen", [1, 16, 60, 65535])
def test_snaplen(snaplen):
    c = C.edges(per_packet_ts=True, snaplen=snaplen)
    cap, n, offs, lens, src = check(c, snaplen)
    buf = cap.tobytes()
    for k, ln in enumerate(C.EDGE_LENS):
        incl, orig = np.frombuffer(buf, "<u4", 2, int(offs[k]) - 8)
        assert incl == min(ln, snaplen) and orig == ln, (k, ln)
        o = int(c["offsets"][k])
        assert buf[int(offs[k]):int(offs[k]) + incl] == c["slab"][o:o + incl].tobytes()


def test_batch_clamping():
    indexed, fixed = C.clamped()
    cap, n, offs, lens, src = check(indexed, "clamped indexed")
    assert list(lens) == [50, 100, 0, 0, 1, 1000]  # past slab_len: clamped; starting past it: empty
    cap, n, offs, lens, src = check(fixed, "clamped fixed")
    assert n == 18 and list(lens[14:]) == [64, 40, 0, 0]


def test_capacity_and_empty():
    c = C.edges()
    want = C.expect(c)[0]
    total = len(want)
    dst = np.full(total + 64, 0xA5, np.uint8)
    cap, n, *_ = write(c, dst[:total])  # dst_len == total
    assert cap.tobytes() == want and (dst[total:] == 0xA5).all()
    dst = np.full(total + 64, 0xA5, np.uint8)
    cap, n, *_ = write(c, dst)          # room to spare: nothing at or past total is written
    assert cap.size == total and cap.tobytes() == want and (dst[total:] == 0xA5).all()
    dst = np.full(total + 64, 0xA5, np.uint8)
    with pytest.raises(ValueError, match=str(total)):
        write(c, dst[:total - 1])
    assert (dst[total - 1:] == 0xA5).all()
    # the raw call reports both totals with PKT_ERR_INVALID_ARG
    from pktgpu import _lib
    L = _lib.load()
    b = _lib.PktBatch()
    b.slab, b.slab_len = c["slab"].ctypes.data, c["slab"].size
    b.offsets, b.lens, b.n = c["offsets"].ctypes.data, c["lens"].ctypes.data, c["n"]
    nb, nr = ctypes.c_uint64(), ctypes.c_uint64()
    rc = L.pkt_pcap_write_host(ctypes.byref(b), None, 0, 0, 0, None, None, dst.ctypes.data, total - 1, None, None,
                               None, ctypes.byref(nb), ctypes.byref(nr))
    assert rc == -1 and nb.value == total and nr.value == c["n"]
    b.n = 1 << 32
    assert L.pkt_pcap_write_host(ctypes.byref(b), None, 0, 0, 0, None, None, dst.ctypes.data, dst.size, None, None,
                                 None, ctypes.byref(nb), ctypes.byref(nr)) == -1
    # n == 0 and an empty selection: the 24 header bytes
    cap, n, offs, lens, src = check(CASES["empty_batch"], "n == 0")
    assert cap.tobytes() == gen.PCAP_GLOBAL_HEADER and n == 0 and offs.size == 0
    cap, n, *_ = check(C.select_case("none"), "none selected")
    assert cap.tobytes() == gen.PCAP_GLOBAL_HEADER and n == 0
