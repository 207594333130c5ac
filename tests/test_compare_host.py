"""pkt_compare_host through pktgpu.compare (no device): Packet::compare (packet.rs:326-358) over two
host batches.  Every expected value comes from compare_cases.expect (numpy, from the definition) or is
known by construction; none comes from the code under test."""
import ctypes
import os

import numpy as np
import pytest

import pktgpu
from pktgpu import _lib, gen

import compare_cases as C
from compare_cases import check


@pytest.mark.parametrize("name", C.CASE_NAMES)
def test_cases(name):
    c, want = C.all_cases()[name]
    check(pktgpu.compare(c["a"], c["b"], c["ignore"], c["chain"]), want, name)


def test_case_list_is_complete_and_not_trivial():
    cs = C.all_cases()
    assert sorted(cs) == sorted(C.CASE_NAMES)
    seen = set()
    for name, (c, (res, mt, fd, sm)) in cs.items():
        seen |= set(res.tolist())
        if c["ignore"]:
            # differences confined to ignored bits (packets of mode 1) are EQUAL with matching == len, a
            # flipped neighbouring bit is a difference
            ext = C.extents(c["a"])
            assert sm["n_equal"] > 0 and sm["n_bytes"] + sm["n_len"] > 0, name
            if name != "cut_field":
                assert len(c["neighbour"]) > 3, name
                for i in range(c["a"]["n"]):
                    if c["modes"][i] == 1:
                        assert res[i] == C.EQUAL and mt[i] == ext[i][1], (name, i)
                    if i in c["neighbour"]:
                        assert res[i] == C.BYTES and mt[i] == ext[i][1] - 1, (name, i)
    assert seen == {C.EQUAL, C.LEN, C.BYTES}
    res = cs["cut_field"][1][0]
    assert (res == C.LEN).sum() > 10


def test_alignment():
    c, (res, mt, fd) = C.alignment()
    check(pktgpu.compare(c["a"], c["b"]), (res, mt, fd, None), "alignment")


def test_ref22_to_vec_round_trip():
    """tests/lib.rs:674-679: the 22 packets against their own bytes are all equal; against a capture of
    them (an indexed batch, records at any alignment) too."""
    pk = [bytes(p.to_vec()) for p in gen.reference_22_packets()]
    a = C.indexed(pk, np.random.default_rng(1))
    pc = np.frombuffer(open(os.path.join(C.GOLD, "ref22.pcap"), "rb").read(), np.uint8)
    offs, lens = gen.pcap_index_py(pc.tobytes())
    res, mt, fd, sm = pktgpu.compare(a, C.batch(pc, offs, lens))
    assert sm == dict(n_equal=22, n_len=0, n_bytes=0, first_bad=22)
    assert (res == 0).all() and np.array_equal(mt, lens) and np.array_equal(fd, lens)


def test_argument_errors():
    a = C.batch(gen.gen_c2(4), stride=64)
    b3 = C.batch(gen.gen_c2(3), stride=64)
    ch = C.chain_of(a)
    with pytest.raises(ValueError):
        pktgpu.compare(a, b3)                                     # a->n != b->n
    with pytest.raises(ValueError):
        pktgpu.compare(a, a, [("IPv4", 0, 64, 71)])               # ignores without a chain
    with pytest.raises(ValueError):
        pktgpu.compare(a, a, [("IPv4", 0, 64, 63)], ch)           # end < start
    with pytest.raises(ValueError):
        pktgpu.compare(a, a, [("IPv4", 0, 64, 71)] * 17, ch)      # more than 16
    assert pktgpu.compare(a, a, [("IPv4", 0, 64, 71)] * 16, ch)[3]["n_equal"] == 4
    L = _lib.load()
    assert L.pkt_sizeof_cmp_summary() == ctypes.sizeof(_lib.PktCmpSummary) == 32
    big = _lib.PktBatch()
    big.n = 1 << 32
    big.stride = 64
    assert L.pkt_compare_host(ctypes.byref(big), ctypes.byref(big), None, None, 0, None, None, None, None) != 0
    # NULL outputs: the summary alone
    sm = _lib.PktCmpSummary()
    ba = pktgpu._host_batch(_lib, a)[0]
    assert L.pkt_compare_host(ctypes.byref(ba), ctypes.byref(ba), None, None, 0, None, None, None, ctypes.byref(sm)) == 0
    assert (sm.n_equal, sm.n_len, sm.n_bytes, sm.first_bad) == (4, 0, 0, 4)
