"""pkt_l4_checksum_host through pktgpu.l4_checksum (no device): the TCP / UDP / ICMP checksum of every
packet of a host batch.  Every expected value comes from l4_cases.expect (an independent pure-Python
RFC 1071 loop, pinned by the RFC's own example) or is known by construction; none comes from the code
under test."""
import ctypes

import numpy as np
import pytest

import pktgpu
from pktgpu import _lib, gen, schema

import l4_cases as L4


def run(c, update=False, keep=False, slab=None):
    b = c["batch"]
    return pktgpu.l4_checksum(b["slab"] if slab is None else slab, c["chain"], c["which"], update, keep,
                              stride=b["stride"], n=b["n"], offsets=b["offsets"], lens=b["lens"])


def test_yardstick_is_rfc1071_section_3():
    L4.pin_yardstick()


@pytest.mark.parametrize("name", L4.CASE_NAMES)
def test_cases(name):
    c, want, _, _ = L4.all_cases()[name]
    L4.check(run(c), want, name)


def test_table_covers_every_status_and_both_update_paths():
    cs = L4.all_cases()
    assert sorted(cs) == sorted(L4.CASE_NAMES)
    seen, written, kept = set(), 0, 0
    for name, (c, want, upd, keep) in cs.items():
        seen |= set(want["status"].tolist())
        written += int((upd["slab"] != c["batch"]["slab"]).any())  # cases in which UPDATE stores something new
        kept += int((upd["slab"] != keep["slab"]).any())           # ... and in which KEEP_ZERO_UDP holds a store back
    assert seen == set(range(7)), seen
    assert written > 5 and kept >= 3
    c, want, _, _ = cs["specials"]
    assert want["status"].tolist() == c["known"], [(n, k, s) for n, k, s in zip(c["names"], c["known"], want["status"]) if k != s]
    i = c["names"].index("udp4_sum_ffff")
    assert want["calc"][i] == 0xFFFF and want["stored"][i] == 0xFFFF
    i = c["names"].index("tcp4_calc0_storedffff")
    assert want["calc"][i] == 0 and want["stored"][i] == 0xFFFF and want["status"][i] == L4.OK
    # the segment starts of 0, 1 and 2 Vlan tags, a uniform wave and a 65535-byte packet among short ones
    starts = set(int(cs["protocols"][0]["chain"]["hdr_off"][j, i]) for i in range(108) for j in range(6)
                 if cs["protocols"][0]["chain"]["hdr_type"][j, i] in L4.L4_SIZE)
    assert {34, 38, 42} <= starts
    assert 65535 in cs["long_among_short"][0]["batch"]["lens"][:64] and 64 in cs["long_among_short"][0]["batch"]["lens"][:64]
    assert sorted(int(o) % 16 for o in cs["every_alignment"][0]["batch"]["offsets"][::2]) == list(range(16))
    w = cs["vxlan_which_1"][1]["status"]
    assert (w == L4.OK).sum() == 20 and (w == L4.ABSENT).sum() > 0
    assert (cs["vxlan_which_2"][1]["status"] == L4.ABSENT).all()


@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("name", L4.CASE_NAMES)
def test_update(name, keep):
    """UPDATE: the outputs still describe the field as read; the slab afterwards is the input with only
    the expected two bytes of each written packet changed; a second, read-only pass reports OK wherever
    the first wrote."""
    c, want, upd, kp = L4.all_cases()[name]
    exp = kp if keep else upd
    slab = c["batch"]["slab"].copy()
    L4.check(run(c, True, keep, slab), want, name)
    assert np.array_equal(slab, exp["slab"]), np.flatnonzero(slab != exp["slab"])[:8]
    again = run(c, slab=slab)
    st = want["status"]
    wrote = (st == L4.OK) | (st == L4.BAD) | ((st == L4.UNCHECKED) & (not keep))
    assert (again["status"][wrote] == L4.OK).all()
    assert np.array_equal(again["status"][~wrote], st[~wrote])
    assert np.array_equal(again["calc"], want["calc"])
    assert np.array_equal(again["stored"][wrote], want["calc"][wrote])


def test_null_outputs_and_refusals():
    L = _lib.load()
    c, want, _, _ = L4.all_cases()["mixed_1000"]
    b, keep_alive = pktgpu._host_batch(_lib, c["batch"])
    cols = (c["chain"]["n_hdrs"], c["chain"]["hdr_type"], c["chain"]["hdr_off"])
    ch = _lib.PktChain(*[x.ctypes.data for x in cols])
    n = b.n
    for k, (name, dt) in enumerate((("calc", np.uint16), ("stored", np.uint16), ("status", np.uint8))):
        outs = [np.zeros(n, np.uint16), np.zeros(n, np.uint16), np.zeros(n, np.uint8)]
        ptrs = [o.ctypes.data for o in outs]
        ptrs[k] = None
        assert L.pkt_l4_checksum_host(ctypes.byref(b), ctypes.byref(ch), L4.LAST, 0, *ptrs) == 0
        outs[k] = None
        L4.check(dict(calc=outs[0], stored=outs[1], status=outs[2]), want, "without " + name)
    assert L.pkt_l4_checksum_host(ctypes.byref(b), ctypes.byref(ch), L4.LAST, 0, None, None, None) == 0

    def rc(batch=b, chain=ch, which=0, flags=0):
        return L.pkt_l4_checksum_host(ctypes.byref(batch) if batch is not None else None,
                                      ctypes.byref(chain) if chain is not None else None, which, flags, None, None, None)
    assert rc() == 0
    assert rc(batch=None) == -1 and rc(chain=None) == -1
    for k in range(3):                                                  # a NULL chain column
        p = [x.ctypes.data for x in cols]
        p[k] = None
        assert rc(chain=_lib.PktChain(*p)) == -1
    assert rc(which=16) == -1 and rc(which=0xFE) == -1 and rc(which=15) == 0 and rc(which=0xFF) == 0
    assert rc(flags=4) == -1 and rc(flags=8 | 1) == -1                  # unknown flag bits
    assert rc(flags=schema.L4_KEEP_ZERO_UDP) == -1                      # KEEP_ZERO_UDP without UPDATE
    huge = _lib.PktBatch()
    huge.slab, huge.slab_len, huge.stride, huge.n = b.slab, b.slab_len, 64, 1 << 32
    assert rc(batch=huge) == -1                                         # n >= 2^32
    for bad in (dict(offsets=b.offsets, lens=None, stride=0), dict(offsets=None, lens=None, stride=0),
                dict(offsets=b.offsets, lens=b.lens, stride=0, slab=None)):
        x = _lib.PktBatch()
        x.slab, x.slab_len, x.n = bad.get("slab", b.slab), b.slab_len, n
        x.offsets, x.lens, x.stride = bad["offsets"], bad["lens"], bad["stride"]
        assert rc(batch=x) == -1, bad                                   # offsets without lens, stride 0, null slab
    empty = _lib.PktBatch()
    assert rc(batch=empty) == 0                                         # n == 0 succeeds
    with pytest.raises(ValueError):
        pktgpu.l4_checksum(c["batch"]["slab"], c["chain"], 16, offsets=c["batch"]["offsets"], lens=c["batch"]["lens"])
    assert schema.L4_STATUS == ["OK", "BAD", "UNCHECKED", "ABSENT", "NO_IP", "SPAN", "FRAGMENT"]
    assert (pktgpu.L4_OK, pktgpu.L4_FRAGMENT, pktgpu.L4_LAST) == (0, 6, 0xFF)


def test_reference_builders_leave_the_l4_checksum_undone():
    """The reference's builders take `_tcp_checksum` / `_udp_checksum` and ignore them (utils.rs:156, 213):
    of its 22 packets none carries a good L4 checksum except by the v4 UDP rule (0 = none sent); after
    UPDATE every packet with an L4 header verifies."""
    pk = [bytes(p.to_vec()) for p in gen.reference_22_packets()]
    c = L4.case(L4.indexed(pk, np.random.default_rng(3)), L4.LAST)
    want = L4.expect(c)
    got = run(c)
    L4.check(got, want, "ref22")
    assert not (got["status"] == L4.OK).any()
    summed = got["status"] <= L4.UNCHECKED
    assert summed.sum() >= 14
    slab = c["batch"]["slab"].copy()
    run(c, True, slab=slab)
    again = run(c, slab=slab)
    assert (again["status"][summed] == L4.OK).all() and np.array_equal(again["status"][~summed], got["status"][~summed])
