"""pkt_edit_host through pktgpu.edit (no device): Packet::push / insert / pop / remove (packet.rs:117-164)
and to_vec over a host batch.  Every expected value comes from edit_cases.expect (pyref.parse and plain
Python list operations) or from the reference's own 22 packets; none comes from the code under test."""
import ctypes

import numpy as np
import pytest

import pktgpu
from pktgpu import _lib, gen, schema

import compare_cases as C
import edit_cases as E


def run(c, parsed):
    s = c["src"]
    dst = np.full(c["dst_len"], E.FILL, np.uint8)
    return pktgpu.edit(s["slab"], parsed, c["ops"], stride=s["stride"], n=s["n"], offsets=s["offsets"], lens=s["lens"],
                       select=c["select"], dst=dst, dst_offsets=c["dst_offsets"], slot=c["slot"])


@pytest.mark.parametrize("name", E.CASE_NAMES)
def test_cases(name):
    c, parsed, want = E.get(name)
    E.check(c, run(c, parsed), want, name)


def test_cases_are_not_trivial():
    """The table reaches every status, and the edits it names change what they should."""
    seen = set()
    for name in E.CASE_NAMES:
        seen |= set(E.get(name)[2][2].tolist())
    assert seen == {E.OK, E.SKIPPED, E.DEPTH, E.NO_ROOM}
    assert E.get("depth_insert")[2][2].tolist() == [E.OK, E.DEPTH, E.OK]
    assert E.get("depth_remove_insert")[2][2].tolist() == [E.OK, E.OK, E.OK]
    assert E.get("depth_insert_remove")[2][2].tolist() == [E.OK, E.DEPTH, E.OK]
    st = E.get("long_insert")[2][2]
    assert st[3] == E.NO_ROOM and (np.delete(st, 3) == E.OK).all()
    assert (E.get("long_strip")[2][2] == E.OK).all() and E.get("long_strip")[2][1][3] == 65531
    c, parsed, (outs, ln, st, ch) = E.get("c3_1025_strip0")
    tags = (parsed["hdr_type"] == schema.HDR_ID["Vlan"]).sum(0)
    assert set(tags.tolist()) == {0, 1, 2} and np.array_equal(ln, 128 - 4 * (tags > 0))
    c, parsed, (outs, ln, st, ch) = E.get("room_slot")
    assert (st[ln == 0] == E.NO_ROOM).all() and {99, 100, 60} == set(ln[ln > 0].tolist()) and st[-1] == E.NO_ROOM
    c, parsed, (outs, ln, st, ch) = E.get("room_offsets")
    assert st[5] == st[20] == st[33] == E.NO_ROOM and st[-1] == E.OK and ln[-1] == 100
    c, parsed, (outs, ln, st, ch) = E.get("select")
    for i in np.flatnonzero(c["select"] == 0):
        assert outs[i] == C.packets(c["src"])[i]
    c, parsed, (outs, ln, st, ch) = E.get("clamped")
    assert st[10] == E.SKIPPED and ln[9] in (66, 70)
    # the GRE packet's list is in Q2 order, so its to_vec is not its bytes
    c, parsed, (outs, ln, st, ch) = E.get("mixed_middle_insert")
    g = c["src"]["n"] - 2
    assert [schema.HDR_NAMES[t] for t in parsed["hdr_type"][:6, g]] == ["Ether", "IPv4", "GRE", "GRESequenceNum", "GREKey",
                                                                        "GREChksumOffset"]


def ref22():
    pk = [bytes(p.to_vec()) for p in gen.reference_22_packets()]
    return pk, C.indexed(pk, np.random.default_rng(3))


def edit_packets(src, ops, slot=512):
    parsed = E.parsed_of(src)
    dst, ln, st, ch = pktgpu.edit(src["slab"], parsed, ops, offsets=src["offsets"], lens=src["lens"], slot=slot)
    return [dst[slot * i:slot * i + int(ln[i])].tobytes() for i in range(src["n"])], ln, st, ch, parsed


def test_reference_identities():
    """The reference's own fixtures (tests/lib.rs:454-461, utils.rs:504-550): decap, IP-in-IP, encap."""
    pk, src = ref22()
    out = edit_packets(src, [("remove", 0)] * 4)[0]
    assert out[8] == pk[0] and out[6] == pk[1]                      # _vxlan_tcp / _vxlan_udp decap to _tcp / _udp
    assert edit_packets(src, [("remove", 0)] * 2)[0][12] == edit_packets(src, [("remove", 0)])[0][0] == pk[0][14:]
    out, ln, st, ch, parsed = edit_packets(src, E.encap_ops())
    assert out[0] == pk[8] and ln[0] == len(pk[8])
    assert [schema.HDR_NAMES[t] for t in ch["hdr_type"][:7, 0]] == ["Ether", "IPv4", "UDP", "Vxlan", "Ether", "IPv4", "TCP"]
    o = E.outer50()
    pushes = [("pop",)] * 4 + [("push", "Ether", o[0:14]), ("push", "IPv4", o[14:34]), ("push", "UDP", o[34:42]),
                               ("push", "Vxlan", o[42:50])]
    assert edit_packets(src, pushes)[0][0] == o + pk[0][54:]        # _tcp: three headers, so the list was emptied


def test_identity_is_to_vec():
    """nops = 0: every packet's to_vec (its list's slices, then the payload) and the parse's own chain."""
    pk, src = ref22()
    out, ln, st, ch, parsed = edit_packets(src, [])
    for i, p in enumerate(pk):
        status, hdrs, po, pl = E.pyref.parse(p)
        assert out[i] == b"".join(p[o:o + E.pyref.SIZES[nm]] for nm, o in hdrs) + p[po:po + pl] == p
    for k in ("status", "n_hdrs", "payload_off", "payload_len", "hdr_mask"):
        assert np.array_equal(ch[k], parsed[k]), k
    used = np.arange(schema.MAX_HDRS)[:, None] < parsed["n_hdrs"][None, :]
    assert np.array_equal(ch["hdr_type"][used], parsed["hdr_type"][used])
    assert np.array_equal(ch["hdr_off"][used], parsed["hdr_off"][used])


def _call(L, c, parsed, **kw):
    """pkt_edit_host on a case with some arguments replaced."""
    b, keep = pktgpu._host_batch(_lib, c["src"])
    arr, k, data = pktgpu._edit_ops(_lib, kw.get("ops", c["ops"]))
    po = _lib.PktOut()
    for col in ("status", "n_hdrs", "hdr_type", "hdr_off", "payload_off", "payload_len"):
        if col not in kw.get("drop", ()):
            setattr(po, col, parsed[col].ctypes.data)
    dst = np.full(c["dst_len"], E.FILL, np.uint8)
    n = c["src"]["n"]
    ln, st = np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    ch = {col: np.zeros(schema.column_shape(col, n), schema.column_dtype(col)) for col in E.CHAIN_COLS}
    oc = _lib.PktOut()
    for col, a in ch.items():
        setattr(oc, col, a.ctypes.data)
    want = kw.get("outputs", (True, True, True))
    rc = L.pkt_edit_host(ctypes.byref(kw.get("batch", b)), ctypes.byref(po), kw.get("arr", arr), kw.get("nops", k),
                         kw.get("data", data), kw.get("data_len", len(data)), None, None if kw.get("no_dst") else dst.ctypes.data,
                         dst.size, None, kw.get("slot", c["slot"]), ln.ctypes.data if want[0] else None,
                         st.ctypes.data if want[1] else None, ctypes.byref(oc) if want[2] else None)
    return rc, (dst, ln if want[0] else None, st if want[1] else None, ch if want[2] else None)


def test_null_outputs_and_argument_errors():
    L = _lib.load()
    assert L.pkt_sizeof_edit_op() == ctypes.sizeof(_lib.PktEditOp) == 8
    c, parsed, want = E.get("c3_65_strip0")
    for outputs in ((False, True, True), (True, False, True), (True, True, False), (False, False, False)):
        rc, got = _call(L, c, parsed, outputs=outputs)
        assert rc == 0
        E.check(c, got, want, str(outputs))
    ins = [("insert", "MPLS", E.MPLS)]
    bad_kind = (_lib.PktEditOp * 1)(_lib.PktEditOp(4, 0, 0, 0, 0))
    bad_type = (_lib.PktEditOp * 1)(_lib.PktEditOp(3, 22, 0, 0, 0))
    zero_type = (_lib.PktEditOp * 1)(_lib.PktEditOp(3, 0, 0, 0, 0))
    huge = _lib.PktBatch()
    huge.n, huge.stride = 1 << 32, 64
    for kw in (dict(ops=[("pop",)] * 9), dict(arr=bad_kind, nops=1), dict(arr=bad_type, nops=1, data=bytes(64), data_len=64),
               dict(arr=zero_type, nops=1, data=bytes(64), data_len=64), dict(ops=ins, data_len=3),
               dict(ops=ins, data=bytes(400), data_len=321), dict(slot=0), dict(batch=huge), dict(no_dst=True),
               dict(drop=("status",)), dict(drop=("hdr_off",)), dict(drop=("payload_len",)), dict(arr=None, nops=1)):
        rc, got = _call(L, c, parsed, **kw)
        assert rc == -1, kw
        assert (got[0] == E.FILL).all(), kw
    assert _call(L, c, parsed, ops=[("pop",)] * 8)[0] == 0
    assert _call(L, c, parsed, ops=[("insert", "STP", bytes(35))] * 8)[0] == 0
    empty = _lib.PktBatch()
    assert L.pkt_edit_host(ctypes.byref(empty), ctypes.byref(_lib.PktOut()), None, 0, None, 0, None, None, 0, None, 64, None,
                           None, None) == 0
    with pytest.raises(ValueError):
        pktgpu.edit(c["src"]["slab"], parsed, [("insert", "IPv4", bytes(19))], stride=128)
    with pytest.raises(ValueError):
        pktgpu.edit(c["src"]["slab"], parsed, [("pop",)] * 9, stride=128)


def test_chain_columns_that_are_not_a_parse():
    """Whatever the chain columns hold, the accesses stay inside the packet and the slot: random columns
    over small packets in an exactly sized slab run to the end, and every output is a string of slices
    of its packet no longer than its room."""
    rng = np.random.default_rng(5)
    n = 500
    slab = rng.integers(0, 256, 40 * n, dtype=np.uint8)
    parsed = dict(status=(rng.random(n) < 0.1).astype(np.uint8), n_hdrs=rng.integers(0, 40, n).astype(np.uint8),
                  hdr_type=rng.integers(0, 30, (16, n)).astype(np.uint8),
                  hdr_off=rng.choice([0, 3, 14, 30, 39, 40, 41, 1000, 65535], (16, n)).astype(np.uint16),
                  payload_off=rng.choice([0, 20, 39, 40, 50, 65535], n).astype(np.uint16),
                  payload_len=rng.choice([0, 1, 20, 40, 65535], n).astype(np.uint16))
    dst = np.full(200 * n, E.FILL, np.uint8)
    dst, ln, st, ch = pktgpu.edit(slab, parsed, [("remove", 1), ("insert", "MPLS", E.MPLS, 2)], stride=40, dst=dst, slot=200)
    assert set(st.tolist()) <= {E.OK, E.SKIPPED, E.NO_ROOM} and (ln <= 200).all() and (ln[st != E.OK] == 0).all()
    for i in range(n):
        assert (dst[200 * i + int(ln[i]):200 * (i + 1)] == E.FILL).all()
