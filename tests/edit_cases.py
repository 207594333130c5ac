"""Batches, op programs and expected results shared by test_edit_host.py and test_edit_device.py.

A case is a dict {"src", "ops", "select", "slot", "dst_offsets", "dst_len"}: a source batch over numpy
arrays (compare_cases.batch), the op tuples of pktgpu.edit, an optional selection mask and the
destination layout.  `expect(case)` computes pkt_edit_batch's outputs from its definition: pyref.parse
turns a packet's bytes into the list of (header name, slice) the reference's slow::parse builds, plain
Python list operations apply the program (Vec::pop / remove / insert / push, packet.rs:117-164) and the
slices are joined as to_vec joins them (385-392).  Nothing here calls pkt_edit_host or the device.
"""
import struct

import numpy as np

import pyref
from pktgpu import gen, schema

import compare_cases as C
from compare_cases import batch

OK, SKIPPED, DEPTH, NO_ROOM = 0, 1, 2, 3
FILL = 0x5A
STATUS_ID = {"OK": schema.OK, "TRUNCATED": schema.TRUNCATED, "DEPTH_LIMIT": schema.DEPTH_LIMIT}
CHAIN_COLS = ("status", "n_hdrs", "hdr_type", "hdr_off", "payload_off", "payload_len", "hdr_mask")


def hid(t):
    return schema.HDR_ID[t] if isinstance(t, str) else int(t)


def case(src, ops, slot, select=None, dst_offsets=None, dst_len=None):
    n = src["n"]
    if dst_len is None:
        dst_len = n * slot if dst_offsets is None else int(max(dst_offsets, default=0)) + slot
    return dict(src=src, ops=list(ops), select=None if select is None else np.asarray(select, np.uint8), slot=int(slot),
                dst_offsets=None if dst_offsets is None else np.asarray(dst_offsets, np.uint64), dst_len=int(dst_len))


def parsed_of(b):
    """The chain columns of a parse of b, by the Python model of the parser (slot-major)."""
    n = b["n"]
    cols = {c: np.zeros(schema.column_shape(c, n), schema.column_dtype(c)) for c in CHAIN_COLS}
    for i, p in enumerate(C.packets(b)):
        st, hdrs, po, pl = pyref.parse(p)
        cols["status"][i] = STATUS_ID[st]
        cols["n_hdrs"][i] = len(hdrs)
        for j, (name, o) in enumerate(hdrs):
            cols["hdr_type"][j, i] = schema.HDR_ID[name]
            cols["hdr_off"][j, i] = o
            cols["hdr_mask"][i] |= np.uint32(1 << schema.HDR_ID[name])
        cols["payload_off"][i], cols["payload_len"][i] = po, pl
    return cols


def apply(L, ops):
    """The program on the list L of (type id, bytes), in place -> False once the list passed 16 entries."""
    for op in ops:
        kind = op[0]
        if kind == "pop":
            if L:
                L.pop()
        elif kind == "remove":
            if op[1] < len(L):
                del L[op[1]]
        elif kind == "remove_hdr":
            at = [j for j, e in enumerate(L) if e[0] == hid(op[1])]
            occ = op[2] if len(op) > 2 else 0
            if occ < len(at):
                del L[at[occ]]
        elif kind in ("insert", "push"):
            t = hid(op[1])
            e = (t, bytes(op[2])[:schema.HDR_SIZES[t]])
            index = len(L) if kind == "push" else (op[3] if len(op) > 3 else 0)
            L.insert(len(L) if index == 0xFF else min(index, len(L)), e)
            if len(L) > schema.MAX_HDRS:
                return False
        else:
            raise ValueError(kind)
    return True


def rooms(c):
    """(o_i, room_i) of every destination packet."""
    out = []
    for i in range(c["src"]["n"]):
        o = int(c["dst_offsets"][i]) if c["dst_offsets"] is not None else i * c["slot"]
        out.append((o, 0 if o >= c["dst_len"] else min(c["slot"], c["dst_len"] - o)))
    return out


def expect(c):
    """(bytes per packet or None, out_len, status, chain columns) of the case, from the definition."""
    n = c["src"]["n"]
    outs, out_len, status = [], np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    chain = {k: np.zeros(schema.column_shape(k, n), schema.column_dtype(k)) for k in CHAIN_COLS}
    for i, (p, (o, room)) in enumerate(zip(C.packets(c["src"]), rooms(c))):
        st, hdrs, po, pl = pyref.parse(p)
        outs.append(None)
        if st != "OK":
            status[i], chain["status"][i] = SKIPPED, STATUS_ID[st]
            continue
        L = [(schema.HDR_ID[name], p[at:at + pyref.SIZES[name]]) for name, at in hdrs]
        if not apply(L, c["ops"] if c["select"] is None or c["select"][i] else ()):
            status[i], chain["status"][i] = DEPTH, schema.DEPTH_LIMIT
            continue
        v = b"".join(e[1] for e in L) + p[po:po + pl]
        if len(v) > room or len(v) > 65535:
            status[i], chain["status"][i] = NO_ROOM, schema.TRUNCATED
            continue
        outs[i], out_len[i] = v, len(v)
        chain["n_hdrs"][i] = len(L)
        pos = 0
        for k, (t, raw) in enumerate(L):
            chain["hdr_type"][k, i], chain["hdr_off"][k, i] = t, pos
            chain["hdr_mask"][i] |= np.uint32(1 << t)
            pos += len(raw)
        chain["payload_off"][i], chain["payload_len"][i] = pos, pl
    return outs, out_len, status, chain


def check(c, got, want, label=""):
    """got = (dst, out_len, status, chain) as numpy, any of the last three None when not asked for."""
    dst, out_len, status, chain = got
    outs, w_len, w_status, w_chain = want
    if status is not None:
        bad = np.flatnonzero(status != w_status)
        assert bad.size == 0, (label, "status", bad[:8], status[bad[:8]], w_status[bad[:8]])
    if out_len is not None:
        bad = np.flatnonzero(out_len != w_len)
        assert bad.size == 0, (label, "out_len", bad[:8], out_len[bad[:8]], w_len[bad[:8]])
    assert dst.size == c["dst_len"]
    untouched = np.ones(dst.size, bool)
    for i, ((o, room), v) in enumerate(zip(rooms(c), outs)):
        if v is None:
            continue
        assert dst[o:o + len(v)].tobytes() == v, (label, "bytes of packet", i, len(v))
        untouched[o:o + len(v)] = False
    bad = np.flatnonzero(untouched & (dst != FILL))
    assert bad.size == 0, (label, "bytes written outside the packets", bad[:8])
    if chain is not None:
        for k in ("status", "n_hdrs", "payload_off", "payload_len", "hdr_mask"):
            bad = np.flatnonzero(chain[k] != w_chain[k])
            assert bad.size == 0, (label, k, bad[:8], chain[k][bad[:8]], w_chain[k][bad[:8]])
        used = np.arange(schema.MAX_HDRS)[:, None] < w_chain["n_hdrs"][None, :]
        for k in ("hdr_type", "hdr_off"):
            bad = np.argwhere(used & (chain[k] != w_chain[k]))
            assert bad.size == 0, (label, k, bad[:8])


# ------------------------------------------------------------------ packets
M1, M2 = "00:01:02:03:04:05", "00:06:07:08:09:0a"
MPLS = bytes([0x12, 0x34, 0x51, 0x40])
VLAN7 = bytes([0x60, 0x07, 0x08, 0x00])


def eth(etype):
    return gen.to_mac_bytes(M1) + gen.to_mac_bytes(M2) + struct.pack(">H", etype)


def tagged(ntags, payload, last=0x9999):
    """Ether, ntags Vlan tags and a payload behind an etype the walk accepts at."""
    tags = b"".join(struct.pack(">HH", 100 + t, 0x8100 if t + 1 < ntags else last) for t in range(ntags))
    return eth(0x8100 if ntags else last) + tags + bytes(payload)


def rnd_bytes(rng, k):
    return rng.integers(0, 256, k, dtype=np.uint8).tobytes()


def sixteen_headers():
    """Ether, 13 Vlan tags, IPv4, TCP: a parse of exactly PKT_MAX_HDRS headers."""
    ip = bytes(gen.reference_22_packets()[0].to_vec())[14:]
    return tagged(13, ip, last=0x0800)


def gre_options():
    """Ether / IPv4 / GRE with checksum, key and sequence number (list order Q2: GRE, Seq, Key, Chksum)."""
    inner = gen.reference_22_packets()[0].clone()
    inner.remove(0)
    return bytes(gen.create_gre_packet(M1, M2, False, 10, 3, 5, "192.168.0.199", "192.168.0.1", 0, 64, 0, 0x4000, [], 1, 0,
                                       1, 1, 0, 0, 0, 0x1234, 0, 77, 88, b"", inner).to_vec())


def outer50():
    """The first 50 bytes of the reference's _vxlan_tcp: Ether, IPv4, UDP, Vxlan."""
    return bytes(gen.reference_22_packets()[8].to_vec())[:50]


def encap_ops(o=None):
    o = outer50() if o is None else o
    return [("insert", "Vxlan", o[42:50]), ("insert", "UDP", o[34:42]), ("insert", "IPv4", o[14:34]), ("insert", "Ether", o[0:14])]


# ------------------------------------------------------------------ cases
C3_PROGRAMS = {"strip0": [("remove_hdr", "Vlan", 0)], "strip1": [("remove_hdr", "Vlan", 1)], "pop": [("pop",)],
               "remove1": [("remove", 1)]}
TILING_N = (1, 63, 64, 65, 1025)


def tiling(n, prog):
    return case(batch(gen.gen_c3(n, seed=7 + n), stride=128), C3_PROGRAMS[prog], slot=128)


ALIGN_LENS = [0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65]


def alignment(kind):
    """Every (source offset mod 16, destination offset mod 16) at every output length of ALIGN_LENS that
    the edit can give.  "strip": Ether / Vlan / payload with the tag removed, bytes [0,14) + [18, len), for
    the lengths from 15 (a shorter output has no Ether header to keep).  "insert": Ether / payload with the
    Ether header removed and four constant bytes (MPLS) inserted, the constant and one segment, from 15 too.
    "small": lengths 0 and 1, by Ether / Vlan / Vlan / payload with all three headers removed."""
    rng = np.random.default_rng(61)
    lens = [0, 1] if kind == "small" else [ln for ln in ALIGN_LENS if ln >= 15]
    ops = {"strip": [("remove_hdr", "Vlan", 0)], "insert": [("remove", 0), ("insert", "MPLS", MPLS)],
           "small": [("remove", 0)] * 3}[kind]
    pk, al = [], []
    for pair in range(256):
        for ln in lens:
            pk.append(tagged(1, rnd_bytes(rng, ln - 14)) if kind == "strip" else
                      tagged(0, rnd_bytes(rng, ln - 4)) if kind == "insert" else tagged(2, rnd_bytes(rng, ln)))
            al.append(pair)
    src = C.indexed(pk, rng, align=[a >> 4 for a in al])
    offs = [96 * i + 16 + (a & 15) for i, a in enumerate(al)]
    return case(src, ops, slot=66, dst_offsets=offs, dst_len=96 * len(pk) + 64)


def long_among_short(kind):
    """One 65535-byte packet and packets of 4095, 4096 and 4097 bytes among 64-byte ones, all inside one
    wave's 64 packets (and a second wave of short ones), Ether / Vlan / payload.  The inserted four bytes
    take the 65535-byte packet, and only it, past 65535."""
    rng = np.random.default_rng(67)
    lens = [64] * 100
    for at, ln in ((3, 65535), (10, 4095), (11, 4096), (12, 4097), (40, 4096), (63, 4097), (64, 4095)):
        lens[at] = ln
    pk = [tagged(1, rnd_bytes(rng, ln - 18)) for ln in lens]
    offs, pos = [], 0
    for ln in lens:
        offs.append(pos + int(rng.integers(0, 16)))
        pos = (offs[-1] + ln + 4 + 15) // 16 * 16
    ops = [("remove_hdr", "Vlan", 0)] if kind == "strip" else [("insert", "MPLS", MPLS, 1)]
    return case(C.indexed(pk, rng), ops, slot=65535, dst_offsets=offs, dst_len=pos)


def mixed(kind):
    """compare_cases.mixed_packets() (C3, the 22 reference packets, IPv6, a long and a truncated packet),
    a GRE packet with three options and the 16-header packet."""
    rng = np.random.default_rng(71)
    pk = C.mixed_packets() + [gre_options(), sixteen_headers()]
    o = outer50()
    ops = {
        # types absent from some packets, and the second occurrence
        "absent": [("remove_hdr", "Vlan", 1), ("remove_hdr", "Vxlan", 0), ("remove_hdr", "IPv6", 0), ("remove_hdr", "IPv4", 1),
                   ("remove_hdr", "GREKey", 0)],
        "middle_insert": [("insert", "MPLS", MPLS, 2)],
        "eight": [("pop",), ("remove", 1), ("insert", "Vlan", VLAN7, 1), ("push", "UDP", o[34:42]), ("remove_hdr", "IPv4", 0),
                  ("insert", "Ether", o[0:14]), ("remove_hdr", "Vlan", 1), ("insert", "GRE", bytes([0, 0, 8, 0]), 5)],
        "empty_then_push": [("pop",)] * 4 + [("push", "Ether", o[0:14]), ("push", "IPv4", o[14:34]), ("push", "UDP", o[34:42]),
                                             ("push", "Vxlan", o[42:50])],
    }[kind]
    src = C.indexed(pk, rng)
    offs, pos = [], 0
    for p in pk:
        offs.append(pos + int(rng.integers(0, 16)))
        pos = (offs[-1] + len(p) + 64 + 15) // 16 * 16
    return case(src, ops, slot=5200, dst_offsets=offs, dst_len=pos)


def depth(kind):
    """The 16-header packet between two C3 packets: one insert is DEPTH, a remove before the insert is
    OK, insert then remove is DEPTH."""
    rng = np.random.default_rng(73)
    c3 = gen.gen_c3(2, seed=5)
    pk = [c3[0].tobytes(), sixteen_headers(), c3[1].tobytes()]
    ops = {"insert": [("insert", "MPLS", MPLS, 3)], "remove_insert": [("remove", 1), ("insert", "MPLS", MPLS, 3)],
           "insert_remove": [("insert", "MPLS", MPLS, 3), ("remove", 1)]}[kind]
    return case(C.indexed(pk, rng), ops, slot=256)


def room(kind):
    """Outputs one byte over the slot, exactly at it and under it; a destination offset at and past
    dst_len; dst_len cutting the last slot."""
    rng = np.random.default_rng(79)
    pk = [tagged(1, rnd_bytes(rng, ln - 18)) for ln in [103, 104, 105, 64, 104, 105, 103, 104] * 9]
    src = C.indexed(pk, rng)
    ops = [("remove_hdr", "Vlan", 0)]  # 99, 100, 101, 60
    if kind == "slot":
        return case(src, ops, slot=100, dst_len=100 * len(pk) - 1)      # the last packet (100 bytes) has room 99
    n = len(pk)
    offs = [128 * i + (i % 16) for i in range(n)]
    dst_len = offs[-1] + 100                                            # exactly the room of the last one's 100 bytes
    offs[5], offs[20], offs[33] = dst_len, dst_len + 1000, 1 << 40      # room 0
    return case(src, ops, slot=100, dst_offsets=offs, dst_len=dst_len)


def selected():
    rng = np.random.default_rng(83)
    n = 300
    return case(batch(gen.gen_c3(n, seed=11), stride=128), [("remove_hdr", "Vlan", 0), ("insert", "MPLS", MPLS, 1)], slot=128,
                select=rng.integers(0, 2, n))


def clamped():
    """A fixed-stride batch whose last packets run past slab_len: their parse is TRUNCATED or their
    payload is cut at the slab end."""
    a = gen.gen_c3(10, seed=13).reshape(-1)[:128 * 9 + 70]
    return case(batch(a, stride=128, n=11), [("remove_hdr", "Vlan", 0)], slot=128)


def all_builders():
    cs = {f"c3_{n}_{prog}": (lambda n=n, prog=prog: tiling(n, prog)) for n in TILING_N for prog in C3_PROGRAMS}
    for k in ("strip", "insert", "small"):
        cs[f"align_{k}"] = lambda k=k: alignment(k)
    for k in ("strip", "insert"):
        cs[f"long_{k}"] = lambda k=k: long_among_short(k)
    for k in ("absent", "middle_insert", "eight", "empty_then_push"):
        cs[f"mixed_{k}"] = lambda k=k: mixed(k)
    for k in ("insert", "remove_insert", "insert_remove"):
        cs[f"depth_{k}"] = lambda k=k: depth(k)
    for k in ("slot", "offsets"):
        cs[f"room_{k}"] = lambda k=k: room(k)
    cs["select"] = selected
    cs["clamped"] = clamped
    return cs


CASE_NAMES = list(all_builders())
_CASES = {}


def get(name):
    """name -> (case, parsed columns of its source, expected): built once and shared; nothing may change them."""
    if name not in _CASES:
        c = all_builders()[name]()
        _CASES[name] = (c, parsed_of(c["src"]), expect(c))
    return _CASES[name]
