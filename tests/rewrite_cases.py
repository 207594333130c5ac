"""The yardstick and the case builders of the field getters, setters and checksum refresh (pkt_extract_fields,
pkt_set_fields, pkt_set_fields_csum, pkt_ipv4_update_checksum, pkt_ipv4_checksum_batch, pkt_broadcast):
tests/test_rewrite_cases.py (CPU, against the C oracle) and tests/test_rewrite_device.py (the kernels).

The yardstick works on Python integers and `bytes` and shares nothing with oracle/pkt_oracle.c or the kernels; it
is written from include/pktgpu.h and DESIGN's quirk list:
  header lookup   the `occurrence`-th entry of `hdr_type` among the first min(n_hdrs, 16) slots; absent: getter 0,
                  found 0, setter and refresh leave the packet alone.
  getter          the header as ONE big-endian integer, bits [start..=end] numbered MSB-first; wider than 64 bits
                  (Q8): the low 64 bits of the field, then the low (w mod 64) of those (all 64 when w mod 64 == 0).
  setter          the low min(w, 64) bits of the value into the field, the field's bits above them 0; in spec order.
  checksum        the nine 16-bit words other than bytes 10-11, s = ((s >> 16) + s) & 0xFFFF ONCE (Q1), complement;
                  rfc1071() beside it only counts the inputs on which the two differ.
  extents         compare_cases.extents (pkt_batch_t's rules).

A case is a dict {"batch", "chain", "specs", "values", "floor"}: a batch over numpy arrays, chain columns, specs
(type id, occurrence, start, end), one uint64 array per spec (the setters' values) and a floor: a function that
asserts, from the layout and the yardstick alone, that the case reaches the path it is built for.  TABLE lists
(name, calls); case(name) builds a case once, expected(name, call) its result once; nothing may change them.
Calls: "get", "set", "set+csum0", "set+csum1", "update0", "update1".
"""
import functools

import numpy as np

from pktgpu import fields as F
from pktgpu import gen, schema

import compare_cases as C
import flow_cases as FL
import l4_cases as L4

MAX_HDRS = schema.MAX_HDRS
SIZE = schema.HDR_SIZES
M1, M2 = L4.M1, L4.M2
GET, SET, SET0, SET1, UPD0, UPD1 = "get", "set", "set+csum0", "set+csum1", "update0", "update1"
LAYOUTS = ["s64", "s48", "s128", "gaps", "packed", "pcap"]
SHAPES = [1, 63, 64, 65, 255, 256, 257, 1025]


def T(name):
    return schema.HDR_ID[name]


def fld(hdr, field, occ=0):
    s, e = F.FIELDS[T(hdr)][field]
    return (T(hdr), occ, s, e)


# ------------------------------------------------------------------ the yardstick
def chain_rows(ch, i):
    """[(type, offset)] of packet i: the first min(n_hdrs, 16) slots."""
    return [(int(ch["hdr_type"][j, i]), int(ch["hdr_off"][j, i])) for j in range(min(int(ch["n_hdrs"][i]), MAX_HDRS))]


def lookup(rows, t, occ):
    """Offset of the occ-th header of type t in the list, or None."""
    hits = [o for ty, o in rows if ty == t]
    return hits[occ] if occ < len(hits) else None


def get_field(hdr, s, e):
    w = e - s + 1
    v = (int.from_bytes(hdr, "big") >> (8 * len(hdr) - 1 - e)) & ((1 << w) - 1)
    if w > 64:
        v &= (1 << 64) - 1
        if w % 64:
            v &= (1 << (w % 64)) - 1
    return v


def set_field(hdr, s, e, value):
    w, sh = e - s + 1, 8 * len(hdr) - 1 - e
    h = int.from_bytes(hdr, "big") & ~(((1 << w) - 1) << sh)
    return (h | ((int(value) & ((1 << min(w, 64)) - 1)) << sh)).to_bytes(len(hdr), "big")


def words9(h):
    return sum((h[k] << 8) | h[k + 1] for k in range(0, 20, 2) if k != 10)


def q1(h):
    """Packet::ipv4_checksum: one fold that drops the carry of hi + lo (Q1)."""
    s = words9(h)
    s = ((s >> 16) + s) & 0xFFFF
    return ~s & 0xFFFF


def rfc1071(h):
    s = words9(h)
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return ~s & 0xFFFF


def pin_yardstick():
    """RFC 1071's own example for the plain fold, a hand-worked Q1 case, and the Q8 widths on a known pattern."""
    assert rfc1071(bytes.fromhex("0001f203f4f5f6f7") + bytes(12)) == 0x220D == q1(bytes.fromhex("0001f203f4f5f6f7") + bytes(12))
    h = bytes.fromhex("ffffffff") + bytes(16)             # 0x1FFFE: hi + lo = 0xFFFF, no carry lost
    assert q1(h) == rfc1071(h) == 0
    h = bytes.fromhex("ffffffff0002") + bytes(14)         # 0x20000: hi + lo = 2 both ways
    assert q1(h) == rfc1071(h) == 0xFFFD
    h = bytes.fromhex("ffffffff0001") + bytes(4) + b"\xab\xcd" + bytes(8)  # 0x1FFFF: Q1 0 -> ffff, RFC 1 -> fffe
    assert q1(h) == 0xFFFF and rfc1071(h) == 0xFFFE
    p = bytes(range(1, 17))
    assert get_field(p, 0, 127) == int.from_bytes(p[8:], "big") and get_field(p, 0, 71) == 0x09
    assert get_field(p, 4, 11) == 0x10 and get_field(p, 7, 7) == 1 and get_field(p, 56, 127) == 0x10
    assert set_field(b"\xff" * 16, 0, 127, 0x0123456789ABCDEF) == bytes(8) + (0x0123456789ABCDEF).to_bytes(8, "big")
    assert set_field(bytes(3), 7, 8, 0xFFFFFFFFFFFFFFFF) == b"\x01\x80\x00"


def _ctx(c):
    b = c["batch"]
    return b, c["chain"], [o for o, _ in C.extents(b)]


def expect_get(c, specs=None):
    """(values, found): one uint64 and one uint8 array per spec."""
    b, ch, offs = _ctx(c)
    specs = c["specs"] if specs is None else specs
    slab = b["slab"].tobytes()
    vals = [np.zeros(b["n"], np.uint64) for _ in specs]
    found = [np.zeros(b["n"], np.uint8) for _ in specs]
    for i in range(b["n"]):
        rows = chain_rows(ch, i)
        for k, (t, occ, s, e) in enumerate(specs):
            ho = lookup(rows, t, occ)
            if ho is not None:
                hdr = slab[offs[i] + ho:offs[i] + ho + SIZE[t]]
                assert len(hdr) == SIZE[t], "a header past the slab's end"
                vals[k][i], found[k][i] = get_field(hdr, s, e), 1
    return vals, found


def expect_set(c, csum=None, specs=None, values=None):
    """The slab after the setters in order and then, with csum = occ, the refresh of that IPv4 header."""
    b, ch, offs = _ctx(c)
    specs = c["specs"] if specs is None else specs
    values = c["values"] if values is None else values
    slab = bytearray(b["slab"].tobytes())
    for i in range(b["n"]):
        rows = chain_rows(ch, i)
        for k, (t, occ, s, e) in enumerate(specs):
            ho = lookup(rows, t, occ)
            if ho is not None:
                a = offs[i] + ho
                assert a + SIZE[t] <= len(slab)
                slab[a:a + SIZE[t]] = set_field(bytes(slab[a:a + SIZE[t]]), s, e, values[k][i])
        if csum is not None:
            ho = lookup(rows, T("IPv4"), csum)
            if ho is not None:
                a = offs[i] + ho
                slab[a + 10:a + 12] = q1(bytes(slab[a:a + 20])).to_bytes(2, "big")
    return np.frombuffer(bytes(slab), np.uint8)


def expect_update(c, occ):
    return expect_set(c, csum=occ, specs=[], values=[])


def expect_call(c, call):
    if call == GET:
        return expect_get(c)
    if call.startswith("update"):
        return expect_update(c, int(call[-1]))
    return expect_set(c, csum=int(call[-1]) if "csum" in call else None)


def touched(c, i, csum=None):
    """Packet-relative (first, last) byte of every field packet i's chain lets the case set (refresh included)."""
    rows = chain_rows(c["chain"], i)
    out = []
    for t, occ, s, e in c["specs"]:
        ho = lookup(rows, t, occ)
        if ho is not None:
            out.append((ho + s // 8, ho + e // 8))
    if csum is not None and lookup(rows, T("IPv4"), csum) is not None:
        ho = lookup(rows, T("IPv4"), csum)
        out.append((ho + 10, ho + 11))
    return out


# ------------------------------------------------------------------ packets
SCRAMBLE = {"Ether": [(0, 12)], "IPv4": [(4, 6), (8, 9), (10, 20)], "IPv6": [(8, 40)], "UDP": [(0, 2), (6, 8)],
            "TCP": [(0, 2), (4, 12)], "ARP": [(8, 28)], "MPLS": [(0, 2), (3, 4)], "Vxlan": [(4, 7)]}
_SCR = {schema.HDR_ID[k]: v for k, v in SCRAMBLE.items()}


def scramble(p, rng):
    """`p` with random bytes in the fields that do not steer the parse (addresses, ids, checksums, ports)."""
    hd = L4.hdrs_of(p)
    q = bytearray(p)
    for t, o in hd:
        for lo, hi in _SCR.get(t, ()):
            q[o + lo:o + hi] = L4.rnd(rng, hi - lo)
    assert L4.hdrs_of(bytes(q)) == hd
    return bytes(q)


def udp4(rng, pay=0, vlans=0):
    return scramble(L4.pkt("UDP", vlans=vlans, payload=L4.rnd(rng, pay)), rng)


def v6tcp(rng, pay=0):
    return scramble(L4.pkt("TCP", v6=True, vlans=1, payload=L4.rnd(rng, pay)), rng)


def arp(rng):
    return scramble(bytes(gen.create_arp_packet(M1, M2, False, 0, 0, 1, M1, M2, "10.0.0.1", "10.0.0.2", b"").to_vec()), rng)


def _tags(k, then):
    return [gen.vlan(1, 0, 20 + j, 0x8100 if j + 1 < k else then) for j in range(k)]


def vx(rng, a=0, b=0, l4="TCP", pay=0):
    """Ether / a x Vlan / IPv4 / UDP / Vxlan / Ether / b x Vlan / IPv4 / l4: the inner IPv4 at 64 + 4 (a + b)."""
    size = (20 if l4 == "TCP" else 8) + pay
    inner = [gen.ethernet(M2, M1, 0x8100 if b else 0x0800)] + _tags(b, 0x0800)
    inner.append(gen.ipv4(5, 0, 7, 64, 0x4000, 6 if l4 == "TCP" else 17, "10.1.1.1", "10.2.2.2", 20 + size))
    inner.append(gen.tcp(1000, 2000, 100, 101, 5, 0, 2, 8192, 0, 0) if l4 == "TCP" else gen.udp(1000, 2000, size))
    ilen = sum(len(h.data) for h in inner) + pay
    p = gen.Packet()
    for h in [gen.ethernet(M1, M2, 0x8100 if a else 0x0800)] + _tags(a, 0x0800) + \
            [gen.ipv4(5, 0, 9, 64, 0x4000, 17, "192.168.0.199", "192.168.0.1", 36 + ilen), gen.udp(5555, gen.VXLAN_PORT, 16 + ilen),
             gen.vxlan_hdr(77)] + inner:
        p.push(h)
    p.set_payload(L4.rnd(rng, pay))
    out = scramble(p.to_vec(), rng)
    assert [t for t, _ in L4.hdrs_of(out)].index(T("Vxlan")) == 3 + a
    return out


def vx64(rng):
    """Ether / IPv4 / UDP / Vxlan / Ether, 64 bytes: the inner etype is the slot's last two bytes."""
    p = gen.Packet()
    for h in (gen.ethernet(M1, M2, 0x0800), gen.ipv4(5, 0, 9, 64, 0x4000, 17, "192.168.0.199", "192.168.0.1", 50),
              gen.udp(5555, gen.VXLAN_PORT, 30), gen.vxlan_hdr(77), gen.ethernet(M2, M1, 0x88B5)):
        p.push(h)
    out = scramble(p.to_vec(), rng)
    assert len(out) == 64 and len(L4.hdrs_of(out)) == 5
    return out


def mpls_pkt(rng, k):
    """Ether / k x MPLS (bottom of stack on the last but one: the parser takes one more label after it) / IPv4."""
    p = gen.Packet()
    p.push(gen.ethernet(M1, M2, 0x8847))
    for j in range(k):
        p.push(gen.mpls_raw(1000 + j, 0, 1 if j == k - 2 else 0, 64))
    p.push(gen.ipv4(5, 0, 9, 64, 0x4000, 253, "10.9.9.1", "10.9.9.2", 20))
    out = scramble(p.to_vec(), rng)
    hd = L4.hdrs_of(out)
    assert [t for t, _ in hd] == [T("Ether")] + [T("MPLS")] * k + [T("IPv4")], hd
    return out


def eth_ip(rng, vlans=0):
    """Ether / IPv4 with nothing after it: the IPv4 header is the packet's last 20 bytes."""
    p = gen.Packet()
    p.push(gen.ethernet(M1, M2, 0x8100 if vlans else 0x0800))
    for h in _tags(vlans, 0x0800):
        p.push(h)
    p.push(gen.ipv4(5, 0, 9, 64, 0x4000, 253, "10.9.9.1", "10.9.9.2", 20))
    return scramble(p.to_vec(), rng)


KINDS = {
    "s64": [lambda r: udp4(r, int(r.integers(0, 23))), arp, lambda r: v6tcp(r)[:64]],
    "s48": [lambda r: udp4(r, int(r.integers(0, 7))), arp, lambda r: udp4(r)[:21], lambda r: L4.rnd(r, 5)],
    "s128": [lambda r: udp4(r, int(r.integers(0, 60))), lambda r: v6tcp(r, int(r.integers(0, 40))), arp,
             lambda r: vx(r, int(r.integers(0, 2)), int(r.integers(0, 2)), "TCP", int(r.integers(0, 9))),
             lambda r: L4.rnd(r, 5), lambda r: udp4(r)[:21]],
}
KINDS["gaps"] = KINDS["packed"] = KINDS["pcap"] = [
    lambda r: udp4(r, int(r.integers(0, 90))), lambda r: v6tcp(r, int(r.integers(0, 120))), arp,
    lambda r: vx(r, int(r.integers(0, 3)), int(r.integers(0, 3)), ("TCP", "UDP")[int(r.integers(0, 2))], int(r.integers(0, 40))),
    lambda r: L4.rnd(r, 5), lambda r: udp4(r)[:21]]


def mix(layout, n, rng):
    ks = KINDS[layout]
    return [ks[(i + i // len(ks)) % len(ks)](rng) for i in range(n)]


def lay(layout, pkts, rng, align=None):
    """The packets in one of the six layouts."""
    if layout in ("s64", "s48", "s128"):
        st = int(layout[1:])
        assert all(len(p) <= st for p in pkts)
        slab = np.frombuffer(b"".join(p + L4.rnd(rng, st - len(p)) for p in pkts), np.uint8)
        return C.batch(slab, stride=st) if layout == "s64" else C.batch(slab, lens=[len(p) for p in pkts], stride=st)
    if layout == "gaps":
        return C.indexed(pkts, rng, align=align)
    if layout == "packed":
        offs = np.cumsum([0] + [len(p) for p in pkts[:-1]])
        return C.batch(np.frombuffer(b"".join(pkts), np.uint8), offs, [len(p) for p in pkts])
    raw = gen.pcap_bytes(pkts)
    offs, lens = gen.pcap_index_py(raw)
    return C.batch(np.frombuffer(raw, np.uint8), offs, lens)


def rand_values(rng, n, k, ones=False):
    if ones:
        return [np.full(n, 0xFFFFFFFFFFFFFFFF, np.uint64) for _ in range(k)]
    return [rng.integers(0, 2 ** 64, n, dtype=np.uint64) for _ in range(k)]


def make(b, specs, rng, chain=None, floor=None, ones=False, **extra):
    return dict(batch=b, chain=L4.chain_of(b) if chain is None else chain, specs=list(specs),
                values=rand_values(rng, b["n"], len(specs), ones), floor=floor, **extra)


def shifts(c):
    return [o % 16 for o, _ in C.extents(c["batch"])]


def present(c):
    """(packet, spec index, header offset) of every spec whose header packet i's chain holds."""
    out = []
    for i in range(c["batch"]["n"]):
        rows = chain_rows(c["chain"], i)
        for k, (t, occ, s, e) in enumerate(c["specs"]):
            ho = lookup(rows, t, occ)
            if ho is not None:
                out.append((i, k, ho))
    return out


# ------------------------------------------------------------------ a. shapes
SHAPE_SPECS = [fld("Ether", "src"), fld("Vlan", "vid"), fld("IPv4", "ttl"), fld("IPv4", "dst", 1), fld("IPv6", "src"),
               fld("UDP", "dst"), fld("TCP", "seq_no"), fld("ARP", "target_proto_addr"), fld("IPv4", "flags")]


def shapes(layout, n):
    rng = np.random.default_rng(1000 * LAYOUTS.index(layout) + n)
    c = make(lay(layout, mix(layout, n, rng), rng), SHAPE_SPECS, rng)

    def floor():
        nh = c["chain"]["n_hdrs"]
        if n >= 63:
            assert (nh == 0).sum() >= n // 8 and (nh >= 3).sum() >= n // 5
            hit = {k for _, k, _ in present(c)}
            assert hit >= ({0, 2, 5, 7, 8} if layout in ("s64", "s48") else set(range(9))), hit
    c["floor"] = floor
    return c


# ------------------------------------------------------------------ b. window sweep
SWEEP_SPECS = [fld("IPv4", "dst", 1), fld("IPv4", "ttl", 1), fld("IPv4", "header_checksum", 1), fld("UDP", "src", 1),
               fld("UDP", "dst", 1), fld("TCP", "src"), fld("TCP", "dst")]


TTL_SPECS = [fld("IPv4", "ttl", 1), fld("IPv4", "ttl"), fld("Ether", "src", 1)]


def sweep_in_window():
    """SWEEP_SPECS' inner `dst` ends past window byte 80 in every packet, so those packets are all set outside the
    window.  With the inner `ttl` (header byte 8) as the deepest setter, the packets whose header starts at window
    byte 61..71 stay in window mode while the header straddles byte 80: the refresh reads the header from both
    sides and sends each checksum byte to its own side."""
    c = dict(sweep("gaps"))
    c["specs"] = TTL_SPECS
    c["values"] = c["values"][:3]

    def floor():
        sh = shifts(c)
        x = []
        for i in range(c["batch"]["n"]):
            if max(sh[i] + hi for _, hi in touched(c, i)) < 80:   # every setter inside the window
                x.append(sh[i] + lookup(chain_rows(c["chain"], i), T("IPv4"), 1))
        strad = [v for v in x if v < 80 <= v + 19]
        assert any(v + 11 < 80 for v in strad) and any(v + 10 == 79 for v in strad) and any(v + 10 >= 80 for v in strad)
        assert 0 < len(x) < c["batch"]["n"]   # the packets with a deeper header leave window mode
    c["floor"] = floor
    return c


def sweep(layout):
    rng = np.random.default_rng(77)
    combos = [(a, b, l4) for a in range(3) for b in range(3) for l4 in ("TCP", "UDP")]
    if layout == "gaps":
        pkts, al = [], []
        for s in range(16):
            for a, b, l4 in combos:
                pkts.append(vx(rng, a, b, l4, int(rng.integers(0, 20))))
                al.append(s)
        c = make(lay("gaps", pkts, rng, al), SWEEP_SPECS, rng)
    else:
        c = make(lay("s128", [vx(rng, a, b, l4, int(rng.integers(0, 8))) for a, b, l4 in combos * 4], rng), SWEEP_SPECS, rng)

    def floor():
        sh = shifts(c)
        ip = [lookup(chain_rows(c["chain"], i), T("IPv4"), 1) for i in range(c["batch"]["n"])]
        assert sorted(set(ip)) == [64, 68, 72, 76, 80]
        if layout == "gaps":
            assert sorted(set(sh)) == list(range(16))
            last = {sh[i] + ho + c["specs"][k][3] // 8 for i, k, ho in present(c)}
            assert set(range(72, 88)) <= last, sorted(last)
            x = [s + o for s, o in zip(sh, ip)]
            strad = [v for v in x if v < 80 <= v + 19]
            assert any(v + 11 < 80 for v in strad) and any(v + 10 == 79 for v in strad) and any(v + 10 >= 80 for v in strad)
        else:
            assert set(sh) == {0}
    c["floor"] = floor
    return c


def narrow(layout):
    """4-chunk windows: the field that ends in the slot's (s64) or the packet's (s48, byte 41) last byte."""
    rng = np.random.default_rng(78)
    if layout == "s64":
        specs = [fld("Ether", "etype", 1), fld("Ether", "src", 1), fld("Vxlan", "vni"), fld("IPv4", "dst"), fld("Ether", "dst")]
        c = make(lay("s64", [vx64(rng) for _ in range(70)], rng), specs, rng)
        end = 63
    else:
        specs = [fld("UDP", "checksum"), fld("ARP", "target_proto_addr"), fld("IPv4", "ttl"), fld("Ether", "dst")]
        c = make(lay("s48", [udp4(rng) if i % 3 else arp(rng) for i in range(70)], rng), specs, rng)
        end = 41

    def floor():
        b = c["batch"]
        assert b["offsets"] is None and b["stride"] <= 64 and b["stride"] % 16 == 0
        for i in range(b["n"]):
            assert max(hi for _, hi in touched(c, i)) == end and min(lo for lo, _ in touched(c, i)) == 0
    c["floor"] = floor
    return c


# ------------------------------------------------------------------ c. mixed waves
WAVE_SPECS = [fld("IPv4", "ttl"), fld("UDP", "src"), fld("IPv4", "dst", 1), fld("TCP", "dst"), fld("Ether", "src", 1)]


def waves():
    rng = np.random.default_rng(79)
    deep = lambda: vx(rng, int(rng.integers(0, 3)), int(rng.integers(0, 3)), "TCP", int(rng.integers(0, 9)))  # noqa: E731
    pkts = [deep() if i >= 192 or i == 64 + 17 else udp4(rng, int(rng.integers(0, 4))) for i in range(256)]
    c = make(lay("gaps", pkts, rng), WAVE_SPECS, rng)

    def floor():
        sh = shifts(c)
        deep_at, near = set(), set()
        for i, k, ho in present(c):
            s, e = c["specs"][k][2:]
            if sh[i] + ho + e // 8 >= 80:
                deep_at.add(i)
            if sh[i] + ho + s // 8 + 12 > 80:   # within 12 bytes of the window's end
                near.add(i)
        per = [sum(1 for i in deep_at if i // 64 == w) for w in range(4)]
        assert per == [0, 1, 0, 64] and 64 + 17 in deep_at, per
        assert not any(i // 64 in (0, 2) for i in near)
    c["floor"] = floor
    return c


# ------------------------------------------------------------------ d. chain depth
DEPTH_SPECS = [fld("Vlan", "vid", o) for o in range(6)] + [fld("MPLS", f, o) for o in (0, 3, 4, 7, 8, 15) for f in ("label", "ttl")] + \
              [fld("IPv4", "ttl"), fld("UDP", "src")]


def slots_sought(c):
    """(slot found in, slots of the earlier occurrences) of every present spec."""
    out = []
    for i in range(c["batch"]["n"]):
        rows = chain_rows(c["chain"], i)
        for t, occ, s, e in c["specs"]:
            at = [j for j, (ty, _) in enumerate(rows) if ty == t]
            if occ < len(at):
                out.append((at[occ], at[:occ]))
    return out


def depth():
    rng = np.random.default_rng(80)
    pkts = [udp4(rng, 3, vlans=k) for k in range(7)] + [mpls_pkt(rng, k) for k in range(2, 15)]
    rows = [L4.hdrs_of(p) for p in pkts]
    for _ in range(2):   # a hand-made list of 16 labels over 64 + 20 random bytes
        pkts.append(L4.rnd(rng, 84))
        rows.append([(T("MPLS"), 4 * j) for j in range(16)])
    pkts, rows = pkts * 4, rows * 4   # 88 packets: two waves, every kind at several alignments
    c = make(lay("gaps", pkts, rng), DEPTH_SPECS, rng, chain=FL.chain_from(len(pkts), rows))

    def floor():
        ss = slots_sought(c)
        assert {3, 4, 7, 8, 15} <= {s for s, _ in ss}
        assert any(s >= 4 and before and max(before) <= 3 for s, before in ss)
        assert any(s >= 8 and before and min(before) <= 7 < max(before + [s]) for s, before in ss)
        assert int(c["chain"]["n_hdrs"].max()) == 16
    c["floor"] = floor
    return c


def clamped_chain():
    """n_hdrs of 17 and 255 over 16 real slots (clamped to 16), and n_hdrs 0 over filled slot rows (ignored)."""
    c = dict(depth())
    ch = {k: v.copy() for k, v in c["chain"].items()}
    full = np.flatnonzero(ch["n_hdrs"] == 16)
    assert full.size >= 6
    ch["n_hdrs"][full[0::3]] = 17
    ch["n_hdrs"][full[1::3]] = 255
    some = np.flatnonzero(ch["n_hdrs"] == 4)
    ch["n_hdrs"][some] = 0
    c["chain"] = ch

    def floor():
        assert {0, 17, 255} <= set(ch["n_hdrs"].tolist()) and (ch["hdr_type"][:4, some] != 0).all()
        assert chain_rows(ch, int(full[1])) == chain_rows(depth()["chain"], int(full[1])) and chain_rows(ch, int(some[0])) == []
    c["floor"] = floor
    return c


# ------------------------------------------------------------------ e. spec counts
NSPECS = [1, 2, 3, 4, 5, 31, 32, 33, 64, 65]
_POOL_HDRS = ["IPv4", "UDP", "IPv4", "Ether"]


def spec_pool(k, rng):
    """k specs, header types interleaved (IPv4, UDP, IPv4, Ether, ...): the named fields first, then random ranges
    of at most 64 bits; specs 3|4 and 31|32 name the same bits."""
    named = {h: list(F.FIELDS[T(h)].values()) for h in set(_POOL_HDRS)}
    out = []
    for j in range(k):
        h = _POOL_HDRS[j % 4]
        if named[h] and j < 24:
            s, e = named[h].pop(0)
        else:
            s = int(rng.integers(0, 8 * SIZE[T(h)]))
            e = min(8 * SIZE[T(h)] - 1, s + int(rng.integers(0, 64)))
        out.append((T(h), 0, s, e))
    for j in (3, 31):
        if j + 1 < k:
            out[j + 1] = out[j]
    return out


def counts(layout, k):
    rng = np.random.default_rng(8100 + k)
    pkts = [udp4(rng, 22) if layout == "s64" or i % 5 else arp(rng) for i in range(130)]
    c = make(lay(layout, pkts, rng), spec_pool(k, rng), rng)

    def floor():
        assert len(c["specs"]) == k and len({v.ctypes.data for v in c["values"]}) == k
        for j in (3, 31):
            if j + 1 < k:
                w = min(64, c["specs"][j][3] - c["specs"][j][2] + 1)
                assert c["specs"][j] == c["specs"][j + 1]
                assert ((c["values"][j] ^ c["values"][j + 1]) & np.uint64((1 << w) - 1)).any()
                assert any(kk == j for _, kk, _ in present(c))
        ty = [s[0] for s in c["specs"]]
        assert k < 3 or ty != sorted(ty)     # not grouped by header as given
    c["floor"] = floor
    return c


def alias_outputs(k):
    """Output buffer of each of k specs for the shared-pointer getter: specs 2j and 2j + 1 share one buffer."""
    return [j // 2 for j in range(k)]


# ------------------------------------------------------------------ f. widths and phases
WIDTHS = list(range(1, 10)) + [15, 16, 17, 31, 32, 33] + list(range(57, 65)) + [65, 72, 127, 128]


def width_specs(max_w=128):
    out = []
    for h in ("IPv6", "ARP"):
        bits = 8 * SIZE[T(h)]
        for ph in range(8):
            for w in WIDTHS:
                if w > max_w:
                    continue
                s = ph + 8 * ((3 * ph + w) % 5)
                if s + w > bits:
                    s = ph
                if s + w <= bits:
                    out.append((T(h), 0, s, s + w - 1))
    return out


def widths(ones, max_w=128):
    rng = np.random.default_rng(82)
    pkts, al = [], []
    for a in (0, 1, 7, 15):
        for p in (v6tcp(rng, 5), arp(rng), v6tcp(rng, 0)):
            pkts.append(p)
            al.append(a)
    c = make(lay("gaps", pkts, rng, al), width_specs(max_w), rng, ones=ones)

    def floor():
        def span(s, e):
            s2 = e - 63 if e - s + 1 > 64 else s
            return e // 8 - s2 // 8 + 1
        sp = c["specs"]
        assert sum(1 for _, _, s, e in sp if span(s, e) == 9) >= 20
        ws = {e - s + 1 for _, _, s, e in sp}
        assert (len([w for w in ws if w > 64]) >= 4) if max_w > 64 else (max(ws) == 64)
        assert {(s % 8, e - s + 1) for t, _, s, e in sp if t == T("IPv6")} >= {(ph, w) for ph in range(8) for w in WIDTHS if w <= max_w}
        assert sorted(set(shifts(c))) == [0, 1, 7, 15]
    c["floor"] = floor
    return c


# ------------------------------------------------------------------ g. packed neighbours
PACKED_SPECS = [fld("ARP", "target_proto_addr"), fld("UDP", "checksum"), fld("Ether", "dst"), fld("IPv4", "ttl")]


def neighbours(layout):
    rng = np.random.default_rng(83)
    pkts = [arp(rng) if i % 2 == 0 else udp4(rng) for i in range(200)]
    assert all(len(p) == 42 for p in pkts)
    c = make(lay(layout, pkts, rng), PACKED_SPECS, rng)

    def floor():
        owners = {}
        for i, (o, _) in enumerate(C.extents(c["batch"])):
            for lo, hi in touched(c, i, 0):
                for q in range(o + lo, o + hi + 1):
                    owners.setdefault(q // 16, set()).add(i)
        shared = sum(1 for v in owners.values() if len(v) >= 2)
        assert shared >= 100 if layout == "packed" else shared == 0, shared
    c["floor"] = floor
    return c


# ------------------------------------------------------------------ h. slab end
END_SPECS = [fld("IPv4", "ttl"), fld("IPv4", "dst"), fld("IPv4", "header_checksum"), fld("Ether", "src"), fld("UDP", "dst")]
END_MODS = [0, 1, 4, 9, 15]


def slab_end(layout, mod):
    """The last packet's IPv4 header is the slab's final 20 bytes, slab_len % 16 == mod."""
    rng = np.random.default_rng(8400 + mod)
    pkts = [udp4(rng, int(rng.integers(0, 5))) for _ in range(66)]
    if layout == "gaps":
        pkts.append(eth_ip(rng))
        b = lay("gaps", pkts, rng, [int(rng.integers(0, 16)) for _ in range(66)] + [(mod - 34) % 16])
        ch = None
    else:
        ln = {0: 48, 1: 33, 4: 36, 9: 41, 15: 47}[mod]   # 48 k + ln = mod (mod 16)
        pkts.append(L4.rnd(rng, ln - 20) + eth_ip(rng)[14:])
        b = lay("s48", pkts, rng)
        b["slab"] = b["slab"][:48 * 66 + ln].copy()
        # the hand-made list of the last packet: an IPv4 header where its last 20 bytes are
        rows = [L4.hdrs_of(p) for p in pkts[:-1]] + [([(T("Ether"), 0)] if ln >= 34 else []) + [(T("IPv4"), ln - 20)]]
        ch = FL.chain_from(67, rows)
    c = make(b, END_SPECS, rng, chain=ch)

    def floor():
        o, ln_ = C.extents(b)[-1]
        assert o + ln_ == b["slab"].size and b["slab"].size % 16 == mod
        assert lookup(chain_rows(c["chain"], 66), T("IPv4"), 0) == ln_ - 20
    c["floor"] = floor
    return c


def overrun(layout):
    """The last lens[i] runs 40 bytes past slab_len: the packet is the bytes inside the slab."""
    rng = np.random.default_rng(85)
    pkts = [udp4(rng, int(rng.integers(0, 5))) for _ in range(65)]
    b = lay(layout, pkts, rng)
    b["slab"] = b["slab"][:C.extents(b)[-1][0] + len(pkts[-1])].copy()   # the slab ends with the last packet
    b["lens"] = b["lens"].copy()
    b["lens"][-1] += 40
    c = make(b, END_SPECS, rng)

    def floor():
        o, ln_ = C.extents(b)[-1]
        assert o + int(b["lens"][-1]) == b["slab"].size + 40 and ln_ == len(pkts[-1]) and int(c["chain"]["n_hdrs"][-1]) == 3
    c["floor"] = floor
    return c


# ------------------------------------------------------------------ the Q1 fold inside the refresh
def _nine(total, rng):
    """Nine 16-bit words that sum to `total`."""
    w = [total // 9] * 9
    w[0] += total - sum(w)
    for _ in range(20):
        a, b = (int(x) for x in rng.integers(0, 9, 2))
        if a == b:
            continue
        d = int(rng.integers(0, min(w[a], 0xFFFF - w[b]) + 1))
        w[a], w[b] = w[a] - d, w[b] + d
    assert sum(w) == total and all(0 <= x <= 0xFFFF for x in w)
    return w


Q1_SPECS = [fld("Ether", "src"), fld("IPv4", "dst"), fld("UDP", "checksum")]


def q1_fold(layout):
    """Random headers almost never tell the Q1 fold from RFC 1071 (none of the 14 000 headers that cases a-h
    refresh does), so: IPv4 headers whose nine words sum to 0x1FFFF + 0x10000 j, under the chain of the packet as
    built.  Even packets hold such a header already (the refresh alone meets it); odd ones get it from the `dst`
    setter (the refresh after the setters meets it)."""
    rng = np.random.default_rng(86)
    b = lay(layout, [udp4(rng, 22) for _ in range(130)], rng)
    ch = L4.chain_of(b)
    slab = b["slab"].copy()
    dst = np.zeros(b["n"], np.uint64)
    for i, (o, _) in enumerate(C.extents(b)):
        w = _nine(0x1FFFF + 0x10000 * (i % 7), rng)
        w.insert(5, int(rng.integers(0, 0x10000)))
        hdr = b"".join(x.to_bytes(2, "big") for x in w)
        dst[i] = int.from_bytes(hdr[16:], "big")
        slab[o + 14:o + 34] = np.frombuffer(hdr[:16] + (hdr[16:] if i % 2 == 0 else L4.rnd(rng, 4)), np.uint8)
    b["slab"] = slab
    c = make(b, Q1_SPECS, rng, chain=ch)
    c["values"][1] = dst

    def floor():
        def differ(s):
            hs = [s[o + 14:o + 34].tobytes() for o, _ in C.extents(b)]
            return sum(1 for h in hs if q1(h) != rfc1071(h))
        assert differ(expect_set(c)) == b["n"] and differ(slab) >= b["n"] // 2
    c["floor"] = floor
    return c


# ------------------------------------------------------------------ the table
def _table():
    t = {}
    every = (GET, SET, SET0, SET1, UPD0)
    for layout in LAYOUTS:
        for n in SHAPES:
            t[f"shapes-{layout}-{n}"] = (functools.partial(shapes, layout, n), every)
    for layout in ("gaps", "s128"):
        t[f"sweep-{layout}"] = (functools.partial(sweep, layout), (GET, SET, SET1, UPD1))
    t["sweep-in-window"] = (sweep_in_window, (GET, SET, SET1))
    for layout in ("s64", "s48"):
        t[f"narrow-{layout}"] = (functools.partial(narrow, layout), (GET, SET, SET0))
    t["waves"] = (waves, (GET, SET, SET1))
    t["depth"] = (depth, (GET, SET, SET0))
    t["clamped-chain"] = (clamped_chain, (GET, SET, SET0, UPD0))
    for layout in ("gaps", "s64"):
        for k in NSPECS:
            t[f"counts-{layout}-{k}"] = (functools.partial(counts, layout, k), (GET, SET, SET0))
    t["widths-random"] = (functools.partial(widths, False), (GET, SET))
    t["widths-ones"] = (functools.partial(widths, True), (SET,))
    t["widths64-random"] = (functools.partial(widths, False, 64), (SET,))
    t["widths64-ones"] = (functools.partial(widths, True, 64), (SET,))
    for layout in ("packed", "pcap"):
        t[f"neighbours-{layout}"] = (functools.partial(neighbours, layout), (GET, SET, SET0))
    for layout in ("gaps", "s48"):
        for mod in END_MODS:
            t[f"end-{layout}-{mod}"] = (functools.partial(slab_end, layout, mod), (GET, SET0, UPD0))
        t[f"overrun-{layout}"] = (functools.partial(overrun, layout), (GET, SET0, UPD0))
    for layout in ("gaps", "s64"):
        t[f"q1-{layout}"] = (functools.partial(q1_fold, layout), (SET0, UPD0))
    return t


TABLE = _table()
CALLS = [(name, call) for name, (_, calls) in TABLE.items() for call in calls]


@functools.lru_cache(maxsize=None)
def case(name):
    return TABLE[name][0]()


@functools.lru_cache(maxsize=None)
def expected(name, call):
    return expect_call(case(name), call)


def batch_kw(b):
    return dict(stride=b["stride"], offsets=b["offsets"], lens=b["lens"])


# ------------------------------------------------------------------ i. checksum batch
CSUM_N = [1, 63, 64, 65, 257]
CSUM_STRIDES = [20, 21, 24, 33]


@functools.lru_cache(maxsize=None)
def csum_case(n, stride):
    """(bytes of n headers at `stride`, the expected checksums): a third random, a third all 0xFFFF words but one,
    a third with a nine-word sum of 0x1FFFF + 0x10000 j; bytes 10-11 and the bytes between headers random."""
    rng = np.random.default_rng(8600 + 40 * n + stride)
    buf = bytearray(L4.rnd(rng, n * stride))
    for i in range(n):
        if i % 3 == 0:
            continue
        if i % 3 == 1:
            w = [0xFFFF] * 9
            w[int(rng.integers(0, 9))] = int(rng.integers(0, 0x10000))
        else:
            w = _nine(0x1FFFF + 0x10000 * ((i // 3) % 7), rng)
        w.insert(5, int(rng.integers(0, 0x10000)))
        buf[i * stride:i * stride + 20] = b"".join(x.to_bytes(2, "big") for x in w)
    hs = [bytes(buf[i * stride:i * stride + 20]) for i in range(n)]
    want = np.array([q1(h) for h in hs], np.uint16)
    differ = sum(1 for h in hs if q1(h) != rfc1071(h))
    return np.frombuffer(bytes(buf), np.uint8), want, differ, hs


# ------------------------------------------------------------------ j. broadcast
BCAST = [(1, 16), (15, 16), (16, 16), (17, 32), (60, 64), (64, 64), (42, 80), (154, 1040)]
BCAST_N = [1, 3, 257]
BCAST_BIG = (7, 16, 256 * 64 * 256 + 1000)   # past the grid cap of 256 * 64 blocks of 256 chunks


def bcast_case(length, stride, n):
    src = L4.rnd(np.random.default_rng(8700 + length), length)
    return src, np.frombuffer((src + bytes(stride - length)) * n, np.uint8)
