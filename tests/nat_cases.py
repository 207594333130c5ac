"""The yardstick and the case builders of pkt_nat_* (tests/test_nat_host.py, test_nat_device.py).

The yardstick is a sequential pure-Python model written from the text of include/pktgpu.h: dicts for the sessions, a
walk from the cursor for the allocation, RFC 1624 eq. 3 for the checksums.  It never calls the library.  Checksum
validity is judged by a from-scratch RFC 1071 verifier (ones_sum: "the one's-complement sum over the header, or over
pseudo-header + segment, is 0xFFFF"), never by comparing with the code under test.  The model has no forward table, so
it never says TABLE_FULL: the one test of that status checks invariants (invariants()).

Packets are gen.py's (l4_cases.pkt: Ether / 0-2 Vlan / IPv4 / TCP | UDP | ICMP echo) with addresses, ports and checksums
patched in; an item is (bytes, [(type, offset)]).
"""
import struct

import numpy as np

from pktgpu import schema

import compare_cases as C
import flow_cases as F
import l4_cases as L4
import lpm_cases as X

(OK, SKIPPED, NO_IP, SPAN, IPV6, BAD_HDR, FRAGMENT, NO_L4, NO_SESSION, NOT_OURS, EXHAUSTED, TABLE_FULL) = range(12)
NSTATUS = 12
OUT, IN = 0, 1
NONE = 0xFFFFFFFF
STATIC = 0x80000000
LAST = 0xFF
PROTOS = (6, 17, 1)
T_IPV4, T_IPV6, T_TCP, T_UDP, T_ICMP = (schema.HDR_ID[k] for k in ("IPv4", "IPv6", "TCP", "UDP", "ICMP"))
L4_TYPE = (T_TCP, T_UDP, T_ICMP)
L4_NEED = (20, 8, 8)
CSUM_AT = (16, 6, 2)
NAMES = ("status", "entry", "created")


def ip(a):
    """An address as 4 wire bytes: "a.b.c.d", an int (host order) or bytes."""
    if isinstance(a, str):
        return bytes(int(x) for x in a.split("."))
    if isinstance(a, (int, np.integer)):
        return int(a).to_bytes(4, "big")
    return bytes(a)


# ------------------------------------------------------------------ RFC 1071, from scratch
def ones_sum(data):
    """The 16-bit one's-complement sum of `data` (big-endian words, an odd last byte padded with zero)."""
    if len(data) % 2:
        data = bytes(data) + b"\0"
    s = sum(struct.unpack(f">{len(data) // 2}H", bytes(data)))
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return s


def ip_valid(p, ipo):
    return ones_sum(p[ipo:ipo + 20]) == 0xFFFF


def l4_valid(p, ipo, l4o):
    """True / False, or None for a UDP datagram with no checksum.  The segment runs to the IP total length, which must
    lie inside `p`."""
    proto = p[ipo + 9]
    end = ipo + struct.unpack_from(">H", p, ipo + 2)[0]
    assert end <= len(p), "the verifier needs the whole segment"
    seg = p[l4o:end]
    if proto == 17 and seg[6:8] == b"\0\0":
        return None
    pseudo = b"" if proto == 1 else p[ipo + 12:ipo + 20] + struct.pack(">BBH", 0, proto, len(seg))
    return ones_sum(pseudo + seg) == 0xFFFF


def ip_error(p, ipo):
    """How far the stored IPv4 checksum is from the right one, as a one's-complement difference (0: valid)."""
    return 0xFFFF - ones_sum(p[ipo:ipo + 20])


def l4_error(p, ipo, l4o):
    proto = p[ipo + 9]
    seg = p[l4o:ipo + struct.unpack_from(">H", p, ipo + 2)[0]]
    pseudo = b"" if proto == 1 else p[ipo + 12:ipo + 20] + struct.pack(">BBH", 0, proto, len(seg))
    return 0xFFFF - ones_sum(pseudo + seg)


# ------------------------------------------------------------------ the model
def csum_1624(hc, old, new):
    """RFC 1624 eq. 3 over the words old[k] -> new[k], as include/pktgpu.h spells it out."""
    s = (~hc & 0xFFFF) + sum(~m & 0xFFFF for m in old) + sum(new)
    s = (s & 0xFFFF) + (s >> 16)
    s = (s & 0xFFFF) + (s >> 16)
    return ~s & 0xFFFF


def words(b4):
    return [int.from_bytes(b4[0:2], "big"), int.from_bytes(b4[2:4], "big")]


def classify(p, hdrs, which, d):
    """Steps 2 to 5: (status, p index, ip offset, l4 offset, address bytes, port) of packet bytes `p`."""
    ips = [j for j, (t, _) in enumerate(hdrs) if t in (T_IPV4, T_IPV6)]
    ips = ips[-1:] if which == LAST else ips[which:which + 1]
    if not ips:
        return (NO_IP,)
    j = ips[0]
    t, ipo = hdrs[j]
    if t == T_IPV6:
        return (IPV6,)
    if ipo + 20 > len(p):
        return (SPAN,)
    if p[ipo] != 0x45:
        return (BAD_HDR,)
    if struct.unpack_from(">H", p, ipo + 6)[0] & 0x3FFF:
        return (FRAGMENT,)
    if p[ipo + 9] not in PROTOS:
        return (NO_L4,)
    px = PROTOS.index(p[ipo + 9])
    if j + 1 >= len(hdrs) or hdrs[j + 1][0] != L4_TYPE[px]:
        return (NO_L4,)
    l4o = hdrs[j + 1][1]
    if l4o + L4_NEED[px] > len(p):
        return (SPAN,)
    if px == 2 and p[l4o] not in (8, 0):
        return (NO_L4,)
    at = l4o + (4 if px == 2 else 2 if d else 0)
    a = ipo + (16 if d else 12)
    return OK, px, ipo, l4o, bytes(p[a:a + 4]), struct.unpack_from(">H", p, at)[0]


def rewrite(p, px, ipo, l4o, d, addr, port):
    """[(offset in the packet, new bytes)] of an OK packet whose address and port become `addr`, `port`."""
    a = ipo + (16 if d else 12)
    at = l4o + (4 if px == 2 else 2 if d else 0)
    ck = l4o + CSUM_AT[px]
    oa, op = words(p[a:a + 4]), struct.unpack_from(">H", p, at)[0]
    na = words(addr)
    hc = csum_1624(struct.unpack_from(">H", p, ipo + 10)[0], oa, na)
    lc0 = struct.unpack_from(">H", p, ck)[0]
    if px == 2:
        lc = csum_1624(lc0, [op], [port])
    else:
        lc = csum_1624(lc0, oa + [op], na + [port])
        if px == 1:
            lc = 0 if lc0 == 0 else 0xFFFF if lc == 0 else lc
    return [(a, bytes(addr)), (ipo + 10, struct.pack(">H", hc)), (at, struct.pack(">H", port)), (ck, struct.pack(">H", lc))]


class Model:
    """The sequential model of pkt_nat_*.  static: [(proto, in_addr, in_port, out_addr, out_port)]."""

    def __init__(self, pool, ports=(1024, 65535), static=()):
        self.pool = [ip(a) for a in pool]
        self.lo, self.hi = ports
        self.nports = self.hi - self.lo + 1
        self.E = len(self.pool) * self.nports
        self.static = [(PROTOS.index(_proto(pr)), ip(ia), int(ipt), ip(oa), int(opt)) for pr, ia, ipt, oa, opt in static]
        self.s_in = {(px, ia, ipt): k for k, (px, ia, ipt, oa, opt) in enumerate(self.static)}
        self.s_out = {(px, oa, opt): k for k, (px, ia, ipt, oa, opt) in enumerate(self.static)}
        self.clear()

    def clear(self):
        self.fwd = {}                          # (p, inside addr, inside port) -> e
        self.rev = [dict() for _ in range(3)]  # e -> (inside addr, inside port)
        self.seen = [dict() for _ in range(3)]
        self.cursor = [0, 0, 0]

    def outside(self, e):
        return self.pool[e // self.nports], self.lo + e % self.nports

    def alloc(self, px):
        for s in range(self.E):
            e = (self.cursor[px] + s) % self.E
            if e not in self.rev[px]:
                return e
        return None

    def run(self, b, chain, dir=OUT, now=0, select=None, which_ip=0, write=True):
        n = b["n"]
        ext = C.extents(b)
        slab = b["slab"].copy()
        dirs = [int(dir)] * n if isinstance(dir, (int, np.integer)) else [int(x) for x in dir]
        eff = [2 if (select is not None and not select[i]) or dirs[i] > 1 else dirs[i] for i in range(n)]
        st, ent, made, cls = [SKIPPED] * n, [NONE] * n, [0] * n, [None] * n
        pkts = [b["slab"][o:o + ln].tobytes() for o, ln in ext]
        for i in range(n):
            if eff[i] < 2:
                hd = [(int(chain["hdr_type"][j, i]), int(chain["hdr_off"][j, i]))
                      for j in range(min(int(chain["n_hdrs"][i]), schema.MAX_HDRS))]
                cls[i] = classify(pkts[i], hd, which_ip, eff[i])
                st[i] = cls[i][0]
        none_free = [False] * 3
        for i in range(n):  # the OUT packets in index order
            if eff[i] != OUT or st[i] != OK:
                continue
            _, px, ipo, l4o, addr, port = cls[i]
            key = (px, addr, port)
            if key in self.s_in:
                ent[i] = STATIC | self.s_in[key]
            elif key in self.fwd:
                ent[i] = px * self.E + self.fwd[key]
            else:
                e = None if none_free[px] else self.alloc(px)
                if e is None:
                    none_free[px] = True
                    st[i] = EXHAUSTED
                    continue
                self.fwd[key] = e
                self.rev[px][e] = (addr, port)
                self.seen[px][e] = now
                self.cursor[px] = (e + 1) % self.E
                made[i] = 1
                ent[i] = px * self.E + e
        for i in range(n):  # then the IN packets
            if eff[i] != IN or st[i] != OK:
                continue
            _, px, ipo, l4o, addr, port = cls[i]
            if (px, addr, port) in self.s_out:
                ent[i] = STATIC | self.s_out[(px, addr, port)]
            elif addr in self.pool and self.lo <= port <= self.hi:
                e = self.pool.index(addr) * self.nports + port - self.lo
                if e in self.rev[px]:
                    ent[i] = px * self.E + e
                else:
                    st[i] = NO_SESSION
            else:
                st[i] = NOT_OURS
        hits, nbytes = np.zeros(NSTATUS, np.uint64), np.zeros(NSTATUS, np.uint64)
        for i in range(n):
            hits[st[i]] += 1
            nbytes[st[i]] += ext[i][1]
            if st[i] != OK:
                continue
            _, px, ipo, l4o, addr, port = cls[i]
            to = self.target(ent[i], eff[i])
            if not ent[i] & STATIC:
                e = ent[i] - px * self.E
                self.seen[px][e] = max(self.seen[px][e], now)
            if write:
                for o, data in rewrite(pkts[i], px, ipo, l4o, eff[i], *to):
                    slab[ext[i][0] + o:ext[i][0] + o + len(data)] = np.frombuffer(data, np.uint8)
        return dict(status=np.array(st, np.uint8), entry=np.array(ent, np.uint32), created=np.array(made, np.uint8),
                    hits=hits, bytes=nbytes, slab=slab)

    def target(self, entry, d):
        """The (address, port) an OK packet of direction d is rewritten to."""
        if entry & STATIC:
            px, ia, ipt, oa, opt = self.static[entry & ~STATIC]
            return (ia, ipt) if d else (oa, opt)
        px, e = divmod(entry, self.E)
        return self.rev[px][e] if d else self.outside(e)

    def expire(self, now, idle):
        gone = 0
        for px in range(3):
            for e in sorted(self.rev[px]):
                if idle[px] and self.seen[px][e] + idle[px] <= now:
                    addr, port = self.rev[px].pop(e)
                    del self.seen[px][e]
                    del self.fwd[(px, addr, port)]
                    gone += 1
        return gone

    def count(self):
        return tuple(len(r) for r in self.rev)

    def sessions(self):
        rows = []
        for px in range(3):
            for e in sorted(self.rev[px]):
                rows.append((self.rev[px][e], self.outside(e), PROTOS[px], 0, self.seen[px][e]))
        for px, ia, ipt, oa, opt in self.static:
            rows.append(((ia, ipt), (oa, opt), PROTOS[px], schema.NAT_REC_STATIC, 0))
        rec = np.zeros(len(rows), schema.NAT_RECORD_DTYPE)
        for k, ((ia, ipt), (oa, opt), proto, fl, seen) in enumerate(rows):
            rec["in_addr"][k], rec["out_addr"][k] = np.frombuffer(ia, np.uint8), np.frombuffer(oa, np.uint8)
            rec["in_port"][k], rec["out_port"][k], rec["proto"][k], rec["flags"][k], rec["last_seen"][k] = ipt, opt, proto, fl, seen
        return rec


def _proto(pr):
    return {"tcp": 6, "udp": 17, "icmp": 1}.get(pr, pr)


def check(got, want, label=""):
    for name in NAMES + ("hits", "bytes"):
        if got.get(name) is None:
            continue
        g = np.asarray(got[name])
        assert g.shape == want[name].shape, (label, name, g.shape)
        bad = np.flatnonzero(g != want[name])
        assert bad.size == 0, (label, name, "first bad", bad[:8], g[bad[:8]], want[name][bad[:8]])
    if got.get("slab") is not None:
        bad = np.flatnonzero(np.asarray(got["slab"]) != want["slab"])
        assert bad.size == 0, (label, "slab bytes", bad[:16], np.asarray(got["slab"])[bad[:16]], want["slab"][bad[:16]])


def same_sessions(got, want, label=""):
    assert got.dtype == want.dtype and got.shape == want.shape, (label, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), (label, got[:8], want[:8])


# ------------------------------------------------------------------ packets
_TEMPLATE = {}


def mk(l4, src, sport, dst, dport, vlans=0, payload=b"nat-payload", icmp_type=8, good=True, udp_none=False):
    """(bytes, hdrs) of Ether / vlans x Vlan / IPv4 / l4 with valid checksums (good=False: both off by 5).  For ICMP
    `sport` is the echo identifier (dport is ignored) and the payload follows id and sequence number."""
    key = (l4, vlans, payload)
    if key not in _TEMPLATE:
        p = L4.pkt(l4, vlans=vlans, payload=(b"\0\0\0\7" + payload) if l4 == "ICMP" else payload)
        _TEMPLATE[key] = (bytes(p), F.hdrs_of(p))
    p, hdrs = _TEMPLATE[key]
    q = bytearray(p)
    ipo = 14 + 4 * vlans
    l4o = ipo + 20
    q[ipo + 12:ipo + 16], q[ipo + 16:ipo + 20] = ip(src), ip(dst)
    if l4 == "ICMP":
        q[l4o] = icmp_type
        q[l4o + 4:l4o + 6] = struct.pack(">H", sport)
    else:
        q[l4o:l4o + 4] = struct.pack(">HH", sport, dport)
    return finalize(bytes(q), ipo, l4o, good, udp_none), hdrs


def finalize(p, ipo, l4o, good=True, udp_none=False):
    """`p` with its IPv4 and L4 checksums made valid by ones_sum (UDP: 0 -> 0xFFFF; udp_none: left 0)."""
    q = bytearray(p)
    proto = q[ipo + 9]
    ck = l4o + CSUM_AT[PROTOS.index(proto)]
    q[ipo + 10:ipo + 12] = b"\0\0"
    q[ipo + 10:ipo + 12] = struct.pack(">H", 0xFFFF - ones_sum(q[ipo:ipo + 20]))
    q[ck:ck + 2] = b"\0\0"
    if not (proto == 17 and udp_none):
        seg = q[l4o:ipo + struct.unpack_from(">H", q, ipo + 2)[0]]
        pseudo = b"" if proto == 1 else bytes(q[ipo + 12:ipo + 20]) + struct.pack(">BBH", 0, proto, len(seg))
        c = 0xFFFF - ones_sum(pseudo + bytes(seg))
        q[ck:ck + 2] = struct.pack(">H", 0xFFFF if proto == 17 and c == 0 else c)
    if not good:
        q[ipo + 11] = (q[ipo + 11] + 5) & 0xFF
        q[ck + 1] = (q[ck + 1] + 5) & 0xFF
    return bytes(q)


def offsets(item, k=0):
    """(ip offset, l4 offset) of the item's k-th IPv4 header and the entry behind it."""
    hdrs = item[1]
    j = [x for x, (t, _) in enumerate(hdrs) if t == T_IPV4][k]
    return hdrs[j][1], hdrs[j + 1][1]


def reply(item, k=0):
    """The mirrored reply to a packet: addresses and ports swapped (ICMP: type 0, the same identifier), valid checksums."""
    p, hdrs = item
    ipo, l4o = offsets(item, k)
    q = bytearray(p)
    q[ipo + 12:ipo + 16], q[ipo + 16:ipo + 20] = p[ipo + 16:ipo + 20], p[ipo + 12:ipo + 16]
    if p[ipo + 9] == 1:
        q[l4o] = 0
    else:
        q[l4o:l4o + 2], q[l4o + 2:l4o + 4] = p[l4o + 2:l4o + 4], p[l4o:l4o + 2]
    return finalize(bytes(q), ipo, l4o), hdrs


def dport_landing_on_zero(l4, out_addr, out_port):
    """The destination port with which the translated packet's checksum computes to 0: found from the sum of the
    translated packet with port 0 and no checksum."""
    p, h = mk(l4, out_addr, out_port, REMOTE, 0)
    ipo, l4o = offsets((p, h))
    q = bytearray(p)
    ck = l4o + (16 if l4 == "TCP" else 6)
    q[ck:ck + 2] = b"\0\0"
    seg = bytes(q[l4o:])
    s = ones_sum(bytes(q[ipo + 12:ipo + 20]) + struct.pack(">BBH", 0, q[ipo + 9], len(seg)) + seg)
    d = 0xFFFF - s
    assert 0 < d < 0xFFFF
    return d


def cut(item, n):
    return item[0][:n], item[1]


def vxlan():
    """Ether / IPv4 / UDP / Vxlan / Ether / IPv4 / TCP, every checksum valid."""
    p, hdrs = X.template("vxlan")
    item = (p, hdrs)
    ipo1, l4o1 = offsets(item, 1)
    p = finalize(p, ipo1, l4o1)       # the inner segment first: the outer UDP checksum covers it
    ipo0, l4o0 = offsets(item, 0)
    return finalize(p, ipo0, l4o0), hdrs


def layout(items, kind="indexed", seed=3, stride=None):
    """(batch, chain): "indexed": back to back, packet i at alignment i % 16, the last one ending at the slab's last
    byte; "stride": fixed-stride slots with lens."""
    n = len(items)
    chain = F.chain_from(n, [h for _, h in items])
    if kind == "indexed":
        return C.indexed([p for p, _ in items], np.random.default_rng(seed), align=[i % 16 for i in range(n)]), chain
    stride = stride or (max(len(p) for p, _ in items) + 15) // 16 * 16
    slab = np.random.default_rng(seed).integers(0, 256, n * stride, dtype=np.uint8)
    for i, (p, _) in enumerate(items):
        slab[i * stride:i * stride + len(p)] = np.frombuffer(p, np.uint8)
    return C.batch(slab, lens=[len(p) for p, _ in items], stride=stride, n=n), chain


def packet_after(b, slab, i):
    o, ln = C.extents(b)[i]
    return bytes(slab[o:o + ln])


# ------------------------------------------------------------------ shared cases
INSIDE = 0x0A000000   # 10.0.0.0/8: the inside hosts
REMOTE = "198.51.100.7"
POOL1 = ["192.0.2.1"]
STATICS = [("tcp", "10.9.9.9", 8080, "192.0.2.200", 80), ("udp", "10.9.9.9", 5353, "192.0.2.1", 53),
           ("icmp", "10.9.9.8", 77, "192.0.2.201", 77)]


def flow_item(k, l4=None, vlans=0, payload=b"nat-payload"):
    """The k-th inside flow's OUT packet: its protocol cycles TCP, UDP, ICMP unless given."""
    l4 = l4 or ("TCP", "UDP", "ICMP")[k % 3]
    return mk(l4, INSIDE + 1 + k // 7, 2000 + k, REMOTE, 443, vlans=vlans, payload=payload)


def statuses_items():
    """One packet per status the model can give, with its direction: [(item, dir, select)] in status order."""
    good = mk("TCP", "10.0.0.1", 1111, REMOTE, 80)
    arp = X.template("arp")
    v6 = (L4.pkt("UDP", v6=True, payload=b"six"), None)
    v6 = (v6[0], F.hdrs_of(v6[0]))
    ipo, l4o = offsets(good)
    bad_hdr = bytearray(good[0])
    bad_hdr[ipo] = 0x46
    frag = bytearray(good[0])
    frag[ipo + 6:ipo + 8] = struct.pack(">H", 0x2000)
    gre = bytearray(good[0])
    gre[ipo + 9] = 47
    return [(good, OUT, 1), (good, OUT, 0), (arp, OUT, 1), (cut(good, ipo + 19), OUT, 1), (v6, OUT, 1),
            ((bytes(bad_hdr), good[1]), OUT, 1), ((bytes(frag), good[1]), OUT, 1), ((bytes(gre), good[1]), OUT, 1),
            (mk("TCP", REMOTE, 80, "192.0.2.1", 40500), IN, 1), (mk("TCP", REMOTE, 80, "192.0.2.77", 40500), IN, 1)]


def invariants(got, b, chain, model_args, dirs, label=""):
    """What holds of a call whatever the forward table lost: the OK packets' entries form a bijection inside the pool,
    every packet of a key shares its verdict, and each OK packet's bytes are the model's rewrite for its entry."""
    pool, ports, static = model_args
    m = Model(pool, ports, static)
    ext = C.extents(b)
    by_key, by_ent = {}, {}
    for i in range(b["n"]):
        o, ln = ext[i]
        p = b["slab"][o:o + ln].tobytes()
        hd = [(int(chain["hdr_type"][j, i]), int(chain["hdr_off"][j, i])) for j in range(int(chain["n_hdrs"][i]))]
        c = classify(p, hd, 0, dirs[i])
        st, ent = int(got["status"][i]), int(got["entry"][i])
        if c[0] != OK:
            assert st == c[0], (label, i, st, c[0])
            continue
        _, px, ipo, l4o, addr, port = c
        assert dirs[i] == OUT
        assert st in (OK, TABLE_FULL, EXHAUSTED), (label, i, st)
        assert by_key.setdefault((px, addr, port), (st, ent)) == (st, ent), (label, i, "a key's packets disagree")
        want = bytearray(p)
        if st == OK:
            assert px * m.E <= ent < (px + 1) * m.E, (label, i, ent)
            assert by_ent.setdefault(ent, (px, addr, port)) == (px, addr, port), (label, i, "an entry has two keys")
            for at, data in rewrite(p, px, ipo, l4o, OUT, *m.outside(ent - px * m.E)):
                want[at:at + len(data)] = data
        else:
            assert ent == NONE
        assert bytes(got["slab"][o:o + ln]) == bytes(want), (label, i, "bytes")
    return by_key, by_ent
