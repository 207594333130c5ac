"""The yardstick and the case builders of pkt_tunnel_* (tests/test_tunnel_host.py, test_tunnel_device.py).

The yardstick is an independent pure-Python model written from the rules of include/pktgpu.h (RFC 7348, RFC 2784 / 2890,
RFC 2003 / 2473 layouts) with plain struct and numpy: it never calls the library, its checksum is the plain RFC 1071 loop
and its table lookup is a dict.  Given a batch, chain columns, the table and the per-packet inputs it returns the expected
status / out_index / tunnel_out / counters, the output packets byte for byte and their chain rows.

A case is a list of items (packet bytes, [(type, offset)]); frag_cases.layout() puts them into an indexed or a
fixed-stride batch.
"""
import socket
import struct

import numpy as np

from pktgpu import gen, schema

import compare_cases as C
import frag_cases as G
import icmp_cases as I
import l4_cases as L4

# encap / decap statuses, written out again
(E_OK, E_SKIPPED, E_NO_TUNNEL, E_NO_IP, E_SPAN, E_BAD_L2, E_BAD_HDR, E_TRUNC, E_TOO_BIG, E_DEPTH) = range(10)
(D_OK, D_SKIPPED, D_NO_IP, D_SPAN, D_BAD_HDR, D_FRAGMENT, D_NOT_TUNNEL, D_BAD_GRE, D_NO_MATCH, D_TRUNC, D_NO_INNER) = range(11)
NST = {"encap": 10, "decap": 11}
NONE = 0xFFFFFFFF
LAST = 0xFF
NO_WRITE = 1
VXLAN, GRE, IPIP = 0, 1, 2
F_KEY, F_DF, F_INHERIT, F_CSUM, F_ANY = 1, 2, 4, 8, 16
HID = schema.HDR_ID
T_ETHER, T_VLAN, T_IPV4, T_IPV6, T_UDP, T_VXLAN, T_GRE, T_GRE_KEY, T_MPLS = (
    HID[k] for k in ("Ether", "Vlan", "IPv4", "IPv6", "UDP", "Vxlan", "GRE", "GREKey", "MPLS"))
T_GRE_CK, T_GRE_SEQ = HID["GREChksumOffset"], HID["GRESequenceNum"]
MAXH = schema.MAX_HDRS
r16 = G.r16
layout = G.layout
cached = G.cached
check = I.check  # the output-contract comparison (layout rule, zero fill, rows, empty tail) is the same
pkt = I.pkt
udp = I.udp


def be16(p, at):
    return p[at] << 8 | p[at + 1]


def csum(b):
    """RFC 1071: the folded one's-complement sum of the big-endian 16-bit words of b (an odd byte padded)."""
    b = bytes(b) + (b"\0" if len(b) & 1 else b"")
    s = sum(struct.unpack(">%dH" % (len(b) // 2), b))
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return s


def addr(a):
    if isinstance(a, str):
        a = socket.inet_pton(socket.AF_INET6 if ":" in a else socket.AF_INET, a)
    return bytes(a)


def entry(kind, src, dst, ttl=0, tos=0, id=0, sport=(49152, 65535), eth_dst=bytes(6), eth_src=bytes(6), flags=0, ipver=None):
    """An entry as the model reads it."""
    src, dst = addr(src), addr(dst)
    return dict(kind=kind, ipver=ipver or (4 if len(src) == 4 else 6), src=src, dst=dst, ttl=ttl, tos=tos, id=id,
                sport=tuple(sport), eth_dst=bytes(eth_dst), eth_src=bytes(eth_src), flags=flags)


def records(entries):
    """The entries as pkt_tunnel_entry_t records."""
    out = np.zeros(len(entries), schema.TUNNEL_ENTRY_DTYPE)
    for r, e in zip(out, entries):
        r["kind"], r["ipver"], r["ttl"], r["tos"], r["flags"], r["id"] = e["kind"], e["ipver"], e["ttl"], e["tos"], e["flags"], e["id"]
        r["sport_lo"], r["sport_hi"] = e["sport"]
        r["src"][:len(e["src"])] = np.frombuffer(e["src"], np.uint8)
        r["dst"][:len(e["dst"])] = np.frombuffer(e["dst"], np.uint8)
        r["eth_dst"][:] = np.frombuffer(e["eth_dst"], np.uint8)
        r["eth_src"][:] = np.frombuffer(e["eth_src"], np.uint8)
    return out


# ------------------------------------------------------------------ the yardstick: encap
def outer_ip(E, proto, plen, tos, ident):
    ttl = E["ttl"] or 64
    if E["ipver"] == 4:
        h = bytearray(struct.pack(">BBHHHBBH4s4s", 0x45, tos, 20 + plen, ident & 0xFFFF, 0x4000 if E["flags"] & F_DF else 0,
                                  ttl, proto, 0, E["src"][:4], E["dst"][:4]))
        h[10:12] = struct.pack(">H", ~csum(h) & 0xFFFF)
        return bytes(h)
    return struct.pack(">IHBB", 6 << 28 | tos << 20, plen, proto, ttl) + E["src"] + E["dst"]


def ip_tos(p, at, v4):
    return p[at + 1] if v4 else (p[at] & 0xF) << 4 | p[at + 1] >> 4


def pick_ip(hdrs, which):
    ips = [j for j, (t, _) in enumerate(hdrs) if t in (T_IPV4, T_IPV6)]
    ips = ips[-1:] if which == LAST else ips[which:which + 1]
    return ips[0] if ips else None


def encap_one(p, hdrs, t, entries, ent, which, selected, ident, q):
    """(status, output bytes, rows) of packet bytes `p` with the chain `hdrs` (already cut to 16 entries) into entry t."""
    if not selected:
        return E_SKIPPED, None, None
    if t >= len(entries):
        return E_NO_TUNNEL, None, None
    E = entries[t]
    o4 = E["ipver"] == 4
    H = 20 if o4 else 40
    tos = E["tos"]
    if E["kind"] == VXLAN:
        if E["flags"] & F_INHERIT:
            first = [(ty, o) for ty, o in hdrs if ty in (T_IPV4, T_IPV6)][:1]
            if first and first[0][1] + 2 <= len(p):
                tos = ip_tos(p, first[0][1], first[0][0] == T_IPV4)
        if (36 if o4 else 16) + len(p) > 65535:
            return E_TOO_BIG, None, None
        if len(hdrs) + 4 > MAXH:
            return E_DEPTH, None, None
        lo, hi = E["sport"]
        ul = 16 + len(p)
        u = bytearray(struct.pack(">HHHH", lo + ent % (hi - lo + 1), 4789, ul, 0))
        vx = struct.pack(">II", 0x08000000, E["id"] << 8)
        if E["flags"] & F_CSUM:
            pseudo = E["src"][:4] + E["dst"][:4] + struct.pack(">BBH", 0, 17, ul) if o4 else \
                E["src"] + E["dst"] + struct.pack(">IHBB", ul, 0, 0, 17)
            u[6:8] = struct.pack(">H", (~csum(pseudo + bytes(u) + vx + p) & 0xFFFF) or 0xFFFF)
        out = E["eth_dst"] + E["eth_src"] + (b"\x08\x00" if o4 else b"\x86\xdd") + outer_ip(E, 17, ul, tos, ident + q) + \
            bytes(u) + vx + p
        rows = [(T_ETHER, 0), (T_IPV4 if o4 else T_IPV6, 14), (T_UDP, 14 + H), (T_VXLAN, 22 + H)] + \
            [(ty, (o + 30 + H) & 0xFFFF) for ty, o in hdrs]
        return E_OK, out, rows
    e = pick_ip(hdrs, which)
    if e is None:
        return E_NO_IP, None, None
    ty, ip = hdrs[e]
    v4 = ty == T_IPV4
    if ip + (20 if v4 else 40) > len(p):
        return E_SPAN, None, None
    prev = hdrs[e - 1][0] if e else None
    if e and prev not in (T_ETHER, T_VLAN, T_MPLS):
        return E_BAD_L2, None, None
    patch = e and prev in (T_ETHER, T_VLAN)
    if patch and ip < 2:
        return E_SPAN, None, None
    if v4:
        L = be16(p, ip + 2)
        if p[ip] != 0x45 or L < 20:
            return E_BAD_HDR, None, None
    else:
        L = 40 + be16(p, ip + 4)
        if p[ip] >> 4 != 6:
            return E_BAD_HDR, None, None
    if ip + L > len(p):
        return E_TRUNC, None, None
    key = E["kind"] == GRE and E["flags"] & F_KEY
    g = b""
    if E["kind"] == GRE:
        g = struct.pack(">HH", 0x2000 if key else 0, 0x0800 if v4 else 0x86DD) + (struct.pack(">I", E["id"]) if key else b"")
    if (20 if o4 else 0) + len(g) + L > 65535:
        return E_TOO_BIG, None, None
    add = [(T_IPV4 if o4 else T_IPV6, ip)] + ([(T_GRE, ip + H)] if E["kind"] == GRE else []) + ([(T_GRE_KEY, ip + H + 4)] if key else [])
    if len(hdrs) + len(add) > MAXH:
        return E_DEPTH, None, None
    if E["flags"] & F_INHERIT:
        tos = ip_tos(p, ip, v4)
    l2 = bytearray(p[:ip])
    if patch:
        l2[ip - 2:ip] = b"\x08\x00" if o4 else b"\x86\xdd"
    proto = 47 if E["kind"] == GRE else 4 if v4 else 41
    out = bytes(l2) + outer_ip(E, proto, len(g) + L, tos, ident + q) + g + p[ip:ip + L]
    rows = hdrs[:e] + add + [(ty2, (o + H + len(g)) & 0xFFFF) for ty2, o in hdrs[e:]]
    return E_OK, out, rows


# ------------------------------------------------------------------ the yardstick: decap
def lookup_table(entries):
    """The decap lookup as a dict: (kind, ipver, key present, local, remote or None, id) -> entry index."""
    tab = {}
    for k, E in enumerate(entries):
        n = 4 if E["ipver"] == 4 else 16
        key = E["kind"] == GRE and bool(E["flags"] & F_KEY)
        ident = E["id"] if E["kind"] == VXLAN or key else 0
        tab[(E["kind"], E["ipver"], key, E["src"][:n], None if E["flags"] & F_ANY else E["dst"][:n], ident)] = k
    return tab


def decap_one(p, hdrs, tab, which, selected):
    """(status, tunnel_out, output bytes, rows)."""
    if not selected:
        return D_SKIPPED, NONE, None, None
    e = pick_ip(hdrs, which)
    if e is None:
        return D_NO_IP, NONE, None, None
    ty, ip = hdrs[e]
    v4 = ty == T_IPV4
    H = 20 if v4 else 40
    if ip + H > len(p):
        return D_SPAN, NONE, None, None
    A = ip + H
    if (p[ip] != 0x45) if v4 else (p[ip] >> 4 != 6):
        return D_BAD_HDR, NONE, None, None
    if v4 and be16(p, ip + 6) & 0x3FFF:
        return D_FRAGMENT, NONE, None, None
    nxt = hdrs[e + 1:e + 4] + [(0, 0)] * 3
    if nxt[0] == (T_UDP, A) and nxt[1] == (T_VXLAN, A + 8):
        kind, T = VXLAN, 16
    elif nxt[0] == (T_GRE, A):
        kind, T = GRE, 4
    elif nxt[0][0] in (T_IPV4, T_IPV6) and nxt[0][1] == A:
        kind, T = IPIP, 0
    else:
        return D_NOT_TUNNEL, NONE, None, None
    if A + T > len(p):
        return D_SPAN, NONE, None, None
    Lo = be16(p, ip + 2) if v4 else 40 + be16(p, ip + 4)
    ident, key, in6 = 0, False, nxt[0][0] == T_IPV6
    if kind == VXLAN:
        if be16(p, A + 4) != (Lo - H) & 0xFFFFFFFF:
            return D_BAD_HDR, NONE, None, None
        ident = int.from_bytes(p[A + 12:A + 15], "big")
    elif kind == GRE:
        proto = be16(p, A + 2)
        if p[A] & 0xD0 or p[A + 1] & 7 or proto not in (0x0800, 0x86DD) or \
                any(t in (T_GRE_CK, T_GRE_SEQ) for t, _ in nxt[1:3]):
            return D_BAD_GRE, NONE, None, None
        in6 = proto == 0x86DD
        if p[A] & 0x20:
            T = 8
            if A + T > len(p):
                return D_SPAN, NONE, None, None
            key, ident = True, int.from_bytes(p[A + 4:A + 8], "big")
    src, dst = (p[ip + 12:ip + 16], p[ip + 16:ip + 20]) if v4 else (p[ip + 8:ip + 24], p[ip + 24:ip + 40])
    base = (kind, 4 if v4 else 6, key, bytes(dst))
    t = tab.get(base + (bytes(src), ident), tab.get(base + (None, ident)))
    if t is None:
        return D_NO_MATCH, NONE, None, None
    if ip + Lo > len(p):
        return D_TRUNC, t, None, None
    inner = max(0, Lo - H - T)
    rows_out = {VXLAN: 3, GRE: 3 if key else 2, IPIP: 1}[kind]
    if kind == VXLAN:
        if e + rows_out >= len(hdrs) or inner < 14:
            return D_NO_INNER, t, None, None
        return D_OK, t, p[A + 16:ip + Lo], [(ty2, (o - A - 16) & 0xFFFF) for ty2, o in hdrs[e + 3:]]
    if inner < (40 if in6 else 20):
        return D_NO_INNER, t, None, None
    l2 = bytearray(p[:ip])
    if e and hdrs[e - 1][0] in (T_ETHER, T_VLAN) and ip >= 2:
        l2[ip - 2:ip] = b"\x86\xdd" if in6 else b"\x08\x00"
    return D_OK, t, bytes(l2) + p[A + T:ip + Lo], hdrs[:e] + [(ty2, (o - H - T) & 0xFFFF) for ty2, o in hdrs[e + rows_out:]]


def expect(op, b, chain, entries, tunnel=0, entropy=None, ident=0, select=None, which=0):
    """The model's whole result for batch `b`: status / out_index / (tunnel_out) / hits, n_out, bytes_out, and per output:
    pkts (bytes), src_index, rows ([(type, offset)])."""
    n = b["n"]
    out = dict(status=np.zeros(n, np.uint8), out_index=np.full(n, NONE, np.uint32), hits=np.zeros(NST[op], np.uint64),
               pkts=[], src_index=[], rows=[])
    if op == "decap":
        out["tunnel_out"] = np.full(n, NONE, np.uint32)
        tab = lookup_table(entries)
    for i, (off, ln) in enumerate(C.extents(b)):
        p = b["slab"][off:off + ln].tobytes()
        nh = min(int(chain["n_hdrs"][i]), MAXH)
        hdrs = [(int(chain["hdr_type"][j, i]), int(chain["hdr_off"][j, i])) for j in range(nh)]
        sel = select is None or select[i] != 0
        q = len(out["pkts"])
        if op == "encap":
            t = int(tunnel) if np.isscalar(tunnel) else int(tunnel[i])
            st, o, rows = encap_one(p, hdrs, t, entries, 0 if entropy is None else int(entropy[i]), which, sel, ident, q)
        else:
            st, out["tunnel_out"][i], o, rows = decap_one(p, hdrs, tab, which, sel)
        out["status"][i] = st
        out["hits"][st] += 1
        if st == 0:
            out["out_index"][i] = q
            out["pkts"].append(bytes(o))
            out["src_index"].append(i)
            out["rows"].append(rows)
    out["n_out"] = len(out["pkts"])
    out["bytes_out"] = sum(r16(len(q)) for q in out["pkts"])
    return out


def check_all(got, want, cap, label=""):
    check(got, want, cap, label)
    if "tunnel_out" in want and got.get("tunnel_out") is not None:
        assert np.array_equal(got["tunnel_out"], want["tunnel_out"]), (label, "tunnel_out")


# ------------------------------------------------------------------ the table and the packets of the mix
M1, M2 = bytes([0, 1, 2, 3, 4, 5]), bytes([0, 6, 7, 8, 9, 10])
LOC4, REM4, REM4B = "192.0.2.1", "198.51.100.2", "198.51.100.77"
LOC6, REM6 = "2001:db8::1", "2001:db8::2"


def mirror(e):
    """The entry as the other end holds it."""
    return dict(e, src=e["dst"], dst=e["src"])


def table():
    """3 kinds x 2 outer versions and the flag variants (0..13), the same tunnels as their other ends hold them
    (14..27: what decap matches the packets of 0..13 by), and 28, whose packets reach LOC4 from REM4 with VNI 99:
    entries 12 / 13 share their local address and VNI, the exact remote REM4B and the ANY_REMOTE key."""
    base = _base()
    return base + [mirror(e) for e in base] + [entry(VXLAN, REM4, LOC4, id=99, sport=(4000, 4000))]


def _base():
    return [
        entry(VXLAN, LOC4, REM4, id=2000, sport=(9090, 9090), eth_dst=M1, eth_src=M2),                    # 0
        entry(VXLAN, LOC6, REM6, id=0xABCDEF, tos=0x1C, eth_dst=M2, eth_src=M1, flags=F_CSUM),            # 1
        entry(GRE, LOC4, REM4, ttl=33, flags=F_DF),                                                        # 2
        entry(GRE, LOC6, REM6, id=0xDEADBEEF, flags=F_KEY | F_INHERIT),                                    # 3
        entry(IPIP, LOC4, REM4, tos=0x08),                                                                 # 4
        entry(IPIP, LOC6, REM6, ttl=255, flags=F_INHERIT),                                                 # 5
        entry(VXLAN, LOC4, REM4, id=7, sport=(0, 65535), flags=F_CSUM | F_INHERIT | F_DF),                 # 6
        entry(GRE, LOC4, REM4, id=5, flags=F_KEY),                                                         # 7
        entry(GRE, LOC4, REM4B, id=6, flags=F_KEY | F_ANY),                                         # 8
        entry(VXLAN, LOC6, REM6, id=1, sport=(1024, 1027)),                                                # 9
        entry(IPIP, LOC4, REM4B, flags=F_DF),                                                              # 10
        entry(GRE, LOC6, REM6),                                                                            # 11
        entry(VXLAN, LOC4, REM4B, id=99, sport=(5000, 5999)),                                              # 12: exact remote
        entry(VXLAN, LOC4, "203.0.113.9", id=99, flags=F_ANY | F_CSUM),                                    # 13: any remote
    ]


def ref22():
    """The 22 reference packets with the chains of the Python parser model."""
    return [(bytes(p.to_vec()), L4.hdrs_of(bytes(p.to_vec()))) for p in gen.reference_22_packets()]


def mpls(payload, v6=False):
    """Ether / one MPLS label / IP / UDP, with the chain a label-aware parse gives."""
    ip, _ = pkt(payload, v6=v6)
    p = ip[:12] + b"\x88\x47" + struct.pack(">I", 77 << 12 | 1 << 8 | 64) + ip[14:]
    return p, [(T_ETHER, 0), (T_MPLS, 14), (T_IPV6 if v6 else T_IPV4, 18), (T_UDP, 58 if v6 else 38)]


def raw_ip(payload, v6=False):
    """The IP packet alone, the chain starting at the IP entry (a raw-IP batch)."""
    p, hdrs = pkt(payload, v6=v6)
    return p[14:], [(t, o - 14) for t, o in hdrs[1:]]


def deep(k):
    """Ether / (k - 3) VLAN tags / IPv4 / UDP: k rows in all."""
    return pkt(udp(40, k), vlans=k - 3)


def forged():
    """Chain columns that are no parse: offsets past the packet, an Ether entry 'before' an IP entry at offset 0."""
    p, hdrs = pkt(udp(64, 3))
    return [(p, [(T_ETHER, 0), (T_IPV4, 60000), (T_UDP, 65535)]),
            (p, [(T_ETHER, 0), (T_IPV4, len(p) - 5)]),
            (p[14:], [(T_ETHER, 0), (T_IPV4, 0), (T_UDP, 20)]),
            (p, [(T_IPV4, 14), (T_UDP, 65000), (T_VXLAN, 3)]),
            (p, [(T_ETHER, 0), (T_IPV4, 14), (T_GRE, 34), (T_IPV4, 65530)])]


def encap_mix(n, seed=9):
    """n packets and their per-packet tunnel and entropy, deciding every status of encap: the 22 reference packets, 0..2
    VLAN tags, MPLS, raw IP, IPv4 and IPv6 inners, bad headers, lying lengths, rows at 16 and 17, forged chains
    -> (items, tunnel uint32 [n], entropy uint32 [n], select)."""
    rng = np.random.default_rng(seed)
    ntab = len(table())
    items = ref22() + forged()
    while len(items) < n:
        i = len(items)
        k = i % 23
        v6 = bool(rng.integers(0, 2))
        vl = int(rng.integers(0, 3))
        pay = udp(int(rng.integers(8, 300)), seed=i)
        it = pkt(pay, v6=v6, vlans=vl, pad=int(rng.integers(0, 5)) if k == 20 else 0)
        if k == 1:
            it = mpls(pay, v6)
        elif k == 2:
            it = raw_ip(pay, v6)
        elif k == 3:
            it = pkt(pay, v6=v6, vlans=vl, b0=0x50 if v6 else 0x46)                       # BAD_HDR for GRE / IPIP
        elif k == 4:
            it = pkt(pay, v6=v6, vlans=vl, trunc=3)                                       # TRUNC
        elif k == 5:
            it = (bytes(rng.integers(0, 256, 64, dtype=np.uint8)), [(T_ETHER, 0)])        # NO_IP
        elif k == 6:
            p, h = pkt(pay, v6=v6)
            it = (p, [(T_ETHER, 0), (T_UDP, 6), h[1]])                                    # BAD_L2: a UDP row before the IP row
        elif k == 7:
            it = deep(12 + i % 5)                                                         # 12..16 rows: DEPTH by the kind
        elif k == 8:
            it = pkt(pay, vlans=vl, L=10)                                                 # BAD_HDR: IPv4 length below 20
        items.append(it)
    items = items[:n]
    tunnel = rng.integers(0, ntab, n).astype(np.uint32)
    tunnel[np.arange(n) % 29 == 11] = ntab + 5                                            # NO_TUNNEL
    tunnel[np.arange(n) % 31 == 12] = 0xFFFFFFFF
    entropy = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    select = (np.arange(n) % 17 != 5).astype(np.uint8)
    return items, tunnel, entropy, select


def big(inner_len, v6=False):
    """Ether / IP / payload with the IP packet `inner_len` bytes long."""
    H = 40 if v6 else 20
    return pkt(G.pattern(inner_len - H, inner_len), v6=v6, proto=253)


def tunnelled(items, tunnel, entropy=None, ident=0, which=0):
    """The model's encap outputs as items (bytes, rows): the sources of the decap cases."""
    ents = table()
    out = []
    for i, (p, hdrs) in enumerate(items):
        t = int(tunnel) if np.isscalar(tunnel) else int(tunnel[i])
        st, o, rows = encap_one(p, hdrs[:MAXH], t, ents, 0 if entropy is None else int(entropy[i]), which, True, ident, len(out))
        if st == E_OK:
            out.append((bytes(o), rows))
    return out


def edit(item, at, val, rows=None):
    p, h = item
    q = bytearray(p)
    q[at:at + len(val)] = val
    return bytes(q), (h if rows is None else rows)


def decap_mix(n, seed=13):
    """n packets deciding every status of decap: tunnelled packets of every entry, plain packets, fragments, bad GRE
    headers, unknown tunnels, lying lengths, empty inners, forged chains -> (items, select)."""
    rng = np.random.default_rng(seed)
    ents = table()
    src, tun, _, _ = encap_mix(3 * n, seed + 1)
    good = tunnelled(src, tun % len(ents), np.arange(3 * n))
    v4x = [it for it in good if it[1][1] == (T_IPV4, 14) and it[1][2][0] == T_UDP]       # VXLAN over IPv4
    g4 = [it for it in good if it[1][-1][0] and (T_GRE, 34) in it[1] and it[1][1] == (T_IPV4, 14)]
    assert len(v4x) > 8 and len(g4) > 8
    # NO_INNER: VXLAN around 10 bytes that no row follows, and around 12 bytes under an Ether row
    items = forged() + ref22() + tunnelled([(bytes(10), []), (bytes(range(12)), [(T_ETHER, 0)])], 0)
    while len(items) < n:
        i = len(items)
        it = good[(7 * i) % len(good)]
        k = i % 19
        if k == 1:
            it = edit(v4x[i % len(v4x)], 14 + 6, b"\x20\x00")                             # FRAGMENT (MF)
        elif k == 2:
            it = edit(v4x[i % len(v4x)], 14 + 6, b"\x00\x10")                             # FRAGMENT (offset)
        elif k == 3:
            it = edit(g4[i % len(g4)], 34, b"\x80")                                       # BAD_GRE: checksum bit
        elif k == 4:
            it = edit(g4[i % len(g4)], 35, b"\x01")                                       # BAD_GRE: version
        elif k == 5:
            it = edit(g4[i % len(g4)], 36, b"\x65\x58")                                   # BAD_GRE: protocol
        elif k == 6:
            it = edit(v4x[i % len(v4x)], 14 + 16, bytes([10, 9, 8, 7]))                   # NO_MATCH: not our address
        elif k == 7:
            it = edit(v4x[i % len(v4x)], 34 + 4, b"\x00\x11")                             # BAD_HDR: the UDP length
        elif k == 8:
            p, h = v4x[i % len(v4x)]
            it = (p[:len(p) - 7], h)                                                      # TRUNC
        elif k == 9:
            p, h = v4x[i % len(v4x)]
            it = (p[:50], h[:4])                                                          # SPAN / NO_INNER by what is left
        elif k == 10:
            it = edit(v4x[i % len(v4x)], 14, b"\x46")                                     # BAD_HDR: options
        elif k == 11:
            it = pkt(udp(50, i), v6=bool(i & 1), vlans=i % 3)                             # NOT_TUNNEL
        elif k == 12:
            it = (bytes(rng.integers(0, 256, 64, dtype=np.uint8)), [(T_ETHER, 0)])        # NO_IP
        elif k == 13:
            p, h = g4[i % len(g4)]
            it = (p, h[:3] + [(T_GRE_SEQ, 38)] + h[3:])                                   # BAD_GRE: a sequence row
        items.append(it)
    select = (np.arange(n) % 17 != 5).astype(np.uint8)
    return items[:n], select


# ------------------------------------------------------------------ the host twins, called through the C ABI
SHAPES = dict(status=np.uint8, out_index=np.uint32, tunnel_out=np.uint32, out_off=np.uint64, out_len=np.uint32,
              src_index=np.uint32, oc_n_hdrs=np.uint8, oc_hdr_type=np.uint8, oc_hdr_off=np.uint16, hits=np.uint64)
PER_OUTPUT = {"dst", "out_off", "out_len", "src_index", "oc_n_hdrs", "oc_hdr_type", "oc_hdr_off"}


def counts(op, n, cap):
    c = dict(status=n, out_index=n, out_off=cap, out_len=cap, src_index=cap, oc_n_hdrs=cap, oc_hdr_type=MAXH * cap,
             oc_hdr_off=MAXH * cap, hits=NST[op])
    if op == "decap":
        c["tunnel_out"] = n
    return c


def call_args(op, head, tun, per, p, dst_len, cap, oc):
    """The argument list of pkt_tunnel_<op>_host from (batch, chain, which, flags), the handle, the per-call inputs and
    the output pointers p(name)."""
    import ctypes
    if op == "encap":
        tn, tn_all, en, ident, sel = per
        mid = [tun, tn, tn_all, en, ident, sel, p("status"), p("out_index")]
    else:
        mid = [tun, per[-1], p("status"), p("out_index"), p("tunnel_out")]
    return head + mid + [p("dst"), dst_len, cap, p("out_off"), p("out_len"), p("src_index"),
                         ctypes.byref(oc) if oc is not None else None, p("hits")]


class HostTable:
    """pkt_tunnel_create_host over `entries` (the model's dicts)."""

    def __init__(self, entries):
        import ctypes

        from pktgpu import _lib
        self.L = _lib.load()
        self.rec = records(entries)
        self.h = ctypes.c_void_p()
        rc = self.L.pkt_tunnel_create_host(self.rec.ctypes.data, len(self.rec), ctypes.byref(self.h))
        assert rc == 0, self.L.pkt_tunnel_last_error(None)

    def error(self):
        return (self.L.pkt_tunnel_last_error(self.h) or b"").decode()

    def __del__(self):
        if self.h:
            self.L.pkt_tunnel_destroy(self.h)


def host_call(op, T, b, chain, tunnel=0, entropy=None, ident=0, select=None, which=0, flags=0, cap=None, dst_len=None,
              skip=(), guard=64, over=None, handle=True):
    """pkt_tunnel_<op>_host with caller-sized outputs -> (rc, got).  cap / dst_len default to what the model-free sizing
    pass says.  skip: names of outputs passed as NULL.  Every output array has `guard` extra elements filled with 0xA5
    that must come back unchanged (got["guards"]).  over: {position in the argument list: value}."""
    import ctypes

    import pktgpu
    from pktgpu import _lib
    L = _lib.load()
    fn = getattr(L, f"pkt_tunnel_{op}_host")
    pb, keep = pktgpu._host_batch(_lib, b)
    cols = [np.ascontiguousarray(chain[k]) for k in ("n_hdrs", "hdr_type", "hdr_off")]
    ch = _lib.PktChain(*[c.ctypes.data for c in cols])
    n = b["n"]
    ad = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    tn = None if np.isscalar(tunnel) else np.ascontiguousarray(tunnel, np.uint32)
    en = None if entropy is None else np.ascontiguousarray(entropy, np.uint32)
    sel = None if select is None else np.ascontiguousarray(select, np.uint8)
    per = (ad(tn), 0 if tn is not None else int(tunnel), ad(en), ident, ad(sel))
    tot, cnt = ctypes.c_uint64(0), ctypes.c_uint64(0)
    head = [ctypes.byref(pb), ctypes.byref(ch), which, flags]
    tun = T.h if handle else None
    if cap is None or dst_len is None:
        sizing = call_args(op, [head[0], head[1], which, flags | NO_WRITE], tun, per, lambda k: None, 0, 0, None)
        rc = fn(*sizing, ctypes.byref(tot), ctypes.byref(cnt))
        assert rc == 0, T.error()
        cap = max(1, cnt.value) if cap is None else cap
        dst_len = tot.value if dst_len is None else dst_len
    cn = counts(op, n, cap)
    shapes = {k: (cn[k], SHAPES[k]) for k in cn}
    shapes["dst"] = (r16(dst_len) + 16, np.uint8)
    if flags & NO_WRITE:
        skip = set(skip) | PER_OUTPUT
    bufs = {}
    for k, (sz, dt) in shapes.items():
        if k in skip:
            continue
        a = np.full(sz + guard, 0xA5A5A5A5A5A5A5A5 & (256 ** np.dtype(dt).itemsize - 1), dt)
        if k == "hits":
            a[:sz] = 0
        bufs[k] = a
    p = lambda k: bufs[k].ctypes.data if k in bufs else None  # noqa: E731
    oc = _lib.PktChain(p("oc_n_hdrs"), p("oc_hdr_type"), p("oc_hdr_off"))
    args = call_args(op, head, tun, per, p, dst_len, cap, oc) + [ctypes.byref(tot), ctypes.byref(cnt)]
    for k, v in dict(over or {}).items():
        args[k] = v
    rc = fn(*args)
    got = {k: a[:shapes[k][0]] for k, a in bufs.items()}
    got["guards"] = all((a[shapes[k][0]:].view(np.uint8) == 0xA5).all() for k, a in bufs.items())
    got["n_out"], got["bytes_out"], got["cap"] = cnt.value, tot.value, cap
    return rc, got


def outputs(got):
    return [got["dst"][int(o):int(o) + int(ln)].tobytes() for o, ln in zip(got["out_off"][:got["n_out"]], got["out_len"])]


def out_items(got):
    """A call's outputs as items (bytes, rows): the next call's sources."""
    cap = got["cap"]
    ty, of = got["oc_hdr_type"].reshape(MAXH, cap), got["oc_hdr_off"].reshape(MAXH, cap)
    return [(p, [(int(ty[j, q]), int(of[j, q])) for j in range(int(got["oc_n_hdrs"][q]))]) for q, p in enumerate(outputs(got))]
