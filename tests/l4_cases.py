"""Batches and expected results shared by test_l4_checksum_host.py and test_l4_checksum_device.py.

A case is a dict {"batch", "chain", "which"}: a batch over numpy arrays (slab, stride or offsets / lens,
n), the chain columns of a parse of it (the Python parser model pyref) and the `which` of the call.
`expect(case)` computes pkt_l4_checksum_batch's outputs with an independent pure-Python RFC 1071
implementation (rfc1071_sum: a byte-pair big-endian loop with end-around carry over pseudo-header +
segment), packet by packet: never with pkt_l4_checksum_host or the device.  The packets' good checksums
are put in by the same yardstick (finalize); the bad ones are made by flipping bits afterwards.
"""
import struct

import numpy as np

import pyref
from pktgpu import gen, schema

import compare_cases as C
from compare_cases import batch, extents, indexed

OK, BAD, UNCHECKED, ABSENT, NO_IP, SPAN, FRAGMENT = range(7)
LAST = 0xFF
T_IPV4, T_IPV6, T_ICMP, T_TCP, T_UDP = (schema.HDR_ID[k] for k in ("IPv4", "IPv6", "ICMP", "TCP", "UDP"))
L4_SIZE = {T_ICMP: 4, T_TCP: 20, T_UDP: 8}
FIELD = {T_ICMP: 2, T_TCP: 16, T_UDP: 6}
PROTO = {T_TCP: 6, T_UDP: 17, T_ICMP: 58}
M1, M2 = "00:01:02:03:04:05", "00:06:07:08:09:0a"


# ------------------------------------------------------------------ the yardstick
def rfc1071_sum(data):
    """The one's-complement sum of the 16-bit big-endian words of `data` (an odd last byte padded with
    zero), with end-around carry: RFC 1071 section 1, steps (1) and (2)."""
    s = 0
    for k in range(0, len(data), 2):
        s += (data[k] << 8) | (data[k + 1] if k + 1 < len(data) else 0)
        s = (s & 0xFFFF) + (s >> 16)
    return s


def pin_yardstick():
    """RFC 1071 section 3's example: 00 01 f2 03 f4 f5 f6 f7 sum to ddf2, checksum 220d."""
    s = rfc1071_sum(bytes.fromhex("0001f203f4f5f6f7"))
    assert s == 0xDDF2 and (~s & 0xFFFF) == 0x220D
    assert rfc1071_sum(b"\xff\xff\x00\x01") == 1 and rfc1071_sum(b"\x01") == 0x0100 and rfc1071_sum(b"") == 0


def one(p, hdrs, which):
    """(status, calc, stored, the field's offset in the packet or None) of packet bytes `p` whose chain
    is hdrs = [(type id, offset)], by the contract in include/pktgpu.h."""
    l4 = [j for j, (t, _) in enumerate(hdrs) if t in L4_SIZE]
    if which == LAST:
        l4 = l4[-1:]
    elif which < len(l4):
        l4 = [l4[which]]
    else:
        l4 = []
    if not l4:
        return ABSENT, 0, 0, None
    j = l4[0]
    t, s = hdrs[j]
    if j == 0 or hdrs[j - 1][0] not in (T_IPV4, T_IPV6):
        return NO_IP, 0, 0, None
    ipt, ip = hdrs[j - 1]
    v4 = ipt == T_IPV4
    if ip + (20 if v4 else 40) > len(p):
        return SPAN, 0, 0, None
    if v4 and struct.unpack_from(">H", p, ip + 6)[0] & 0x3FFF:
        return FRAGMENT, 0, 0, None
    e = ip + struct.unpack_from(">H", p, ip + 2)[0] if v4 else ip + 40 + struct.unpack_from(">H", p, ip + 4)[0]
    if e > len(p) or e < s + L4_SIZE[t]:
        return SPAN, 0, 0, None
    f = s + FIELD[t]
    seg = bytearray(p[s:e])
    seg[FIELD[t]:FIELD[t] + 2] = b"\0\0"
    if v4:
        pseudo = b"" if t == T_ICMP else p[ip + 12:ip + 20] + struct.pack(">BBH", 0, PROTO[t], e - s)
    else:
        pseudo = p[ip + 8:ip + 40] + struct.pack(">IBBBB", e - s, 0, 0, 0, PROTO[t])
    calc = ~rfc1071_sum(bytes(pseudo) + bytes(seg)) & 0xFFFF
    if t == T_UDP and calc == 0:
        calc = 0xFFFF
    stored = struct.unpack_from(">H", p, f)[0]
    if t == T_UDP and stored == 0:
        st = UNCHECKED if v4 else BAD
    else:
        st = OK if stored == calc or (stored == 0xFFFF and calc == 0) else BAD
    return st, calc, stored, f


def hdrs_of(p, entry="parse"):
    return [(schema.HDR_ID[name], o) for name, o in pyref.parse(p, entry)[1]]


def finalize(p, which=LAST, entry="parse"):
    """`p` with the yardstick's checksum stored in its `which` L4 header (unchanged where there is none)."""
    st, calc, stored, f = one(p, hdrs_of(p, entry), which)
    if f is None:
        return bytes(p)
    q = bytearray(p)
    q[f:f + 2] = struct.pack(">H", calc)
    return bytes(q)


def chain_of(b, entry="parse"):
    """The chain columns of a parse of b with `entry`, by the Python model of the parser (slot-major)."""
    n = b["n"]
    nh = np.zeros(n, np.uint8)
    ty = np.zeros((schema.MAX_HDRS, n), np.uint8)
    of = np.zeros((schema.MAX_HDRS, n), np.uint16)
    for i, p in enumerate(C.packets(b)):
        hdrs = hdrs_of(p, entry)
        nh[i] = len(hdrs)
        for j, (t, o) in enumerate(hdrs):
            ty[j, i] = t
            of[j, i] = o
    return dict(n_hdrs=nh, hdr_type=ty, hdr_off=of)


def case(b, which=0, entry="parse", chain=None):
    return dict(batch=b, chain=chain_of(b, entry) if chain is None else chain, which=which)


def expect(c, update=False, keep=False):
    """calc, stored, status of the case and, for an UPDATE call, the slab afterwards."""
    b, ch = c["batch"], c["chain"]
    n = b["n"]
    calc, stored, status = np.zeros(n, np.uint16), np.zeros(n, np.uint16), np.zeros(n, np.uint8)
    slab = b["slab"].copy()
    for i, (o, ln) in enumerate(extents(b)):
        p = b["slab"][o:o + ln].tobytes()
        hdrs = [(int(ch["hdr_type"][j, i]), int(ch["hdr_off"][j, i])) for j in range(min(int(ch["n_hdrs"][i]), schema.MAX_HDRS))]
        status[i], calc[i], stored[i], f = one(p, hdrs, c["which"])
        if update and f is not None and not (keep and status[i] == UNCHECKED):
            slab[o + f] = calc[i] >> 8
            slab[o + f + 1] = calc[i] & 0xFF
    return dict(calc=calc, stored=stored, status=status, slab=slab)


def check(got, want, label=""):
    for name in ("calc", "stored", "status"):
        if got.get(name) is None:
            continue
        g = np.asarray(got[name])
        bad = np.flatnonzero(g != want[name])
        assert bad.size == 0, (label, name, "first bad packets", bad[:8], g[bad[:8]], want[name][bad[:8]],
                               want["status"][bad[:8]])


# ------------------------------------------------------------------ packets
def pkt(l4, v6=False, vlans=0, payload=b"", frag=0x4000, sport=1234, dport=80, src=None, dst=None):
    """Ether / `vlans` x Vlan / IPv4 | IPv6 / TCP | UDP | ICMP / payload from gen.py's header builders, the
    L4 checksum field 0 (the segment starts at 34 + 4 * vlans for IPv4)."""
    p = gen.Packet()
    et = 0x86DD if v6 else 0x0800
    p.push(gen.ethernet(M1, M2, 0x8100 if vlans else et))
    for k in range(vlans):
        p.push(gen.vlan(3, 0, 10 + k, 0x8100 if k + 1 < vlans else et))
    size = L4_SIZE[schema.HDR_ID[l4]] + len(payload)
    if v6:
        p.push(gen.ipv6(4, 5, {"TCP": 6, "UDP": 17, "ICMP": 58}[l4], 64, src or "AAAA::1", dst or "BBBB::2", size))
    else:
        p.push(gen.ipv4(5, 0, 115, 64, frag, {"TCP": 6, "UDP": 17, "ICMP": 1}[l4], src or "10.10.10.1", dst or "11.11.11.1",
                        20 + size))
    if l4 == "TCP":
        p.push(gen.tcp(sport, dport, 100, 101, 5, 0, 2, 8192, 0, 0))
    elif l4 == "UDP":
        p.push(gen.udp(sport, dport, size))
    else:
        p.push(gen.icmp(8, 0))
    p.set_payload(payload)
    return p.to_vec()


def rnd(rng, k):
    return rng.integers(0, 256, k, dtype=np.uint8).tobytes()


def put16(p, at, v):
    q = bytearray(p)
    q[at:at + 2] = struct.pack(">H", v & 0xFFFF)
    return bytes(q)


def zero_sum(p):
    """`p` (two zero bytes at its end, L4 field 0) with those two bytes set so that the whole sum folds to
    0xFFFF: calc = ~0xFFFF = 0, which UDP sends as 0xFFFF."""
    st, calc, stored, f = one(p, hdrs_of(p), LAST)
    s = ~calc & 0xFFFF  # the fold of the sum
    return put16(p, len(p) - 2, 0xFFFF - s if s != 0xFFFF else 0)


PAY_LENS = [0, 1, 15, 16, 17, 33]


def protocol_packets(rng):
    """TCP, UDP and ICMP over IPv4 and IPv6 with 0, 1 and 2 Vlan tags at the payload lengths of PAY_LENS
    (header only, an odd tail, around a chunk edge), good checksums."""
    out = []
    for l4 in ("TCP", "UDP", "ICMP"):
        for v6 in (False, True):
            for vlans in (0, 1, 2):
                for pl in PAY_LENS:
                    out.append(finalize(pkt(l4, v6, vlans, rnd(rng, pl), sport=int(rng.integers(1, 65536)))))
    return out


def specials(rng):
    """name -> packet: the hand-made ones, each with the status it must get."""
    ref = [bytes(p.to_vec()) for p in gen.reference_22_packets()]
    sp = {}
    good = finalize(pkt("UDP", payload=rnd(rng, 40)))
    sp["udp4_good"] = (good, OK)
    sp["all_ff"] = (finalize(pkt("TCP", payload=b"\xff" * 1461)), OK)
    sp["udp4_sum_ffff"] = (put16(zero_sum(pkt("UDP", payload=rnd(rng, 30) + b"\0\0")), 40, 0xFFFF), OK)  # calc reads 0xFFFF
    z = zero_sum(pkt("TCP", payload=rnd(rng, 30) + b"\0\0"))
    sp["tcp4_calc0_stored0"] = (z, OK)
    sp["tcp4_calc0_storedffff"] = (put16(z, 34 + 16, 0xFFFF), OK)
    pad = finalize(pkt("UDP", payload=rnd(rng, 4)))                    # 46 bytes, padded to 60 with non-zero bytes
    sp["padded60"] = (pad + bytes(range(0x81, 0x81 + 14)), OK)
    sp["total_len_past"] = (put16(good, 16, len(good) - 14 + 1), SPAN)
    sp["total_len_short_udp"] = (put16(good, 16, 20 + 8 - 1), SPAN)
    sp["total_len_short_tcp"] = (put16(finalize(pkt("TCP", payload=rnd(rng, 9))), 16, 20 + 20 - 1), SPAN)
    sp["total_len_header_only"] = (put16(good, 16, 20 + 8), BAD)        # e = s + 8: summed, no longer the sender's sum
    sp["v6_payload_len_0"] = (put16(finalize(pkt("TCP", True, payload=rnd(rng, 9))), 14 + 4, 0), SPAN)
    sp["v6_payload_len_past"] = (put16(finalize(pkt("UDP", True, payload=rnd(rng, 9))), 14 + 4, 18), SPAN)
    sp["mf_set"] = (finalize(pkt("UDP", payload=rnd(rng, 20), frag=0x2000)), FRAGMENT)
    sp["frag_offset_1"] = (finalize(pkt("TCP", payload=rnd(rng, 20), frag=0x0001)), FRAGMENT)
    sp["df_only"] = (finalize(pkt("TCP", payload=rnd(rng, 20), frag=0x4000)), OK)
    sp["reserved_flag_only"] = (finalize(pkt("TCP", payload=rnd(rng, 20), frag=0x8000)), OK)
    sp["udp4_stored_0"] = (pkt("UDP", payload=rnd(rng, 21)), UNCHECKED)
    sp["udp6_stored_0"] = (pkt("UDP", True, payload=rnd(rng, 21)), BAD)
    sp["payload_bit"] = (C.flip(finalize(pkt("TCP", payload=rnd(rng, 100))), 54 + 77, 0x10), BAD)
    sp["v6_address_bit"] = (C.flip(finalize(pkt("ICMP", True, payload=rnd(rng, 12))), 14 + 8 + 31, 0x01), BAD)
    sp["v4_address_bit"] = (C.flip(finalize(pkt("UDP", payload=rnd(rng, 12))), 14 + 15, 0x40), BAD)
    sp["icmp4_all_zero"] = (put16(put16(pkt("ICMP"), 34, 0), 36, 0xFFFF), OK)  # the sum is 0: calc 0xFFFF
    sp["icmp4_all_zero_stored_0"] = (put16(pkt("ICMP"), 34, 0), BAD)
    sp["truncated"] = (ref[0][:20], ABSENT)                              # n_hdrs 0
    sp["arp"] = (bytes(gen.create_arp_packet(M1, M2, False, 0, 0, 1, M1, M2, "10.0.0.1", "10.0.0.2", b"").to_vec()), ABSENT)
    inner = gen.test_tcp_packet_with_payload(rnd(rng, 57))
    inner.remove(0)                                                      # IP-in-IP carries no inner Ether
    ipip = gen.create_ipv4ip_packet(M1, M2, False, 10, 3, 5, "192.168.0.199", "192.168.0.1", 0, 64, 0, 0x4000, [], inner)
    sp["ip_in_ip"] = (finalize(bytes(ipip.to_vec())), OK)
    inner6 = gen.create_udpv6_packet(M1, M2, False, 10, 3, 4, 5, 64, "AAAA::1", "BBBB::1", 1234, 9090, False, rnd(rng, 18))
    inner6.remove(0)
    ip6ip = gen.create_ipv4ip_packet(M1, M2, True, 10, 3, 5, "192.168.0.199", "192.168.0.1", 0, 64, 0, 0x4000, [], inner6)
    sp["ip6_in_ip4"] = (finalize(bytes(ip6ip.to_vec())), OK)
    sp["ip_in_ip_outer_mf"] = (finalize(put16(bytes(ipip.to_vec()), 14 + 6, 0x2000)), OK)  # the outer IP is not consulted
    return sp


def vxlan_packets(rng, k=20):
    """VXLAN packets (outer UDP at 0, inner TCP at 1 = LAST), both checksums good, between plain TCP ones."""
    out = []
    for i in range(k):
        inner = gen.test_tcp_packet_with_payload(rnd(rng, int(rng.integers(0, 90))))
        v = gen.create_vxlan_packet(M1, M2, False, 10, 3, 5, "192.168.0.199", "192.168.0.1", 0, 64, 0, 0x4000, [],
                                    gen.VXLAN_PORT, 9090, False, 2000 + i, inner)
        out.append(finalize(finalize(bytes(v.to_vec()), 1), 0))
        if i % 3 == 0:
            out.append(finalize(pkt("TCP", payload=rnd(rng, 10))))
    return out


def long_packet():
    """A 65535-byte TCP/IPv4 packet, all-0xFF payload: the largest segment and the largest sum."""
    return finalize(pkt("TCP", payload=b"\xff" * (65535 - 54)))


def c2_patched(n, seed):
    """gen_c2's n x 64 B Ether/IPv4/UDP packets at fixed stride 64 (every chunk count equal: the uniform
    walk): a third keep the stored 0 (UNCHECKED), a third get the good checksum, the rest a random one."""
    a = gen.gen_c2(n, seed=seed)
    rng = np.random.default_rng(seed)
    for i in range(n):
        m = (i + seed) % 3
        if m == 1:
            a[i] = np.frombuffer(finalize(a[i].tobytes()), np.uint8)
        elif m == 2:
            a[i, 40:42] = rng.integers(1, 256, 2)
    return a


# ------------------------------------------------------------------ the table
def build():
    rng = np.random.default_rng(1071)
    cs = {}
    prot = protocol_packets(rng)
    cs["protocols"] = case(indexed(prot, rng))
    sp = specials(rng)
    cs["specials"] = dict(case(indexed([p for p, _ in sp.values()], rng), LAST), names=list(sp), known=[s for _, s in sp.values()])
    # every offset mod 16, twice: a UDP/IPv4 packet of 63 bytes and a TCP/IPv6 one whose segment ends on a
    # 16-byte boundary of the slab at that alignment
    al, pk = [], []
    for a in range(16):
        pk.append(finalize(pkt("UDP", payload=rnd(rng, 21))))
        al.append(a)
        pk.append(finalize(pkt("TCP", True, payload=rnd(rng, (16 - (a + 74) % 16) % 16 + 16))))
        al.append(a)
    cs["every_alignment"] = case(indexed(pk, rng, align=al))
    for i, (o, ln) in enumerate(extents(cs["every_alignment"]["batch"])):
        assert o % 16 == al[i] and (i % 2 == 0 or (o + ln) % 16 == 0)
    for n in (1, 63, 64, 65, 1000):
        cs[f"c2_stride64_{n}"] = case(batch(c2_patched(n, 7 + n), stride=64))
    # stride 61: 61-byte UDP packets back to back, every packet at another alignment
    s61 = [finalize(pkt("UDP", payload=rnd(rng, 19), sport=i + 1)) for i in range(65)]
    assert all(len(p) == 61 for p in s61)
    cs["stride61"] = case(batch(np.frombuffer(b"".join(s61), np.uint8), stride=61))
    # a 65535-byte packet among 64-byte ones in one wave, a second wave of short ones
    mix = [finalize(pkt("UDP", payload=rnd(rng, 22))) for _ in range(130)]
    mix[3] = long_packet()
    mix[70] = C.flip(long_packet(), 65534, 0x01)
    cs["long_among_short"] = case(indexed(mix, rng))
    vx = vxlan_packets(rng)
    vb = indexed(vx, rng)
    for w in (0, 1, 2, LAST):
        cs[f"vxlan_which_{w}"] = case(vb, w)
    # entry parse_tcp: a list of one TCP header, no IP before it
    cs["no_ip"] = case(indexed([gen.tcp(1, 2, 3, 4, 5, 0, 2, 100, 0, 0).data + rnd(rng, 12) for _ in range(5)], rng), 0, "parse_tcp")
    # the last packet's lens run past the slab end: clamped, its IP length then passes the packet
    cl = indexed([finalize(pkt("TCP", payload=rnd(rng, 30))) for _ in range(3)], rng)
    cl["slab"] = cl["slab"][:int(cl["offsets"][2]) + 70]
    cs["clamped"] = case(cl, 0, chain=chain_of(dict(cl, slab=np.concatenate([cl["slab"], np.zeros(64, np.uint8)]))))
    # 1000 packets of everything above, shuffled, some with a flipped bit
    pool = prot + [p for p, _ in sp.values()] + vx
    pick = rng.integers(0, len(pool), 1000)
    mixed = []
    for k, j in enumerate(pick):
        p = pool[int(j)]
        if k % 5 == 0 and len(p) > 60:
            p = C.flip(p, int(rng.integers(54, len(p))), 1 << int(rng.integers(0, 8)))
        mixed.append(p)
    cs["mixed_1000"] = case(indexed(mixed, rng), LAST)
    # s is the chain's hdr_off, not IP + 20: IPv4 / IPv6 packets with 4 and 8 bytes between the IP header and
    # the L4 header (an IPv4 option; a gap) and hand-made chains that say so, good checksums over [s, e)
    gp, gh = [], []
    for k in range(40):
        l4, v6, gap = ("TCP", "UDP", "ICMP")[k % 3], k % 2 == 1, 4 + 4 * (k % 2 == 0 and k % 4 == 0) + (k % 5 == 0)
        p = bytearray(pkt(l4, v6, payload=rnd(rng, 5 + k)))
        ip = 14
        at = ip + (40 if v6 else 20)
        p[at:at] = rnd(rng, gap)
        if v6:
            p[ip + 4:ip + 6] = struct.pack(">H", len(p) - ip - 40)
        else:
            p[ip + 2:ip + 4] = struct.pack(">H", len(p) - ip)
        hd = [(schema.HDR_ID["Ether"], 0), (T_IPV6 if v6 else T_IPV4, ip), (schema.HDR_ID[l4], at + gap)]
        st, calc, stored, f = one(bytes(p), hd, 0)
        p[f:f + 2] = struct.pack(">H", calc if k % 7 else calc ^ 0x0100)
        gp.append(bytes(p))
        gh.append(hd)
    gb = indexed(gp, rng)
    gch = dict(n_hdrs=np.full(40, 3, np.uint8), hdr_type=np.zeros((schema.MAX_HDRS, 40), np.uint8),
               hdr_off=np.zeros((schema.MAX_HDRS, 40), np.uint16))
    for i, hd in enumerate(gh):
        for j, (t, o) in enumerate(hd):
            gch["hdr_type"][j, i], gch["hdr_off"][j, i] = t, o
    cs["chain_offset"] = case(gb, 0, chain=gch)
    e = batch(np.zeros(0, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint32))
    cs["empty_batch"] = case(e)
    return cs


CASE_NAMES = ["protocols", "specials", "every_alignment", "c2_stride64_1", "c2_stride64_63", "c2_stride64_64",
              "c2_stride64_65", "c2_stride64_1000", "stride61", "long_among_short", "vxlan_which_0", "vxlan_which_1",
              "vxlan_which_2", "vxlan_which_255", "no_ip", "clamped", "mixed_1000", "chain_offset", "empty_batch"]

_CASES = None


def all_cases():
    """name -> (case, expected, expected after UPDATE, expected after UPDATE | KEEP_ZERO_UDP): built once and
    shared; nothing may change them."""
    global _CASES
    if _CASES is None:
        _CASES = {k: (c, expect(c), expect(c, True), expect(c, True, True)) for k, c in build().items()}
    return _CASES
