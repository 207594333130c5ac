"""Batches, expected flow keys and the table model shared by test_flow_host.py and test_flow_device.py.

The yardstick is independent of the library: `one` reads packet bytes and the chain and builds the 40-byte
key by the contract in include/pktgpu.h, `splitmix64` / `flow_hash` work on Python ints, `toeplitz` is the
bitwise definition over a Python big integer (checked against tests/golden/rss_vectors.json, the Microsoft
"verifying the RSS hash calculation" table), and `TableModel` is a dict from tag to record that returns, per
packet, the expected status and its flow, and per flow the record.  Nothing here calls pkt_flow_key_host, the
host table or the device.
"""
import ipaddress
import json
import os
import struct

import numpy as np

from pktgpu import gen, schema

import compare_cases as C
import l4_cases as L4
import pktgen_templates as T
from compare_cases import batch, extents, indexed

OK, NO_IP, SPAN = range(3)
UPD_OK, UPD_SKIPPED, UPD_COLLISION, UPD_FULL = range(4)
LAST = 0xFF
NONE = 0xFFFFFFFF
T_IPV4, T_IPV6, T_TCP, T_UDP = (schema.HDR_ID[k] for k in ("IPv4", "IPv6", "TCP", "UDP"))
M64 = (1 << 64) - 1
SEED = 0x0123456789ABCDEF
GOLD = os.path.join(C.GOLD, "rss_vectors.json")


def rss_gold():
    g = json.load(open(GOLD))
    return bytes.fromhex(g["key"]), g["vectors"]


RSS_KEY = rss_gold()[0]


# ------------------------------------------------------------------ the yardstick
def splitmix64(x):
    z = (x + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def pin_yardstick():
    """splitmix64's published first output for state 0, and the Toeplitz table."""
    assert splitmix64(0) == 0xE220A8397B1DCDAF
    key, vec = rss_gold()
    assert len(key) == 40 and len(vec) == 8
    for v in vec:
        s, d = ipaddress.ip_address(v["src"]).packed, ipaddress.ip_address(v["dst"]).packed
        assert toeplitz(key, s + d) == int(v["addr_only"], 16), v
        assert toeplitz(key, s + d + struct.pack(">HH", v["sport"], v["dport"])) == int(v["with_ports"], 16), v


def flow_hash(seed, key):
    h = seed
    for w in struct.unpack("<5Q", key):
        h = splitmix64(h ^ w)
    return h


def toeplitz(key, data):
    """For each set input bit b, MSB first, the 32 bits of `key` that start at bit b, XORed together."""
    kbits = 8 * len(key)
    k = int.from_bytes(key, "big") << 64  # bits past the key's end are zero
    kbits += 64
    r = 0
    for b in range(8 * len(data)):
        if data[b >> 3] & (0x80 >> (b & 7)):
            r ^= (k >> (kbits - 32 - b)) & 0xFFFFFFFF
    return r


def one(p, hdrs, which_ip=LAST, symmetric=False, ports=True, seed=SEED, rss_key=RSS_KEY):
    """{status, key (40 bytes), hash, rss, dir} of packet bytes `p` whose chain is hdrs = [(type id, offset)]."""
    zero = dict(status=NO_IP, key=bytes(40), hash=0, rss=0, dir=0)
    ips = [j for j, (t, _) in enumerate(hdrs) if t in (T_IPV4, T_IPV6)]
    if which_ip == LAST:
        ips = ips[-1:]
    elif which_ip < len(ips):
        ips = [ips[which_ip]]
    else:
        ips = []
    if not ips:
        return zero
    j = ips[0]
    t, ip = hdrs[j]
    v4 = t == T_IPV4
    if ip + (20 if v4 else 40) > len(p):
        return dict(zero, status=SPAN)
    a = 4 if v4 else 16
    at = ip + (12 if v4 else 8)
    src, dst = p[at:at + a], p[at + a:at + 2 * a]
    take = ports and j + 1 < len(hdrs) and hdrs[j + 1][0] in (T_TCP, T_UDP)
    if take and v4 and struct.unpack_from(">H", p, ip + 6)[0] & 0x3FFF:
        take = False
    sp = dp = b"\0\0"
    if take:
        l4 = hdrs[j + 1][1]
        if l4 + 4 > len(p):
            return dict(zero, status=SPAN)
        sp, dp = p[l4:l4 + 2], p[l4 + 2:l4 + 4]
    d = 0
    if symmetric and src.ljust(16, b"\0") + sp > dst.ljust(16, b"\0") + dp:
        src, dst, sp, dp, d = dst, src, dp, sp, 1
    key = src.ljust(16, b"\0") + dst.ljust(16, b"\0") + struct.pack("<HHBBH", int.from_bytes(sp, "big"),
                                                                     int.from_bytes(dp, "big"), p[ip + (9 if v4 else 6)],
                                                                     4 if v4 else 6, 0)
    data = src + dst + (sp + dp if take else b"")
    assert len(data) in (8, 12, 32, 36)
    return dict(status=OK, key=key, hash=flow_hash(seed, key), rss=toeplitz(rss_key, data) if rss_key else 0, dir=d)


def chain_rows(ch, i):
    return [(int(ch["hdr_type"][j, i]), int(ch["hdr_off"][j, i])) for j in range(min(int(ch["n_hdrs"][i]), schema.MAX_HDRS))]


def expect(c, **over):
    """keys, hash, rss, dir, plen, status of the case (its own options, or `over`)."""
    b, ch = c["batch"], c["chain"]
    opt = dict(c["opt"], **over)
    n = b["n"]
    res = dict(keys=np.zeros((n, 40), np.uint8), hash=np.zeros(n, np.uint64), rss=np.zeros(n, np.uint32),
               dir=np.zeros(n, np.uint8), plen=np.zeros(n, np.uint32), status=np.zeros(n, np.uint8))
    for i, (o, ln) in enumerate(extents(b)):
        r = one(b["slab"][o:o + ln].tobytes(), chain_rows(ch, i), **opt)
        res["keys"][i] = np.frombuffer(r["key"], np.uint8)
        res["hash"][i], res["rss"][i], res["dir"][i], res["status"][i], res["plen"][i] = r["hash"], r["rss"], r["dir"], r["status"], ln
    return res


def check(got, want, label=""):
    for name in ("status", "plen", "dir", "keys", "hash", "rss"):
        if got.get(name) is None:
            continue
        g = np.asarray(got[name])
        if g.shape[0] == 0:
            continue
        bad = np.flatnonzero((g != want[name]).reshape(g.shape[0], -1).any(axis=1))
        assert bad.size == 0, (label, name, "first bad packets", bad[:8], g[bad[:8]], want[name][bad[:8]],
                               want["status"][bad[:8]])


class TableModel:
    """tag -> [key, first, pkts[2], bytes[2]].  An entry belongs to one tag and keeps the key of the first
    packet that reached it; the table is full when it holds `slots` entries (linear probing visits every slot,
    so a new tag finds a free one exactly while there is one)."""

    def __init__(self, slots, tag_bits=64):
        self.slots, self.tag_bits, self.e, self.hwm = slots, tag_bits, {}, 0

    def update(self, keys, hash, dir=None, weight=None, status=None, base=0):
        """(flow, upd_status): flow[i] = the `first` of packet i's entry (its name, the same from run to run),
        -1 unless UPD_OK."""
        n = len(hash)
        assert base >= self.hwm
        self.hwm = base + n
        flow, upd = np.full(n, -1, np.int64), np.zeros(n, np.uint8)
        mask = (1 << self.tag_bits) - 1
        for i in range(n):
            if status is not None and status[i]:
                upd[i] = UPD_SKIPPED
                continue
            tag = (int(hash[i]) & mask) or 1
            k = keys[i].tobytes()
            e = self.e.get(tag)
            if e is None:
                if len(self.e) == self.slots:
                    upd[i] = UPD_FULL
                    continue
                e = self.e[tag] = [k, base + i, [0, 0], [0, 0]]
            if e[0] != k:
                upd[i] = UPD_COLLISION
                continue
            d = int(dir[i]) & 1 if dir is not None else 0
            e[2][d] += 1
            e[3][d] += int(weight[i]) if weight is not None else 0
            flow[i] = e[1]
        return flow, upd

    def records(self):
        """The records sorted by first, as FlowTable.flows() gives them."""
        es = sorted(self.e.values(), key=lambda e: e[1])
        return dict(key=np.array([np.frombuffer(e[0], np.uint8) for e in es], np.uint8).reshape(-1, 40),
                    first=np.array([e[1] for e in es], np.uint64),
                    pkts=np.array([e[2] for e in es], np.uint64).reshape(-1, 2),
                    bytes=np.array([e[3] for e in es], np.uint64).reshape(-1, 2))


def same_partition(flow_id, flow):
    """flow_id (slots, NONE where not counted) splits the packets exactly as the model's flow names do."""
    flow_id, flow = np.asarray(flow_id).astype(np.int64), np.asarray(flow)
    if not np.array_equal(flow_id == NONE, flow < 0):
        return False
    m = flow >= 0
    pairs = np.unique(np.stack([flow_id[m], flow[m]], axis=1), axis=0)
    return len(np.unique(pairs[:, 0])) == len(pairs) == len(np.unique(pairs[:, 1]))


def check_records(got, want, label=""):
    for name in ("first", "key", "pkts", "bytes"):
        assert got[name].shape == want[name].shape and np.array_equal(got[name], want[name]), (label, name, got[name][:4], want[name][:4])


def synth_keys(rng, n_flows, v6_every=3):
    """n_flows distinct well-formed keys (uint8 [n_flows, 40]) and their hashes under SEED."""
    keys = np.zeros((n_flows, 40), np.uint8)
    for f in range(n_flows):
        v6 = f % v6_every == 0
        a = 16 if v6 else 4
        keys[f, 0:a] = rng.integers(0, 256, a)
        keys[f, 16:16 + a] = rng.integers(0, 256, a)
        keys[f, 32:36] = rng.integers(0, 256, 4)
        keys[f, 36] = 6 if f % 2 else 17
        keys[f, 37] = 6 if v6 else 4
        keys[f, 12:16] = np.frombuffer(struct.pack("<I", f), np.uint8) if v6 else 0  # distinct whatever the draw
        if not v6:
            keys[f, 32:36] = np.frombuffer(struct.pack("<I", f ^ 0x5A5A0000), np.uint8)
    assert len({k.tobytes() for k in keys}) == n_flows
    return keys, np.array([flow_hash(SEED, k.tobytes()) for k in keys], np.uint64)


def traffic(rng, n, n_flows, both_dirs=True):
    """n packets over n_flows synthetic flows in random order: a flow_keys-style dict and the flow of each."""
    fk, fh = synth_keys(rng, n_flows)
    f = rng.integers(0, n_flows, n)
    f[:min(n, n_flows)] = rng.permutation(n_flows)[:min(n, n_flows)]  # every flow at least once where n allows
    return dict(keys=fk[f].copy(), hash=fh[f].copy(), dir=(rng.integers(0, 2, n) if both_dirs else np.zeros(n)).astype(np.uint8),
                plen=rng.integers(60, 1515, n).astype(np.uint32), status=np.zeros(n, np.uint8)), f


def check_full(table, k, upd, fid, slots):
    """A full table's properties, whoever lost: `slots` flows stored, every FULL packet's key absent from the
    export, every OK packet's key present, the counters exact for the stored flows."""
    rec = table.flows()
    stored = {r.tobytes(): j for j, r in enumerate(rec["key"])}
    assert table.count() == slots == len(stored)
    pk, by = np.zeros((slots, 2), np.uint64), np.zeros((slots, 2), np.uint64)
    for i in range(len(upd)):
        key = k["keys"][i].tobytes()
        if upd[i] == UPD_FULL:
            assert key not in stored and fid[i] == NONE
        else:
            assert upd[i] == UPD_OK and key in stored
            pk[stored[key], k["dir"][i]] += 1
            by[stored[key], k["dir"][i]] += k["plen"][i]
    assert np.array_equal(rec["pkts"], pk) and np.array_equal(rec["bytes"], by)


# ------------------------------------------------------------------ packets
def hdrs_of(p, entry="parse"):
    return L4.hdrs_of(p, entry)


def chain_from(n, rows):
    """Chain columns from per-packet [(type, offset)] lists."""
    ch = dict(n_hdrs=np.zeros(n, np.uint8), hdr_type=np.zeros((schema.MAX_HDRS, n), np.uint8),
              hdr_off=np.zeros((schema.MAX_HDRS, n), np.uint16))
    for i, hd in enumerate(rows):
        ch["n_hdrs"][i] = len(hd)
        for j, (t, o) in enumerate(hd[:schema.MAX_HDRS]):
            ch["hdr_type"][j, i], ch["hdr_off"][j, i] = t, o
    return ch


def case(b, which_ip=LAST, symmetric=False, ports=True, chain=None, entry="parse"):
    return dict(batch=b, chain=L4.chain_of(b, entry) if chain is None else chain,
                opt=dict(which_ip=which_ip, symmetric=symmetric, ports=ports))


def pkt(l4, v6=False, **kw):
    return L4.pkt(l4, v6, **kw)


def vxlan(rng, i):
    inner = gen.test_tcp_packet_with_payload(L4.rnd(rng, 10 + i))
    return bytes(gen.create_vxlan_packet(L4.M1, L4.M2, False, 10, 3, 5, f"192.168.{i}.199", "192.168.0.1", 0, 64, 0, 0x4000, [],
                                         gen.VXLAN_PORT, 9000 + i, False, 2000 + i, inner).to_vec())


def protocol_packets(rng):
    out = []
    for l4 in ("TCP", "UDP", "ICMP"):
        for v6 in (False, True):
            for vlans in (0, 1, 3):  # 3 Vlan tags: the IP entry sits at slot 4, past the rows loaded up front
                out.append(pkt(l4, v6, vlans=vlans, payload=L4.rnd(rng, int(rng.integers(0, 40))),
                               sport=int(rng.integers(1, 65536)), dport=int(rng.integers(1, 65536))))
    out.append(bytes(T.template_bytes("greip4")))   # GRE: no ports at which_ip 0; the inner TCP at LAST
    out.append(bytes(T.template_bytes("greip6")))
    out.append(bytes(T.template_bytes("ip4ip4")))
    out.append(bytes(T.template_bytes("ip6ip4")))
    out.append(bytes(T.template_bytes("arp_req")))  # NO_IP
    out.append(bytes(T.template_bytes("tcp"))[:20])  # n_hdrs 0: NO_IP
    out.append(pkt("UDP", payload=L4.rnd(rng, 20), frag=0x2000))  # MF: ports 0
    out.append(pkt("TCP", payload=L4.rnd(rng, 20), frag=0x0001))  # offset 1: ports 0
    out.append(pkt("TCP", payload=L4.rnd(rng, 20), frag=0x4000))  # DF alone: ports
    out.append(pkt("UDP", payload=L4.rnd(rng, 20), frag=0x8000))  # the reserved flag alone: ports
    return out


def symmetric_packets():
    out = []
    for v6 in (False, True):
        a, b = ("AAAA::1", "AAAA::2") if v6 else ("10.0.0.1", "10.0.0.2")
        out.append(pkt("TCP", v6, src=a, dst=b, sport=40000, dport=443))
        out.append(pkt("TCP", v6, src=b, dst=a, sport=443, dport=40000))      # the other direction
        out.append(pkt("UDP", v6, src=a, dst=a, sport=53, dport=53))          # equal endpoints
        out.append(pkt("UDP", v6, src=a, dst=a, sport=2000, dport=1000))      # equal addresses, ports decide
        out.append(pkt("UDP", v6, src=a, dst=a, sport=1000, dport=2000))
        out.append(pkt("UDP", v6, src=a, dst=a, sport=0x0100, dport=0x00FF))  # big-endian order, not little
        out.append(pkt("ICMP", v6, src=b, dst=a))
        out.append(pkt("ICMP", v6, src=a, dst=b))
    out.append(pkt("TCP", False, src="1.0.0.2", dst="2.0.0.1", sport=1, dport=2))  # the first byte decides
    out.append(pkt("TCP", False, src="2.0.0.1", dst="1.0.0.2", sport=2, dport=1))
    out.append(pkt("TCP", True, src="AAAA::1:0", dst="AAAA::2", sport=1, dport=2))  # decided in the second word
    out.append(pkt("TCP", True, src="AAAA::2", dst="AAAA::1:0", sport=2, dport=1))
    return out


def rss_packets():
    key, vec = rss_gold()
    pk = []
    for v in vec:
        v6 = ipaddress.ip_address(v["src"]).version == 6
        pk.append(pkt("TCP", v6, src=v["src"], dst=v["dst"], sport=v["sport"], dport=v["dport"]))
    return key, vec, pk


def build():
    rng = np.random.default_rng(40)
    cs = {}
    prot = protocol_packets(rng)
    pb = indexed(prot, rng)
    cs["protocols"] = case(pb)
    cs["protocols_first_ip"] = case(pb, which_ip=0)
    cs["protocols_second_ip"] = case(pb, which_ip=1)
    cs["no_ports"] = case(pb, ports=False)
    vb = indexed([vxlan(rng, i) for i in range(9)] + [pkt("TCP")], rng)
    for w in (0, 1, 2, LAST):
        cs[f"vxlan_which_{w}"] = case(vb, which_ip=w)
    sym = symmetric_packets()
    sb = indexed(sym, rng)
    cs["symmetric"] = case(sb, symmetric=True)
    cs["symmetric_no_ports"] = case(sb, symmetric=True, ports=False)
    cs["not_symmetric"] = case(sb)
    # every offset mod 16, an IPv4 and an IPv6 packet each: the address span's 1 to 4 chunks
    al = [a for a in range(16) for _ in range(2)]
    ev = [pkt("UDP" if k % 4 < 2 else "TCP", k % 2 == 1, sport=k + 1, dport=2 * k + 1) for k in range(32)]
    cs["every_alignment"] = case(indexed(ev, rng, align=al), symmetric=True)
    # fixed stride 64 (gen_c2's Ether/IPv4/UDP) at the wave and block edges, and 61-byte packets back to back
    for n in (1, 63, 64, 65, 257, 1000):
        cs[f"c2_stride64_{n}"] = case(batch(gen.gen_c2(n, seed=90 + n), stride=64), symmetric=n % 2 == 0)
    s61 = [pkt("UDP", payload=L4.rnd(rng, 19), sport=i + 1) for i in range(67)]
    assert all(len(p) == 61 for p in s61)
    cs["stride61"] = case(batch(np.frombuffer(b"".join(s61), np.uint8), stride=61))
    # SPAN: the IP header cut by the slab end (the chain is that of the whole packets) ...
    cut = indexed([pkt("TCP", payload=L4.rnd(rng, 30)), pkt("UDP", True), pkt("TCP")], rng, align=[3, 9, 5])
    whole = L4.chain_of(cut)
    cs["span_slab_end"] = case(dict(cut, slab=cut["slab"][:int(cut["offsets"][2]) + 14 + 19]), chain=whole)
    cs["span_slab_end_ports"] = case(dict(cut, slab=cut["slab"][:int(cut["offsets"][2]) + 14 + 20 + 3]), chain=whole)  # 3 port bytes
    # ... by lens: the header short by one byte, whole, ports cut after 3 bytes, ports whole; IPv4 and IPv6
    lp, ll = [], []
    for v6 in (False, True):
        hs = 14 + (40 if v6 else 20)
        for ln in (hs - 1, hs, hs + 3, hs + 4, 14, 0):
            lp.append(pkt("UDP", v6, payload=L4.rnd(rng, 8)))
            ll.append(ln)
    lb = indexed(lp, rng)
    lch = L4.chain_of(lb)
    lb["lens"] = np.array(ll, np.uint32)
    cs["span_lens"] = case(lb, chain=lch)
    cs["span_lens_no_ports"] = case(lb, chain=lch, ports=False)  # ports that are not taken cannot be cut
    # ... and by the 65535 clamp: lens 70000, the IP header at 65515 (ends at the clamp: OK, ports cut: with
    # ports SPAN, without OK) and at 65516 (SPAN); an IPv6 one that ends at the clamp with its ports not asked
    big = rng.integers(0, 256, 3 * 70016, dtype=np.uint8)
    rows = []
    for k, (v6, at) in enumerate(((False, 65515), (False, 65516), (True, 65495))):
        p = pkt("TCP", v6)
        o = k * 70016
        big[o + at:o + at + len(p) - 14] = np.frombuffer(p[14:], np.uint8)
        rows.append([(schema.HDR_ID["Ether"], 0), (T_IPV6 if v6 else T_IPV4, at), (T_TCP, min(at + (40 if v6 else 20), 65535))])
    kb = batch(big, [0, 70016, 2 * 70016], [70000] * 3)
    cs["span_clamp"] = case(kb, chain=chain_from(3, rows))
    cs["span_clamp_no_ports"] = case(kb, chain=chain_from(3, rows), ports=False)
    # chains that point past the packet, that put the L4 header elsewhere (IPv4 options; a gap), that count
    # more than 16 headers, and one whose taken IP entry is the last row
    hp = [pkt("TCP", payload=L4.rnd(rng, 12)) for _ in range(8)]
    hrows = [hdrs_of(p) for p in hp]
    hrows[0] = [(schema.HDR_ID["Ether"], 0), (T_IPV4, 60000), (T_TCP, 60020)]
    hrows[1] = [(schema.HDR_ID["Ether"], 0), (T_IPV4, 14), (T_TCP, 65535)]
    hrows[2] = [(schema.HDR_ID["Ether"], 0), (T_IPV4, 14), (T_TCP, 38)]   # the ports are the bytes at 38
    hrows[3] = [(schema.HDR_ID["Ether"], 0), (T_IPV6, 65500)]
    hrows[4] = [(T_IPV4, 14)] * 16                                        # LAST: slot 15, nothing behind it
    hrows[5] = [(schema.HDR_ID["Vlan"], 0)] * 14 + [(T_IPV4, 14), (T_UDP, 34)]
    hb = indexed(hp, rng)
    hch = chain_from(8, hrows)
    hch["n_hdrs"][6] = 255                                                # taken as 16: rows 3.. are zeros
    cs["odd_chains"] = case(hb, chain=hch)
    cs["odd_chains_which_3"] = case(hb, chain=hch, which_ip=3)
    cs["odd_chains_symmetric"] = case(hb, chain=hch, symmetric=True)
    cs["empty_batch"] = case(batch(np.zeros(0, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint32)))
    return cs


CASE_NAMES = ["protocols", "protocols_first_ip", "protocols_second_ip", "no_ports", "vxlan_which_0", "vxlan_which_1",
              "vxlan_which_2", "vxlan_which_255", "symmetric", "symmetric_no_ports", "not_symmetric", "every_alignment",
              "c2_stride64_1", "c2_stride64_63", "c2_stride64_64", "c2_stride64_65", "c2_stride64_257", "c2_stride64_1000",
              "stride61", "span_slab_end", "span_slab_end_ports", "span_lens", "span_lens_no_ports", "span_clamp",
              "span_clamp_no_ports", "odd_chains", "odd_chains_which_3", "odd_chains_symmetric", "empty_batch"]

# what the hand-made cases must come to, by packet: the yardstick is itself held to the contract here
KNOWN = {
    "span_slab_end": [OK, OK, SPAN],
    "span_slab_end_ports": [OK, OK, SPAN],
    "span_lens": [SPAN, SPAN, SPAN, OK, SPAN, SPAN] * 2,        # lens == the header's end: ports taken, and cut
    "span_lens_no_ports": [SPAN, OK, OK, OK, SPAN, SPAN] * 2,
    "span_clamp": [SPAN, SPAN, SPAN],
    "span_clamp_no_ports": [OK, SPAN, OK],
    "vxlan_which_2": [NO_IP] * 10,
}

_CASES = None


def all_cases():
    """name -> (case, expected): built once and shared; nothing may change them."""
    global _CASES
    if _CASES is None:
        _CASES = {k: (c, expect(c)) for k, c in build().items()}
        assert list(_CASES) == CASE_NAMES
        for name, st in KNOWN.items():
            assert _CASES[name][1]["status"].tolist() == st, (name, _CASES[name][1]["status"].tolist())
    return _CASES
