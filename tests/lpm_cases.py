"""The yardstick and the case builders of pkt_lpm_* (tests/test_lpm_host.py, test_lpm_device.py).

The yardstick shares nothing with the library's trie: one dict of integer prefixes per (IP version, length), and a
lookup that tries the lengths from the longest to the shortest (include/pktgpu.h: "the route of the address's IP
version with the greatest plen whose first plen bits equal the address's").  Its cost is O(n x lengths).

A route here is (ver, plen, addr, nexthop) with addr the whole address as an integer, host bits zero; a probe is
(ver, addr).  to_array turns routes into pkt_lpm_route_t records, to_strings into the ("10.0.0.0/8", nexthop) form
Parser.lpm also takes.
"""
import ipaddress

import numpy as np

from pktgpu import gen, schema

import compare_cases as C
import flow_cases as F
import l4_cases as L4

OK, NO_ROUTE, NO_IP, SPAN, SKIPPED = range(5)
NONE = 0xFFFFFFFF
LAST = 0xFF
W = {4: 32, 6: 128}
T_IPV4, T_IPV6 = schema.HDR_ID["IPv4"], schema.HDR_ID["IPv6"]
NAMES = ("route", "nexthop", "plen", "status")
DT = dict(route=np.uint32, nexthop=np.uint32, plen=np.uint8, status=np.uint8)
DEFAULT = 0xDEF0


# ------------------------------------------------------------------ the yardstick
class Model:
    def __init__(self, routes, default=DEFAULT):
        self.default = default
        self.routes = list(routes)
        self.tabs = {}  # (ver, plen) -> {the first plen bits: route index}
        for i, (ver, plen, addr, nh) in enumerate(self.routes):
            t = self.tabs.setdefault((ver, plen), {})
            key = addr >> (W[ver] - plen)
            assert key not in t, "duplicate route"
            t[key] = i
        self.lengths = {v: sorted((p for (vv, p) in self.tabs if vv == v), reverse=True) for v in (4, 6)}

    def miss(self, status):
        return (NONE, self.default, 0xFF, status)

    def lookup(self, ver, addr):
        for plen in self.lengths[ver]:
            i = self.tabs[(ver, plen)].get(addr >> (W[ver] - plen))
            if i is not None:
                return (i, self.routes[i][3], plen, OK)
        return self.miss(NO_ROUTE)


def columns(rows):
    """[(route, nexthop, plen, status)] -> the four arrays."""
    a = np.array(rows, np.uint64).reshape(-1, 4)
    return {k: a[:, j].astype(DT[k]) for j, k in enumerate(NAMES)}


def expect_probes(model, probes, key_status=None):
    """What pkt_lpm_lookup_keys gives for keys made of `probes` (a version outside 4 / 6 is SKIPPED)."""
    rows = []
    for i, (ver, addr) in enumerate(probes):
        if (key_status is not None and key_status[i]) or ver not in (4, 6):
            rows.append(model.miss(SKIPPED))
        else:
            rows.append(model.lookup(ver, addr))
    return columns(rows)


def expect_batch(model, b, chain, which_ip=0, src=False):
    """What pkt_lpm_lookup_batch gives: the address taken from the packet bytes by the header's text."""
    rows = []
    n = b["n"]
    for i, (off, ln) in enumerate(C.extents(b)):
        p = b["slab"][off:off + ln].tobytes()
        nh = min(int(chain["n_hdrs"][i]), schema.MAX_HDRS)
        ips = [(int(chain["hdr_type"][j, i]), int(chain["hdr_off"][j, i])) for j in range(nh)
               if int(chain["hdr_type"][j, i]) in (T_IPV4, T_IPV6)]
        if which_ip == LAST:
            ent = ips[-1] if ips else None
        else:
            ent = ips[which_ip] if which_ip < len(ips) else None
        if ent is None:
            rows.append(model.miss(NO_IP))
            continue
        t, o = ent
        v4 = t == T_IPV4
        if o + (20 if v4 else 40) > ln:
            rows.append(model.miss(SPAN))
            continue
        at = o + ((12 if src else 16) if v4 else (8 if src else 24))
        rows.append(model.lookup(4 if v4 else 6, int.from_bytes(p[at:at + (4 if v4 else 16)], "big")))
    assert len(rows) == n
    return columns(rows)


def check(got, want, label=""):
    for name in NAMES:
        if got.get(name) is None:
            continue
        g = np.asarray(got[name])
        assert g.dtype == DT[name] and g.shape == want[name].shape, (label, name, g.dtype, g.shape)
        bad = np.flatnonzero(g != want[name])
        assert bad.size == 0, (label, name, "first bad", bad[:8], g[bad[:8]], want[name][bad[:8]], want["status"][bad[:8]])


def assert_mix(want, label):
    """The issue's floor on a random case, on the model's output alone: at least 1/4 of the probes hit, at least
    1/8 miss, and the hits cover at least 4 distinct prefix lengths."""
    st, n = want["status"], want["status"].size
    hits = st == OK
    assert hits.sum() * 4 >= n, (label, "hits", int(hits.sum()), n)
    assert (st == NO_ROUTE).sum() * 8 >= n, (label, "misses", int((st == NO_ROUTE).sum()), n)
    assert np.unique(want["plen"][hits]).size >= 4, (label, np.unique(want["plen"][hits]))


# ------------------------------------------------------------------ routes and probes in the library's forms
def mask(ver, plen, addr):
    return addr >> (W[ver] - plen) << (W[ver] - plen)


def to_array(routes):
    arr = np.zeros(len(routes), schema.LPM_ROUTE_DTYPE)
    for i, (ver, plen, addr, nh) in enumerate(routes):
        raw = addr.to_bytes(W[ver] // 8, "big")
        arr["addr"][i, :len(raw)] = np.frombuffer(raw, np.uint8)
        arr["ipver"][i], arr["plen"][i], arr["nexthop"][i] = ver, plen, nh
    return arr


def to_strings(routes):
    return [(f"{ipaddress.ip_address(a) if v == 6 else ipaddress.IPv4Address(a)}/{p}", nh) for v, p, a, nh in routes]


def keys_of(probes):
    """pkt_flow_key_t records [n, 40] with the probes as dst (src = its complement) and ipver set."""
    k = np.zeros((len(probes), 40), np.uint8)
    for i, (ver, addr) in enumerate(probes):
        nb = W.get(ver, 32) // 8
        k[i, 16:16 + nb] = np.frombuffer(addr.to_bytes(nb, "big"), np.uint8)
        k[i, 0:nb] = 255 - k[i, 16:16 + nb]
        k[i, 37] = ver
    return k


def edge_probes(routes):
    """Every prefix's first and last address and the addresses just outside both ends."""
    out = []
    for ver, plen, addr, _ in routes:
        top = (1 << W[ver]) - 1
        lo, hi = addr, addr | (top >> plen if plen else top)
        for a in (lo, hi, lo - 1, hi + 1):
            if 0 <= a <= top:
                out.append((ver, a))
    return out


# ------------------------------------------------------------------ (a) boundary tables
V4_LENS = [0, 1, 15, 16, 17, 23, 24, 25, 31, 32]
V6_LENS = [0, 1, 16, 17, 24, 25, 63, 64, 65, 120, 121, 127, 128]
A4 = 0xC6336B5D                                 # 198.51.107.93
A6 = 0x20010DB885A3C7D19F2E8A2E0370B3A5


def boundary():
    """Nested routes at every length where the layout changes level, both versions in one table."""
    routes = [(4, L, mask(4, L, A4), 400 + L) for L in V4_LENS] + [(6, L, mask(6, L, A6), 600 + L) for L in V6_LENS]
    return routes, edge_probes(routes)


def boundary_no_default():
    """The same without the /0s, so that the addresses outside the /1s miss."""
    routes = [r for r in boundary()[0] if r[1] != 0]
    return routes, edge_probes(routes)


# ------------------------------------------------------------------ (b) leaf-push cases
def ip4(s):
    return int(ipaddress.IPv4Address(s))


def ip6(s):
    return int(ipaddress.IPv6Address(s))


def leaf_push():
    """name -> (routes, probes).  The routes are in the CALLER's order, which the compiler must not depend on."""
    t = {}
    # a short route given after a longer one below it (its child exists by then) and one where no child exists
    t["short_after_long"] = [(4, 24, ip4("10.1.2.0"), 1), (4, 32, ip4("10.1.2.77"), 2), (4, 8, ip4("10.0.0.0"), 3),
                             (4, 12, ip4("172.16.0.0"), 4), (4, 16, ip4("10.1.0.0"), 5),
                             (6, 64, ip6("2001:db8:1:2::"), 6), (6, 128, ip6("2001:db8:1:2::7"), 7),
                             (6, 32, ip6("2001:db8::"), 8), (6, 20, ip6("2a00::"), 9)]
    t["short_before_long"] = list(reversed(t["short_after_long"]))
    # siblings that share a node, one of them covering the others' range in part
    t["siblings"] = [(4, 24, ip4("10.1.2.0"), 1), (4, 24, ip4("10.1.3.0"), 2), (4, 25, ip4("10.1.2.128"), 3),
                     (4, 17, ip4("10.1.0.0"), 4), (4, 23, ip4("10.1.2.0"), 5), (4, 30, ip4("10.1.2.132"), 6),
                     (6, 48, ip6("2001:db8:aa::"), 7), (6, 48, ip6("2001:db8:ab::"), 8), (6, 47, ip6("2001:db8:aa::"), 9),
                     (6, 41, ip6("2001:db8:80::"), 10)]
    t["only_32"] = [(4, 32, ip4("203.0.113.9"), 1)]
    t["only_128"] = [(6, 128, ip6("2001:db8::1:2:3"), 1)]
    t["only_defaults"] = [(4, 0, 0, 1), (6, 0, 0, 2)]
    out = {}
    for name, routes in t.items():
        probes = edge_probes(routes) + [(4, ip4("10.1.2.200")), (4, ip4("10.200.0.1")), (6, ip6("2001:db8:1:2::9")),
                                        (6, ip6("2001:db8:ffff::")), (4, 0), (6, 0)]
        out[name] = (routes, probes)
    return out


# ------------------------------------------------------------------ (c) a seeded random table
RANDOM_SEED = 20261
# prefix length -> weight: most of a real table is /24 (IPv4) and /48 (IPv6)
V4_DIST = {8: 2, 12: 2, 16: 10, 19: 4, 20: 6, 22: 10, 24: 50, 27: 3, 28: 3, 30: 2, 32: 8}
V6_DIST = {20: 2, 32: 20, 40: 5, 48: 40, 56: 8, 64: 18, 96: 2, 127: 1, 128: 4}
V4_TOPS = [10, 23, 45, 77, 100, 101, 172, 192, 198, 203, 11, 12]  # the first byte: few, so that routes nest
V6_TOPS = [0x2001, 0x2400, 0x2600, 0x2A00, 0x2A02, 0xFD00]        # the first 16 bits


def random_routes(rng, n4, n6):
    routes, seen = [], set()
    for ver, n, dist, tops, tb in ((4, n4, V4_DIST, V4_TOPS, 8), (6, n6, V6_DIST, V6_TOPS, 16)):
        lens = np.array(sorted(dist))
        p = np.array([dist[int(k)] for k in lens], float)
        k = 0
        while k < n:
            plen = int(rng.choice(lens, p=p / p.sum()))
            below = W[ver] - tb
            rest = int.from_bytes(rng.bytes(16), "big") >> (128 - below)
            # the byte below the top takes 16 values only: a route often lies inside an earlier, shorter one (a draw
            # that repeats a route is made again, with a new length)
            rest = rest & ((1 << (below - 8)) - 1) | int(rng.integers(0, 16)) * 13 % 256 << (below - 8)
            addr = int(rng.choice(tops)) << below | rest
            addr = mask(ver, plen, addr)
            if (ver, plen, addr) in seen:
                continue
            seen.add((ver, plen, addr))
            routes.append((ver, plen, addr, 1000 + len(routes)))
            k += 1
    order = rng.permutation(len(routes))
    return [routes[i] for i in order]


def random_probes(rng, routes, n):
    """Half inside a random route with random host bits, half uniform over the version's whole space."""
    out = []
    for k in range(n):
        if k % 2 == 0:
            ver, plen, addr, _ = routes[int(rng.integers(0, len(routes)))]
            host = int.from_bytes(rng.bytes(16), "big") & (((1 << W[ver]) - 1) >> plen if plen else (1 << W[ver]) - 1)
            out.append((ver, addr | host))
        else:
            ver = 4 if rng.random() < 0.6 else 6
            out.append((ver, int.from_bytes(rng.bytes(16), "big") >> (128 - W[ver])))
    return out


def random_table():
    rng = np.random.default_rng(RANDOM_SEED)
    routes = random_routes(rng, 1400, 600)
    return routes, random_probes(rng, routes, 4096)


# ------------------------------------------------------------------ (d) a larger table
LARGE_SEED = 20262


def large_table():
    """70,080 IPv4 /24s in 320 distinct /16s (219 each), 240 /16s, 60 /12s and 40 /8s: the nodes' entries pass 2^16."""
    rng = np.random.default_rng(LARGE_SEED)
    tops = rng.permutation(1 << 16)[:320]
    routes = []
    for t in tops:
        for third in rng.permutation(256)[:219]:
            routes.append((4, 24, int(t) << 16 | int(third) << 8, len(routes) & 0xFFFF))
    for t in list(tops[:120]) + list(rng.permutation(1 << 16)[:120]):
        routes.append((4, 16, int(t) << 16, 70000 + len(routes)))
    routes = list(dict.fromkeys((v, p, a) for v, p, a, _ in routes))  # a /16 drawn twice
    routes = [(v, p, a, 7 * i + 1) for i, (v, p, a) in enumerate(routes)]
    for t in rng.permutation(1 << 12)[:60]:
        routes.append((4, 12, int(t) << 20, 80000 + len(routes)))
    for t in rng.permutation(256)[:40]:
        routes.append((4, 8, int(t) << 24, 90000 + len(routes)))
    order = rng.permutation(len(routes))
    routes = [routes[i] for i in order]
    return routes, random_probes(rng, routes, 4096)


_CACHE = {}


def cached(name):
    """(routes, probes, Model, expected lookup_keys result) of boundary / boundary_no_default / random / large and of
    every leaf-push case, computed once and left unchanged."""
    if name not in _CACHE:
        if name in ("boundary", "boundary_no_default", "random", "large"):
            routes, probes = dict(boundary=boundary, boundary_no_default=boundary_no_default, random=random_table,
                                  large=large_table)[name]()
        else:
            routes, probes = leaf_push()[name]
        m = Model(routes)
        _CACHE[name] = (routes, probes, m, expect_probes(m, probes))
    return _CACHE[name]


SMALL = ["boundary", "boundary_no_default", "short_after_long", "short_before_long", "siblings", "only_32", "only_128",
         "only_defaults"]


# ------------------------------------------------------------------ packets
_TEMPLATES = {}


def template(kind):
    """(bytes, [(type, offset)]) of a packet kind, its header list by the Python model of the parser."""
    if kind not in _TEMPLATES:
        if kind == "v4":      # Ether / IPv4 / UDP
            p = L4.pkt("UDP", payload=b"lpm-v4-payload")
        elif kind == "v6":    # Ether / Vlan / IPv6 / TCP
            p = L4.pkt("TCP", v6=True, vlans=1, payload=b"lpm-v6")
        elif kind == "arp":
            p = bytes(gen.create_arp_packet(L4.M1, L4.M2, False, 0, 0, 1, L4.M2, L4.M1, "10.0.0.1", "10.0.0.2", b"").to_vec())
        elif kind == "vxlan":  # Ether / IPv4 / UDP / Vxlan / Ether / IPv4 / TCP
            p = F.vxlan(np.random.default_rng(5), 3)
        _TEMPLATES[kind] = (bytes(p), F.hdrs_of(p))
    return _TEMPLATES[kind]


def ip_slots(hdrs):
    return [(t, o) for t, o in hdrs if t in (T_IPV4, T_IPV6)]


def packet_for(probe, src_too=True):
    """The v4 / v6 template with the probe as its destination address (and its complement as the source)."""
    ver, addr = probe
    p, hdrs = template("v4" if ver == 4 else "v6")
    q = bytearray(p)
    t, o = ip_slots(hdrs)[0]
    nb, d, s = (4, o + 16, o + 12) if ver == 4 else (16, o + 24, o + 8)
    raw = addr.to_bytes(nb, "big")
    q[d:d + nb] = raw
    if src_too:
        q[s:s + nb] = bytes(255 - x for x in raw)
    return bytes(q), hdrs


def vxlan_for(outer, inner):
    """The VXLAN template with IPv4 destinations `outer` and `inner`."""
    p, hdrs = template("vxlan")
    q = bytearray(p)
    for (t, o), a in zip(ip_slots(hdrs), (outer, inner)):
        q[o + 16:o + 20] = a.to_bytes(4, "big")
    return bytes(q), hdrs


def fixed(pkts, stride):
    """Packets in fixed-stride slots (random bytes behind each), with their lengths."""
    rng = np.random.default_rng(len(pkts) + stride)
    slab = rng.integers(0, 256, len(pkts) * stride, dtype=np.uint8)
    for i, p in enumerate(pkts):
        assert len(p) <= stride
        slab[i * stride:i * stride + len(p)] = np.frombuffer(p, np.uint8)
    return C.batch(slab, lens=[len(p) for p in pkts], stride=stride, n=len(pkts))


def batch_case(items, layout="indexed", seed=7):
    """[(bytes, hdrs)] -> (batch dict, chain columns): "indexed" puts the packets back to back at random offsets
    mod 16 (a capture's layout), an integer is a fixed stride."""
    pkts = [p for p, _ in items]
    if layout == "indexed":
        b = C.indexed(pkts, np.random.default_rng(seed))
    else:
        b = fixed(pkts, layout)
    return b, F.chain_from(len(items), [h for _, h in items])


def probe_items(probes):
    return [packet_for(pr) for pr in probes]


def mixed_items(probes):
    """IPv4 / IPv6 probes with an ARP packet, a packet cut inside its IP header and a packet with no header list
    between them, so that the lanes of one wave take different depths and statuses."""
    out = []
    arp = template("arp")
    for k, pr in enumerate(probes):
        p, h = packet_for(pr)
        if k % 7 == 3:
            out.append(arp)
        elif k % 7 == 5:
            o = ip_slots(h)[0][1]
            out.append((p[:o + (19 if pr[0] == 4 else 39)], h))  # one byte short of the IP header: SPAN
        elif k % 11 == 6:
            out.append((p, []))  # n_hdrs == 0
        else:
            out.append((p, h))
    return out
