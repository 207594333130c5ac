"""The yardstick and the case builders of pkt_fwd_* (tests/test_fwd_host.py, test_fwd_device.py).

The yardstick is an independent pure-Python model written from the text of include/pktgpu.h: it never calls
pkt_fwd_host.  Given a batch, chain columns, adjacencies, the next hops (an array, or an lpm_cases.Model for the fused
route lookup) and the flags it returns the expected status / port / adj_index / counters and the expected slab, byte
for byte.

A case is a dict {"items": [(packet bytes, [(type, offset)])], "adj": [(dmac, smac, port, mtu, action)], "nexthop":
uint32 [n] or None, "routes": lpm_cases routes or None, "select": uint8 [n] or None, "which", "keep_l2"}; layout()
puts its packets into a batch, so that one case runs in every layout.
"""
import numpy as np

from pktgpu import schema

import compare_cases as C
import flow_cases as F
import l4_cases as L4
import lpm_cases as X

(OK, SKIPPED, NO_IP, SPAN, NO_ETHER, TTL, NO_ADJ, DROP, PUNT, MTU) = range(10)
NSTATUS = 10
NONE = 0xFFFFFFFF
LAST = 0xFF
FORWARD, ACT_DROP, ACT_PUNT = 0, 1, 2
T_ETHER, T_IPV4, T_IPV6 = schema.HDR_ID["Ether"], schema.HDR_ID["IPv4"], schema.HDR_ID["IPv6"]
NAMES = ("status", "port", "adj_index")
DT = dict(status=np.uint8, port=np.uint32, adj_index=np.uint32)
LPM_DEFAULT = 5  # the fused cases' default_nexthop: an adjacency of its own


# ------------------------------------------------------------------ the yardstick
def csum_1624(hc, m):
    """RFC 1624 eq. 3 for m -> m - 0x0100, as include/pktgpu.h spells it out."""
    m2 = m - 0x0100
    s = (~hc & 0xFFFF) + (~m & 0xFFFF) + m2
    s = (s & 0xFFFF) + (s >> 16)
    s = (s & 0xFFFF) + (s >> 16)
    return ~s & 0xFFFF


def one(p, hdrs, adj, a_of, which, keep_l2, selected):
    """(status, port, adj_index, [(offset in the packet, new bytes)]) of packet bytes `p` with the chain `hdrs`;
    a_of(version, destination address) gives the adjacency index."""
    if not selected:
        return SKIPPED, NONE, NONE, []
    ips = [j for j, (t, _) in enumerate(hdrs) if t in (T_IPV4, T_IPV6)]
    if which == LAST:
        ips = ips[-1:]
    else:
        ips = ips[which:which + 1]
    if not ips:
        return NO_IP, NONE, NONE, []
    j = ips[0]
    t, ip = hdrs[j]
    v4 = t == T_IPV4
    if ip + (20 if v4 else 40) > len(p):
        return SPAN, NONE, NONE, []
    eth = None
    if not keep_l2:
        before = [o for tt, o in hdrs[:j] if tt == T_ETHER]
        if not before:
            return NO_ETHER, NONE, NONE, []
        eth = before[-1]
        if eth + 14 > len(p):
            return SPAN, NONE, NONE, []
    ttl = p[ip + 8] if v4 else p[ip + 7]
    if ttl <= 1:
        return TTL, NONE, NONE, []
    a = a_of(4 if v4 else 6, int.from_bytes(p[ip + 16:ip + 20] if v4 else p[ip + 24:ip + 40], "big"))
    if a >= len(adj):
        return NO_ADJ, NONE, a, []
    dmac, smac, port, mtu, action = adj[a]
    if action == ACT_DROP:
        return DROP, NONE, a, []
    if action == ACT_PUNT:
        return PUNT, NONE, a, []
    l3 = int.from_bytes(p[ip + 2:ip + 4], "big") if v4 else 40 + int.from_bytes(p[ip + 4:ip + 6], "big")
    if mtu and l3 > mtu:
        return MTU, NONE, a, []
    wr = []
    if not keep_l2:
        wr.append((eth, bytes(dmac) + bytes(smac)))
    if v4:
        hc = csum_1624(int.from_bytes(p[ip + 10:ip + 12], "big"), int.from_bytes(p[ip + 8:ip + 10], "big"))
        wr.append((ip + 8, bytes([ttl - 1])))
        wr.append((ip + 10, hc.to_bytes(2, "big")))
    else:
        wr.append((ip + 7, bytes([ttl - 1])))
    return OK, port, a, wr


def expect(case, b, chain, write=True, nexthop="case"):
    """status, port, adj_index, hits, bytes and the slab after the call, for the case's packets laid out as `b`."""
    adj = case["adj"]
    nexthop = case["nexthop"] if isinstance(nexthop, str) else nexthop
    lpm = None
    if nexthop is None:
        lpm = lpm_model(case["routes"])
    n = b["n"]
    out = dict(status=np.zeros(n, np.uint8), port=np.zeros(n, np.uint32), adj_index=np.zeros(n, np.uint32),
               hits=np.zeros(NSTATUS, np.uint64), bytes=np.zeros(NSTATUS, np.uint64), slab=b["slab"].copy())
    sel = case.get("select")
    for i, (off, ln) in enumerate(C.extents(b)):
        p = b["slab"][off:off + ln].tobytes()
        nh = min(int(chain["n_hdrs"][i]), schema.MAX_HDRS)
        hdrs = [(int(chain["hdr_type"][j, i]), int(chain["hdr_off"][j, i])) for j in range(nh)]
        a_of = (lambda v, d: lpm.lookup(v, d)[1]) if lpm is not None else (lambda v, d, i=i: int(nexthop[i]))
        st, port, a, wr = one(p, hdrs, adj, a_of, case["which"], case["keep_l2"], sel is None or sel[i] != 0)
        out["status"][i], out["port"][i], out["adj_index"][i] = st, port, a
        out["hits"][st] += 1
        out["bytes"][st] += ln
        if write:
            for o, data in wr:
                out["slab"][off + o:off + o + len(data)] = np.frombuffer(data, np.uint8)
    return out


_LPM = {}


def lpm_model(routes):
    key = id(routes)
    if key not in _LPM:
        _LPM[key] = (routes, X.Model(routes, LPM_DEFAULT))
    return _LPM[key][1]


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


# ------------------------------------------------------------------ packets
def rfc1071(hdr):
    """The checksum of an IPv4 header whose field is zero: the complement of the end-around-carry sum of its words."""
    return ~L4.rfc1071_sum(bytes(hdr)) & 0xFFFF


def fix_csum(p, ip):
    q = bytearray(p)
    q[ip + 10:ip + 12] = b"\0\0"
    q[ip + 10:ip + 12] = rfc1071(q[ip:ip + 20]).to_bytes(2, "big")
    return bytes(q)


def v4(ttl=64, vlans=0, payload=b"fwd", l4="UDP", good=True, dst=None):
    """(bytes, hdrs) of Ether / Vlan* / IPv4 / l4 with the given ttl and an RFC 1071 checksum (good=False: off by 5)."""
    p = bytearray(L4.pkt(l4, vlans=vlans, payload=payload, dst=dst))
    hdrs = L4.hdrs_of(bytes(p))
    ip = X.ip_slots(hdrs)[0][1]
    p[ip + 8] = ttl
    p = bytearray(fix_csum(p, ip))
    if not good:
        p[ip + 11] = (p[ip + 11] + 5) & 0xFF
    return bytes(p), hdrs


def v6(hop=64, vlans=0, payload=b"", l4="UDP", dst=None):
    p = bytearray(L4.pkt(l4, v6=True, vlans=vlans, payload=payload, dst=dst))
    hdrs = L4.hdrs_of(bytes(p))
    p[X.ip_slots(hdrs)[0][1] + 7] = hop
    return bytes(p), hdrs


def cut_ip(item, short=1):
    p, hdrs = item
    t, o = X.ip_slots(hdrs)[0]
    return p[:o + (20 if t == T_IPV4 else 40) - short], hdrs


def without(item, ty):
    p, hdrs = item
    return p, [(t, o) for t, o in hdrs if t != ty]


def l3len(item, k=0):
    p, hdrs = item
    t, o = X.ip_slots(hdrs)[k]
    return int.from_bytes(p[o + 2:o + 4], "big") if t == T_IPV4 else 40 + int.from_bytes(p[o + 4:o + 6], "big")


def mac(k):
    return bytes([0x02, 0xAD, k >> 16 & 0xFF, k >> 8 & 0xFF, k & 0xFF, 0x5A ^ (k & 0xFF)])


def adjacency(k, port=None, mtu=0, action=FORWARD):
    return (mac(2 * k), mac(2 * k + 1), 100 + k if port is None else port, mtu, action)


def adj_array(adj):
    arr = np.zeros(len(adj), schema.FWD_ADJ_DTYPE)
    for i, (d, s, port, mtu, action) in enumerate(adj):
        arr["dmac"][i], arr["smac"][i] = np.frombuffer(d, np.uint8), np.frombuffer(s, np.uint8)
        arr["port"][i], arr["mtu"][i], arr["action"][i] = port, mtu, action
    return arr


# adjacencies of the named cases: 0 and 1 forward, 2 drops, 3 punts, 4 has an mtu no packet passes, 5 forwards (the
# fused cases' default)
ADJ = [adjacency(0), adjacency(1, mtu=1500), adjacency(2, action=ACT_DROP), adjacency(3, action=ACT_PUNT),
       adjacency(4, mtu=20), adjacency(5, port=7)]


def case(items, nexthop=None, adj=ADJ, which=0, keep_l2=False, select=None, routes=None):
    n = len(items)
    if nexthop is None and routes is None:
        nexthop = [0] * n
    return dict(items=list(items), adj=list(adj), which=which, keep_l2=keep_l2, routes=routes,
                nexthop=None if nexthop is None else np.asarray(nexthop, np.uint32),
                select=None if select is None else np.asarray(select, np.uint8))


def statuses(ver):
    """One packet per status, in status order."""
    mk = v4 if ver == 4 else v6
    arp = X.template("arp")
    items = [mk(), mk(), arp, cut_ip(mk()), without(mk(), T_ETHER), mk(1), mk(), mk(), mk(), mk()]
    return case(items, nexthop=[0, 0, 0, 0, 0, 0, len(ADJ), 2, 3, 4], select=[1, 0, 1, 1, 1, 1, 1, 1, 1, 1])


def named():
    """name -> (case, the statuses it must give in the "indexed" layout, or None)."""
    t = {}
    t["statuses_v4"] = (statuses(4), list(range(10)))
    t["statuses_v6"] = (statuses(6), list(range(10)))
    t["ttl_v4"] = (case([v4(0), v4(1), v4(2), v4(255)]), [TTL, TTL, OK, OK])
    t["ttl_v6"] = (case([v6(0), v6(1), v6(2), v6(255)]), [TTL, TTL, OK, OK])
    a, b = v4(payload=b"x" * 9), v6(payload=b"yz")
    adj = [adjacency(0, mtu=l3len(a)), adjacency(1, mtu=l3len(a) - 1), adjacency(2, mtu=l3len(b)),
           adjacency(3, mtu=l3len(b) - 1), adjacency(4, mtu=0)]
    t["mtu"] = (case([a, a, b, b, a, b], nexthop=[0, 1, 2, 3, 4, 4], adj=adj), [OK, MTU, OK, MTU, OK, OK])
    vx = X.template("vxlan")
    t["vxlan_outer"] = (case([vx, v4(), vx], nexthop=[1, 0, 0]), [OK, OK, OK])
    t["vxlan_inner"] = (case([vx, v4(), vx], nexthop=[1, 0, 0], which=LAST), [OK, OK, OK])
    t["double_vlan"] = (case([v4(vlans=2), v6(vlans=0), v4(vlans=2, good=False)], nexthop=[0, 1, 5]), [OK, OK, OK])
    # packets that start at their IP header (a parse with PKT_ENTRY_IPV4): no Ether entry
    bare = [(p[14:], [(t_, o - 14) for t_, o in h if t_ != T_ETHER]) for p, h in (v4(), v4(9, payload=b"bare"))]
    t["entry_ipv4"] = (case(bare, nexthop=[0, 1]), [NO_ETHER, NO_ETHER])
    t["entry_ipv4_keep_l2"] = (case(bare, nexthop=[0, 1], keep_l2=True), [OK, OK])
    t["cut_ip"] = (case([cut_ip(v4()), cut_ip(v6()), cut_ip(v4(), 20), v4()]), [SPAN, SPAN, SPAN, OK])
    # an IPv4 header at byte 0 and 6 bytes behind it; the columns say an Ether header starts at byte 14
    p = v4()[0][14:34] + b"\1\2\3\4\5\6"
    t["cut_ether_forged"] = (case([(p, [(T_ETHER, 14), (T_IPV4, 0)]), (p, [(T_ETHER, 12), (T_IPV4, 0)]),
                                   (p, [(T_ETHER, 65535), (T_IPV4, 0)]), (p, [(T_ETHER, 0), (T_IPV4, 65535)])]),
                             [SPAN, OK, SPAN, SPAN])
    t["no_adjacency"] = (case([v4(), v6(), v4()], nexthop=[len(ADJ), NONE, len(ADJ) - 1]), [NO_ADJ, NO_ADJ, OK])
    t["nadj_0"] = (case([v4(), v6(), v4(1), X.template("arp")], nexthop=[0, 0, 0, 0], adj=[]), [NO_ADJ, NO_ADJ, TTL, NO_IP])
    t["keep_l2"] = (case([v4(), v6(), without(v4(), T_ETHER)], nexthop=[0, 1, 5], keep_l2=True), [OK, OK, OK])
    return t


# ------------------------------------------------------------------ the seeded random mix
MIX_SEED = 20271
MIX_N = 4096


def mix_adj(nadj, seed=MIX_SEED):
    """nadj adjacencies: index % 8 == 5 drops, 6 punts, 7 has an mtu of 27 (below every packet's L3 length), the rest
    forward with no mtu or 1500."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(nadj):
        r = k % 8
        out.append((rng.bytes(6), rng.bytes(6), int(rng.integers(0, 4)) if k % 3 else int(rng.integers(0, 1 << 32)),
                    27 if r == 7 else (0, 1500)[k & 1], ACT_DROP if r == 5 else ACT_PUNT if r == 6 else FORWARD))
    return out


def mix(n=MIX_N, nadj=64, seed=MIX_SEED):
    """n packets of at most 64 bytes whose statuses the generator aims at: a target status per packet, OK three
    times as likely as each of the others."""
    rng = np.random.default_rng(seed)
    adj = mix_adj(nadj, seed)
    by = {r: [k for k in range(nadj) if k % 8 == r] for r in range(8)}
    fwd = [k for k in range(nadj) if k % 8 < 5]
    arp = X.template("arp")
    items, nexthop, select = [], [], []
    for i in range(n):
        target = int(rng.integers(0, 12))
        target = OK if target >= 10 else target
        is4 = rng.random() < 0.6
        ttl = int(rng.integers(2, 256))
        if is4:
            vl = int(rng.integers(0, 2))
            l4 = "UDP" if vl else ("UDP", "TCP")[int(rng.integers(0, 2))]
            room = 64 - (14 + 4 * vl + 20 + (8 if l4 == "UDP" else 20))
            it = v4(ttl, vlans=vl, payload=L4.rnd(rng, int(rng.integers(0, room + 1))), l4=l4, good=rng.random() < 0.8)
        else:
            it = v6(ttl, payload=L4.rnd(rng, int(rng.integers(0, 3))))
        a = fwd[int(rng.integers(0, len(fwd)))]
        s = 1
        if target == SKIPPED:
            s = 0
        elif target == NO_IP:
            it = arp if rng.random() < 0.5 else (it[0], [])
        elif target == SPAN:
            it = cut_ip(it, int(rng.integers(1, 21)))
        elif target == NO_ETHER:
            it = without(it, T_ETHER)
        elif target == TTL:
            it = (v4 if is4 else v6)(int(rng.integers(0, 2)))
        elif target == NO_ADJ:
            a = int(rng.choice([nadj, nadj + 1, 1 << 20, NONE]))
        elif target in (DROP, PUNT, MTU):
            r = {DROP: 5, PUNT: 6, MTU: 7}[target]
            a = by[r][int(rng.integers(0, len(by[r])))]
        assert len(it[0]) <= 64
        items.append(it)
        nexthop.append(a)
        select.append(s)
    return case(items, nexthop=nexthop, adj=adj, select=select)


def assert_mix(want, b, chain, label="mix"):
    """On the model's output alone: every status at least 8 times, both IP versions among the OK packets."""
    counts = np.bincount(want["status"], minlength=NSTATUS)
    assert (counts >= 8).all(), (label, counts)
    vers = set()
    for i in np.flatnonzero(want["status"] == OK):
        nh = int(chain["n_hdrs"][i])
        vers |= {int(chain["hdr_type"][j, i]) for j in range(nh)} & {T_IPV4, T_IPV6}
    assert vers == {T_IPV4, T_IPV6}, (label, vers)


# ------------------------------------------------------------------ fused route lookup
def fused(name, kind="probe"):
    """The probes of an lpm_cases table as packets, the table's next hops folded onto the adjacencies of ADJ + 2 more
    (so that every status from step 5 on comes up).  kind: "probe" (IPv4 and IPv6), "vxlan" (the inner IP routed)."""
    routes, probes, _, _ = X.cached(name)
    adj = ADJ + [adjacency(6), adjacency(7, mtu=50)]
    folded = _FOLDED.setdefault(name, [(v, p, a, nh % (len(adj) + 1)) for v, p, a, nh in routes])
    probes = probes[:400]
    if kind == "vxlan":
        v4p = [a for v, a in probes if v == 4]
        items = [X.vxlan_for(v4p[k], v4p[-1 - k]) for k in range(min(120, len(v4p)))]
        return case(items, adj=adj, which=LAST, routes=folded)
    items = []
    for k, pr in enumerate(probes):
        p, h = X.packet_for(pr)
        q = bytearray(p)
        o = X.ip_slots(h)[0][1]
        if pr[0] == 4:
            q[o + 8] = 2 + k % 200
            q = bytearray(fix_csum(q, o))
        items.append((bytes(q), h))
    return case(items, adj=adj, routes=folded)


_FOLDED = {}


# ------------------------------------------------------------------ layouts
LAYOUTS = ["s64", "s64_lens", "s128", "s128_lens", "indexed"]


def layout(c, name, seed=3):
    """(batch, chain) of the case's packets: "s64" / "s128" fixed-stride slots (a longer packet is cut at the slot),
    "_lens" with the packets' lengths, without them every packet is its whole slot; "indexed": back to back, packet i
    at alignment i % 16, the last one ending at the slab's last byte."""
    items = c["items"]
    n = len(items)
    chain = F.chain_from(n, [h for _, h in items])
    if name == "indexed":
        return C.indexed([p for p, _ in items], np.random.default_rng(seed), align=[i % 16 for i in range(n)]), chain
    stride = int(name[1:].split("_")[0])
    rng = np.random.default_rng(seed + stride)
    slab = rng.integers(0, 256, n * stride, dtype=np.uint8)
    lens = []
    for i, (p, _) in enumerate(items):
        p = p[:stride]
        slab[i * stride:i * stride + len(p)] = np.frombuffer(p, np.uint8)
        lens.append(len(p))
    return C.batch(slab, lens=lens if name.endswith("_lens") else None, stride=stride, n=n), chain


def head(c, n):
    """The case's first n packets."""
    cut = lambda a: None if a is None else a[:n]  # noqa: E731
    return dict(c, items=c["items"][:n], nexthop=cut(c["nexthop"]), select=cut(c["select"]))


_CACHE = {}


def cached(key, build):
    if key not in _CACHE:
        _CACHE[key] = build()
    return _CACHE[key]


def named_cached():
    return cached("named", named)


def mix_cached():
    return cached("mix", mix)


NAMED = ["statuses_v4", "statuses_v6", "ttl_v4", "ttl_v6", "mtu", "vxlan_outer", "vxlan_inner", "double_vlan",
         "entry_ipv4", "entry_ipv4_keep_l2", "cut_ip", "cut_ether_forged", "no_adjacency", "nadj_0", "keep_l2"]
