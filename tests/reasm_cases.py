"""The yardstick and the case builders of pkt_reasm_* (tests/test_reasm_host.py, test_reasm_device.py).

The yardstick is an independent pure-Python model written from the text of include/pktgpu.h (RFC 791's reassembly with
overlaps refused): a dict by key, a sort by offset, a walk.  It never calls pkt_reasm_host and shares no code with
pktgpu_reasm.hpp.  Given a batch, chain columns, the select mask and the flags it returns the expected status /
out_index / counters, the output packets byte for byte and their rows.  The model of fragmentation in frag_cases.py
(one()) makes the inputs of the round trips.

A case is a list of items (packet bytes, [(type, offset)]); frag_cases.layout() puts them into an indexed or a
fixed-stride batch.  cases() is the one list the host and the device tests both run.
"""
import numpy as np

from pktgpu import schema

import compare_cases as C
import frag_cases as G

(WHOLE, JOINED, PENDING, SKIPPED, NO_IP, SPAN, BAD_HDR, TRUNC, TOO_BIG) = range(9)
NSTATUS = 9
NONE = 0xFFFFFFFF
LAST = 0xFF
ONLY_JOINED, NO_WRITE = 1, 2
MAXH = schema.MAX_HDRS
T_ETHER, T_VLAN, T_IPV4, T_IPV6, T_UDP = G.T_ETHER, G.T_VLAN, G.T_IPV4, G.T_IPV6, G.T_UDP
r16, be16, layout = G.r16, G.be16, G.layout
_CACHE = {}


def cached(key, build):
    """(A cache of this module's own: frag_cases' keys are other tests'.)"""
    if key not in _CACHE:
        _CACHE[key] = build()
    return _CACHE[key]


# ------------------------------------------------------------------ the yardstick
def classify(p, hdrs, which, selected):
    """(status, member) of packet bytes `p` with the chain `hdrs` (cut to 16 entries): member = dict(key, s, ln, mf, ip,
    e) where the packet is a fragment that may join (status PENDING until the datagram's verdict), else None; for WHOLE
    member is None too."""
    if not selected:
        return SKIPPED, None
    ips = [j for j, (t, _) in enumerate(hdrs) if t in (T_IPV4, T_IPV6)]
    ips = ips[-1:] if which == LAST else ips[which:which + 1]
    if not ips:
        return NO_IP, None
    e = ips[0]
    t, ip = hdrs[e]
    if ip + (20 if t == T_IPV4 else 40) > len(p):
        return SPAN, None
    if t == T_IPV6 or be16(p, ip + 6) & 0x3FFF == 0:
        return WHOLE, None
    L, w = be16(p, ip + 2), be16(p, ip + 6)
    mf = bool(w & 0x2000)
    if p[ip] != 0x45 or L <= 20 or (mf and (L - 20) % 8):
        return BAD_HDR, None
    if ip + L > len(p):
        return TRUNC, None
    key = (bytes(p[ip + 12:ip + 16]), bytes(p[ip + 16:ip + 20]), p[ip + 9], bytes(p[ip + 4:ip + 6]))
    return PENDING, dict(key=key, s=8 * (w & 0x1FFF), ln=L - 20, mf=mf, ip=ip, e=e)


def verdict(ms):
    """A datagram's verdict from its members (sorted by s): the tiling of the header comment, walked."""
    if sum(1 for m in ms if not m["mf"]) != 1:
        return PENDING
    at = 0
    for m in ms:
        if m["s"] != at:
            return PENDING
        at = m["s"] + m["ln"]
    if ms[-1]["mf"]:
        return PENDING
    return TOO_BIG if 20 + at > 65535 else JOINED


def join(pk, ms):
    """The joined packet from the members (sorted by s; pk[i]: packet i's bytes)."""
    m0 = ms[0]
    p0, ip0 = pk[m0["i"]], m0["ip"]
    E = ms[-1]["s"] + ms[-1]["ln"]
    L, w, hc = be16(p0, ip0 + 2), be16(p0, ip0 + 6), be16(p0, ip0 + 10)
    L2, w2 = 20 + E, w & 0xC000
    hc2 = ~G.fold2((~hc & 0xFFFF) + (~L & 0xFFFF) + L2 + (~w & 0xFFFF) + w2) & 0xFFFF
    out = bytearray(p0[:ip0 + 20]) + bytearray(E)
    out[ip0 + 2:ip0 + 4], out[ip0 + 6:ip0 + 8], out[ip0 + 10:ip0 + 12] = L2.to_bytes(2, "big"), w2.to_bytes(2, "big"), hc2.to_bytes(2, "big")
    for m in ms:
        p = pk[m["i"]]
        out[ip0 + 20 + m["s"]:ip0 + 20 + m["s"] + m["ln"]] = p[m["ip"] + 20:m["ip"] + 20 + m["ln"]]
    return bytes(out)


def expect(b, chain, select=None, which=0, flags=0):
    """The model's whole result for batch `b`: status / out_index / hits, n_out, bytes_out, and per output: pkts
    (bytes), src_index, nfrag, rows ([(type, offset)])."""
    n = b["n"]
    out = dict(status=np.zeros(n, np.uint8), out_index=np.full(n, NONE, np.uint32), hits=np.zeros(NSTATUS, np.uint64),
               pkts=[], src_index=[], nfrag=[], rows=[])
    pk, hd, groups = [], [], {}
    for i, (off, ln) in enumerate(C.extents(b)):
        p = b["slab"][off:off + ln].tobytes()
        nh = min(int(chain["n_hdrs"][i]), MAXH)
        hdrs = [(int(chain["hdr_type"][j, i]), int(chain["hdr_off"][j, i])) for j in range(nh)]
        st, m = classify(p, hdrs, which, select is None or select[i] != 0)
        pk.append(p)
        hd.append(hdrs)
        out["status"][i] = st
        if m:
            m["i"] = i
            groups.setdefault(m["key"], []).append(m)
    owner = {}
    for ms in groups.values():
        ms.sort(key=lambda m: (m["s"], m["i"]))
        v = verdict(ms)
        for m in ms:
            out["status"][m["i"]] = v
        if v == JOINED:
            owner[max(m["i"] for m in ms)] = ms
    for i in range(n):
        st = out["status"][i]
        if st == WHOLE and not flags & ONLY_JOINED:
            out["out_index"][i] = len(out["pkts"])
            out["pkts"].append(pk[i])
            out["nfrag"].append(1)
            out["rows"].append(hd[i])
        elif i in owner:
            ms = owner[i]
            for m in ms:
                out["out_index"][m["i"]] = len(out["pkts"])
            out["pkts"].append(join(pk, ms))
            out["nfrag"].append(len(ms))
            out["rows"].append(hd[ms[0]["i"]][:ms[0]["e"] + 1])
        else:
            continue
        out["src_index"].append(i)
    for st in out["status"]:
        out["hits"][st] += 1
    out["n_out"] = len(out["pkts"])
    out["bytes_out"] = sum(r16(len(q)) for q in out["pkts"])
    return out


def check(got, want, cap, label=""):
    """got: numpy arrays by name (dst = the whole destination, [0, dst_len)) against the model: the per-source arrays,
    the totals, every output's bytes with its zero padding, the layout rule, the chain rows and the empty tail."""
    for name in ("status", "out_index", "hits"):
        if got.get(name) is not None:
            g = np.asarray(got[name])
            bad = np.flatnonzero(g != want[name])
            assert bad.size == 0, (label, name, bad[:8], g[bad[:8]], want[name][bad[:8]])
    assert (got["n_out"], got["bytes_out"]) == (want["n_out"], want["bytes_out"]), (label, "totals", got["n_out"], got["bytes_out"], want["n_out"], want["bytes_out"])
    if got.get("out_off") is None:
        return
    k = want["n_out"]
    pos = 0
    dst = got["dst"]
    for q, p in enumerate(want["pkts"]):
        assert int(got["out_off"][q]) == pos and int(got["out_len"][q]) == len(p), (label, "layout", q, int(got["out_off"][q]), pos, int(got["out_len"][q]), len(p))
        g = dst[pos:pos + r16(len(p))].tobytes()
        if g != p + bytes(r16(len(p)) - len(p)):
            w = p + bytes(r16(len(p)) - len(p))
            bad = [j for j in range(len(w)) if g[j] != w[j]]
            raise AssertionError((label, "bytes of output", q, want["src_index"][q], "first bad bytes", bad[:8], len(p)))
        pos += r16(len(p))
    assert pos == want["bytes_out"]
    for name, empty in (("src_index", NONE), ("nfrag", 0)):
        if got.get(name) is not None:
            assert np.array_equal(got[name][:k], np.asarray(want[name], got[name].dtype)), (label, name)
            assert (got[name][k:cap] == empty).all(), (label, name, "tail")
    assert (got["out_off"][k:cap] == 0).all() and (got["out_len"][k:cap] == 0).all(), (label, "tail")
    if got.get("oc_n_hdrs") is not None:
        assert np.array_equal(got["oc_n_hdrs"][:k], np.asarray([len(r) for r in want["rows"]], np.uint8)), (label, "n_hdrs")
        assert (got["oc_n_hdrs"][k:cap] == 0).all(), (label, "n_hdrs tail")
    for name, col in (("oc_hdr_type", 0), ("oc_hdr_off", 1)):
        if got.get(name) is not None:
            g = got[name].reshape(MAXH, cap)
            for q, r in enumerate(want["rows"]):
                assert [int(g[j, q]) for j in range(len(r))] == [x[col] for x in r], (label, name, q)


# ------------------------------------------------------------------ packets
SRC, DST = bytes([10, 1, 2, 3]), bytes([11, 4, 5, 6])


def ip4(L, w=0, ident=0x1234, proto=17, src=SRC, dst=DST, b0=0x45, bad_csum=0):
    h = bytearray(20)
    h[0] = b0
    h[2:4], h[4:6], h[6:8] = (L & 0xFFFF).to_bytes(2, "big"), ident.to_bytes(2, "big"), w.to_bytes(2, "big")
    h[8], h[9] = 64, proto
    h[12:16], h[16:20] = src, dst
    h[10:12] = ((~G.rfc1071(h) + bad_csum) & 0xFFFF).to_bytes(2, "big")
    return bytes(h)


def l2(vlan):
    return bytes(range(1, 13)) + (b"\x81\x00\x00\x0a\x08\x00" if vlan else b"\x08\x00")


def l2_rows(vlan):
    return [(T_ETHER, 0)] + ([(T_VLAN, 14)] if vlan else [])


def dgram(payload, ident, vlan=False, pad=0, bad_csum=0, **kw):
    """Ether / [Vlan] / IPv4 / payload (+ pad trailing bytes), unfragmented: (bytes, hdrs)."""
    pre = l2(vlan)
    p = pre + ip4(20 + len(payload), 0, ident, bad_csum=bad_csum, **kw) + payload + bytes([0xEE]) * pad
    hdrs = l2_rows(vlan) + [(T_IPV4, len(pre))] + ([(T_UDP, len(pre) + 20)] if len(payload) >= 8 else [])
    return p, hdrs


def udp_dgram(n, ident, seed=0):
    """A UDP datagram of n data bytes with a valid UDP checksum."""
    data = G.pattern(n, seed)
    u = bytearray((4000).to_bytes(2, "big") + (4001).to_bytes(2, "big") + (8 + n).to_bytes(2, "big") + b"\0\0" + data)
    ps = SRC + DST + bytes([0, 17]) + (8 + n).to_bytes(2, "big") + bytes(u) + (b"\0" if n % 2 else b"")
    c = ~G.rfc1071(ps) & 0xFFFF
    u[6:8] = (c or 0xFFFF).to_bytes(2, "big")
    return dgram(bytes(u), ident)


def mkfrag(payload, s, ln, mf, ident, vlan=False, pad=0, b0=0x45, L=None, hi=0, **kw):
    """The fragment [s, s + ln) of `payload` as a packet of its own, its chain cut at the IP entry: (bytes, hdrs)."""
    pre = l2(vlan)
    w = hi | (0x2000 if mf else 0) | s // 8
    p = pre + ip4(20 + ln if L is None else L, w, ident, b0=b0, **kw) + payload[s:s + ln] + bytes([0xEE]) * pad
    return p, l2_rows(vlan) + [(T_IPV4, len(pre))]


def frags(item, m, which=0):
    """The item cut at mtu m by frag_cases' model, each fragment with the rows pkt_frag_batch gives it."""
    p, hdrs = item
    st, e, outs = G.one(p, hdrs[:MAXH], m, which, True)
    return [(o, hdrs[:e + 1]) for o in outs] if st == G.SPLIT else [item]


def original(item, which=0):
    """What a joined datagram must equal when the header checksum was valid: the item's bytes [0, ip_off + L)."""
    p, hdrs = item
    ips = [o for t, o in hdrs if t == T_IPV4]
    ip = ips[-1] if which == LAST else ips[which]
    return p[:ip + be16(p, ip + 2)]


def arrange(groups, order, seed=5):
    """One list from lists of fragments: each list in order / reversed / shuffled, one after the other, or ("interleaved")
    dealt round-robin from all the lists."""
    rng = np.random.default_rng(seed)
    if order == "interleaved":
        out, k = [], 0
        while any(k < len(g) for g in groups):
            out += [g[k] for g in groups if k < len(g)]
            k += 1
        return out
    out = []
    for g in groups:
        g = list(g)
        if order == "reversed":
            g.reverse()
        elif order == "shuffled":
            g = [g[j] for j in rng.permutation(len(g))]
        out += g
    return out


MTUS = (28, 68, 576, 1280)
ORDERS = ("in_order", "reversed", "shuffled", "interleaved")


def round_trip(m, order):
    """-> (items, originals [(item, valid checksum)]): four datagrams cut at mtu m, one VLAN-tagged with trailing
    padding, one with a wrong header checksum, whole packets (IPv4, IPv6, a non-IP frame) before, between and after."""
    origs = [dgram(G.pattern(1391, 1), 0x0101), dgram(G.pattern(2000, 2), 0x0102, vlan=True, pad=5),
             dgram(G.pattern(1400, 3), 0x0103, bad_csum=0x1F3), dgram(G.pattern(1281 if m > 28 else 300, 4), 0x0104)]
    gs = [frags(o, m) for o in origs]
    assert all(len(g) >= 2 for g in gs)
    whole = [dgram(G.pattern(100, 9), 0x0777), G.v6(200, seed=3), (bytes(60), [(T_ETHER, 0)])]
    if order == "interleaved":
        items = [whole[0]] + arrange(gs[:2], order) + [whole[1]] + arrange(gs[2:], order) + [whole[2]]
    else:
        items = [whole[0]] + arrange(gs[:2], order) + [whole[1]] + arrange(gs[2:], order, seed=6) + [whole[2]]
    return items, [(o, k != 2) for k, o in enumerate(origs)]


# five fragments of a 100-byte payload: [0, 24) [24, 48) [48, 72) [72, 96) [96, 100)
def five(ident, **kw):
    pay = G.pattern(100, ident)
    return [mkfrag(pay, s, min(24, 100 - s), s + 24 < 100, ident, **kw) for s in range(0, 100, 24)]


def cases():
    """name -> dict(items, select=None, which=0, statuses (None: the model's are enough), n_out).  Every case is run by
    the host twin and by the device in both layouts."""
    t = {}
    pay = G.pattern(100, 7)
    f = five(0x0201)
    P5 = [PENDING] * 5

    def case(name, items, statuses=None, n_out=None, select=None, which=0):
        t[name] = dict(items=items, select=None if select is None else np.asarray(select, np.uint8), which=which,
                       statuses=statuses, n_out=n_out)

    case("complete", f, [JOINED] * 5, 1)
    case("first_missing", f[1:], [PENDING] * 4, 0)
    case("middle_missing", f[:2] + f[3:], [PENDING] * 4, 0)
    case("last_missing", f[:4], [PENDING] * 4, 0)
    case("duplicate", f[:2] + [f[1]] + f[2:], [PENDING] * 6, 0)
    case("partial_overlap", [f[0], mkfrag(pay, 16, 32, True, 0x0201)] + f[2:], P5, 0)
    case("overlap_that_keeps_the_sum", [f[0], mkfrag(pay, 24, 32, True, 0x0201), mkfrag(pay, 48, 16, True, 0x0201)] + f[3:], P5, 0)
    case("two_finals", f[:3] + [mkfrag(pay, 72, 24, False, 0x0201), f[4]], P5, 0)
    case("two_finals_at_the_end", f + [f[4]], [PENDING] * 6, 0)
    case("fragment_past_the_end", f + [mkfrag(G.pattern(300, 1), 200, 8, True, 0x0201)], [PENDING] * 6, 0)
    case("same_key_twice", f + f, [PENDING] * 10, 0)
    case("same_key_twice_interleaved", arrange([f, f], "interleaved"), [PENDING] * 10, 0)
    case("member_deselected", f, [PENDING, PENDING, SKIPPED, PENDING, PENDING], 0, select=[1, 1, 0, 1, 1])
    case("member_byte0_0x46", f[:2] + [mkfrag(pay, 48, 24, True, 0x0201, b0=0x46)] + f[3:], [PENDING, PENDING, BAD_HDR, PENDING, PENDING], 0)
    case("member_L_20", f[:2] + [mkfrag(pay, 48, 24, True, 0x0201, L=20)] + f[3:], [PENDING, PENDING, BAD_HDR, PENDING, PENDING], 0)
    case("member_mf_len_4_mod_8", f[:2] + [mkfrag(pay, 48, 20, True, 0x0201)] + f[3:], [PENDING, PENDING, BAD_HDR, PENDING, PENDING], 0)
    case("member_truncated", f[:2] + [(f[2][0][:-3], f[2][1])] + f[3:], [PENDING, PENDING, TRUNC, PENDING, PENDING], 0)
    case("order_of_the_tests", [mkfrag(pay, 48, 20, True, 1, b0=0x46, L=20), (mkfrag(pay, 48, 20, True, 1)[0][:40], f[0][1]),
                                (f[0][0][:30], f[0][1]), (f[0][0], [(T_ETHER, 0)]), (mkfrag(pay, 0, 100, False, 1, b0=0x47)[0][:50], f[0][1])],
         [BAD_HDR, BAD_HDR, SPAN, NO_IP, WHOLE], 1)
    # the key: the same identification under another source, destination or protocol is another datagram
    ks = [five(0x0301), five(0x0301, src=bytes([10, 1, 2, 4])), five(0x0301, dst=bytes([11, 4, 5, 7])), five(0x0301, proto=6)]
    case("keys_interleaved", arrange(ks, "interleaved"), [JOINED] * 20, 4)
    case("keys_shuffled", arrange([arrange(ks, "interleaved")], "shuffled"), [JOINED] * 20, 4)
    # DF and the reserved bit ride along on the first fragment; a single-fragment "datagram" (offset 0, MF clear) is WHOLE
    case("flag_bits", [mkfrag(pay, 0, 48, True, 0x0401, hi=0x8000), mkfrag(pay, 48, 52, False, 0x0401, hi=0x4000)], [JOINED] * 2, 1)
    case("final_first", [f[4], f[3], f[0], f[2], f[1]], [JOINED] * 5, 1)
    # 20 + E = 65556: 44 fragments of 1480, one of 392, the final one at offset 8189 with 24 bytes
    big = G.pattern(65536, 9)
    cuts = [(s, 1480) for s in range(0, 65120, 1480)] + [(65120, 392), (65512, 24)]
    assert cuts[-1][0] // 8 == 8189
    case("too_big", [mkfrag(big, s, ln, s != 65512, 0x0501) for s, ln in cuts], [TOO_BIG] * 46, 0)
    case("largest_datagram", [mkfrag(big, s, ln, s != 65120, 0x0502) for s, ln in cuts[:-2] + [(65120, 395)]], [JOINED] * 45, 1)
    # members with different prefixes: the output takes the s = 0 member's
    case("vlan_on_a_middle_member", f[:2] + [mkfrag(pay, 48, 24, True, 0x0201, vlan=True, pad=3)] + f[3:], [JOINED] * 5, 1)
    case("vlan_on_the_first_member", [mkfrag(pay, 0, 24, True, 0x0201, vlan=True)] + f[1:], [JOINED] * 5, 1)
    # inner headers: the fragments of a tunnelled packet's inner IPv4, by which_ip 1 and PKT_FLOW_LAST; the outer header is whole
    vx = G.vxlan(1000, seed=4)
    vf = frags(vx, 576, which=1) + [dgram(G.pattern(64, 1), 0x0601)]
    case("vxlan_inner_which_1", vf, [JOINED, JOINED, NO_IP], 1, which=1)
    case("vxlan_inner_last", vf, [JOINED, JOINED, WHOLE], 2, which=LAST)
    case("vxlan_outer", vf, [WHOLE] * 3, 3, which=0)
    # the place of an output: its last-arriving member's
    W = [dgram(G.pattern(40 + k, k), 0x0700 + k) for k in range(3)]
    A = [mkfrag(pay, 0, 40, True, 0x0711), mkfrag(pay, 40, 40, True, 0x0711), mkfrag(pay, 80, 20, False, 0x0711)]
    B = [mkfrag(pay, 0, 64, True, 0x0712), mkfrag(pay, 64, 36, False, 0x0712)]
    case("ordering", [W[0], A[0], B[0], W[1], A[1], B[1], W[2], A[2]], [WHOLE, JOINED, JOINED, WHOLE, JOINED, JOINED, WHOLE, JOINED], 5)
    case("ordering_final_first", [A[2], W[0], B[1], A[0], B[0], A[1]], [JOINED, WHOLE, JOINED, JOINED, JOINED, JOINED], 3)
    for m in MTUS:
        for order in ORDERS:
            items, origs = round_trip(m, order)
            t[f"round_trip_{m}_{order}"] = dict(items=items, select=None, which=0, statuses=None, n_out=len(origs) + 2, originals=origs)
    return t


ORDERING = dict(src_index=[0, 3, 5, 6, 7], nfrag=[1, 1, 2, 1, 3], out_index=[0, 4, 2, 1, 4, 2, 3, 4])
CASES = sorted(cases())


def get_case(name):
    return cached("reasm_cases", cases)[name]


def check_case(name, c, got, want):
    """What a case asks beyond the model: the statuses written down, the number of outputs, the originals back."""
    if c["statuses"] is not None:
        assert want["status"].tolist() == c["statuses"], (name, "the model", want["status"].tolist())
    assert want["n_out"] == c["n_out"], (name, want["n_out"])
    if c["n_out"] == 0:
        assert got["n_out"] == 0 and got["bytes_out"] == 0 and (np.asarray(got["out_index"]) == NONE).all()
    if name == "ordering":
        for k, v in ORDERING.items():
            assert np.asarray(got[k])[:len(v)].tolist() == v, (name, k)
    if "originals" in c:
        outs = [got["dst"][int(o):int(o) + int(ln)].tobytes() for o, ln in zip(got["out_off"][:got["n_out"]], got["out_len"])]
        joined = [p for p, k in zip(outs, got["nfrag"]) if k > 1]
        assert len(joined) == len(c["originals"])
        for item, valid in c["originals"]:
            want_p = original(item)
            if valid:
                assert want_p in joined, (name, "an original did not come back")
            else:  # off by the same amount: everything but the checksum field is the original's
                ip = [o for ty, o in item[1] if ty == T_IPV4][0]
                assert any(len(p) == len(want_p) and p[:ip + 10] == want_p[:ip + 10] and p[ip + 12:] == want_p[ip + 12:]
                           for p in joined), (name, "the original with the wrong checksum")


def mix(n, seed=17):
    """n source packets: datagrams of 9..3000 payload bytes cut at an mtu from MTUS, their fragments shuffled inside
    windows of 40 packets, whole IPv4 / IPv6 / non-IP packets and VLAN-tagged members among them; every fifth datagram
    is broken (a fragment dropped, doubled, or its header spoilt) -> (items, select)."""
    rng = np.random.default_rng(seed)
    items, ident = [], 0x1000
    while len(items) < n:
        win = []
        while len(win) < 40:
            r = int(rng.integers(0, 12))
            ident += 1
            if r == 0:
                win.append(G.v6(int(rng.integers(10, 900)), seed=ident))
            elif r == 1:
                win.append((bytes(rng.integers(0, 256, 60, dtype=np.uint8)), [(T_ETHER, 0)]))
            elif r in (2, 3):
                win.append(dgram(G.pattern(int(rng.integers(1, 1400)), ident), ident, vlan=r == 3, pad=int(rng.integers(0, 4))))
            else:
                pay = G.pattern(int(rng.integers(9, 3001)), ident)
                m = int(MTUS[int(rng.integers(0 if len(pay) < 200 else 1 if len(pay) < 700 else 2, 4))])
                g = frags(dgram(pay, ident, vlan=r == 4, pad=int(rng.integers(0, 3)), bad_csum=7 if r == 5 else 0), m)
                if ident % 5 == 0 and len(g) > 1:
                    k = int(rng.integers(0, len(g)))
                    how = int(rng.integers(0, 3))
                    if how == 0:
                        del g[k]
                    elif how == 1:
                        g.insert(k, g[k])
                    else:
                        q = bytearray(g[k][0])
                        q[g[k][1][-1][1]] = 0x46
                        g[k] = (bytes(q), g[k][1])
                win += g
        items += [win[j] for j in rng.permutation(len(win))]
    items = items[:n]
    select = (np.arange(n) % 101 != 5).astype(np.uint8)
    return items, select


# ------------------------------------------------------------------ the host twin, called through the C ABI
def host_call(b, chain, select=None, which=0, flags=0, cap=None, dst_len=None, skip=(), guard=64, over=None):
    """pkt_reasm_host with caller-sized outputs -> (rc, got).  cap / dst_len default to what the model-free sizing pass
    says.  skip: names of outputs passed as NULL.  Every output array has `guard` extra elements filled with 0xA5.. that
    must come back unchanged (got["guards"])."""
    import ctypes

    import pktgpu
    from pktgpu import _lib
    L = _lib.load()
    pb, keep = pktgpu._host_batch(_lib, b)
    cols = [np.ascontiguousarray(chain[k]) for k in ("n_hdrs", "hdr_type", "hdr_off")]
    ch = _lib.PktChain(*[c.ctypes.data for c in cols])
    n = b["n"]
    sel = None if select is None else np.ascontiguousarray(select, np.uint8)
    sp = sel.ctypes.data if sel is not None and sel.size else None
    tot, cnt = ctypes.c_uint64(0), ctypes.c_uint64(0)
    if cap is None or dst_len is None:
        rc = L.pkt_reasm_host(ctypes.byref(pb), ctypes.byref(ch), which, flags | NO_WRITE, sp, None, None, None, 0, 0,
                              None, None, None, None, None, None, ctypes.byref(tot), ctypes.byref(cnt))
        assert rc == 0
        cap = max(1, cnt.value) if cap is None else cap
        dst_len = tot.value if dst_len is None else dst_len
    shapes = dict(status=(n, np.uint8), out_index=(n, np.uint32), dst=(r16(dst_len) + 16, np.uint8),
                  out_off=(cap, np.uint64), out_len=(cap, np.uint32), src_index=(cap, np.uint32), nfrag=(cap, np.uint32),
                  oc_n_hdrs=(cap, np.uint8), oc_hdr_type=(MAXH * cap, np.uint8), oc_hdr_off=(MAXH * cap, np.uint16),
                  hits=(NSTATUS, np.uint64))
    if flags & NO_WRITE:
        skip = set(skip) | {"dst", "out_off", "out_len", "src_index", "nfrag", "oc_n_hdrs", "oc_hdr_type", "oc_hdr_off"}
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
    args = [ctypes.byref(pb), ctypes.byref(ch), which, flags, sp, p("status"), p("out_index"), p("dst"), dst_len, cap,
            p("out_off"), p("out_len"), p("src_index"), p("nfrag"), ctypes.byref(oc), p("hits"), ctypes.byref(tot),
            ctypes.byref(cnt)]
    for k, v in dict(over or {}).items():
        args[k] = v
    rc = L.pkt_reasm_host(*args)
    got = {k: a[:shapes[k][0]] for k, a in bufs.items()}
    got["guards"] = all((a[shapes[k][0]:].view(np.uint8) == 0xA5).all() for k, a in bufs.items())
    if "dst" in bufs:
        got["dst_rest"] = bufs["dst"]
    got["n_out"], got["bytes_out"], got["cap"] = cnt.value, tot.value, cap
    return rc, got
