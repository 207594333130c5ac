"""The yardstick and the case builders of pkt_icmp_err_* (tests/test_icmp_err_host.py, test_icmp_err_device.py).

The yardstick is an independent pure-Python model written from the rules of include/pktgpu.h (RFC 792 / 1191 / 4443's
layouts): it never calls pkt_icmp_err_host, and its checksum is l4_cases' RFC 1071 loop.  Given a batch, chain columns,
the codes, the map, the mtu(s), the cfg and the select mask it returns the expected status / out_index / counters,
the output packets byte for byte and their chain rows.

A case is a list of items (packet bytes, [(type, offset)]); frag_cases.layout() puts them into an indexed or a
fixed-stride batch.
"""
import socket
import struct

import numpy as np

from pktgpu import schema

import compare_cases as C
import frag_cases as G
from l4_cases import rfc1071_sum

(SENT, SKIPPED, BAD_REASON, NO_IP, SPAN, NO_ETHER, NO_SRC, BAD_HDR, FRAGMENT, BAD_SRC, MCAST, ICMP_ERR) = range(12)
NSTATUS = 12
NONE = 0xFFFFFFFF
LAST = 0xFF
NO_WRITE = 1
(R_NONE, R_TIME_EXCEEDED, R_TOO_BIG, R_NET_UNREACH, R_HOST_UNREACH, R_PROHIBITED, R_PORT_UNREACH) = range(7)
# the header's table, written out again: reason -> ((type, code) IPv4, (type, code) IPv6)
TYPE_CODE = {1: ((11, 0), (3, 0)), 2: ((3, 4), (2, 0)), 3: ((3, 0), (1, 0)), 4: ((3, 1), (1, 3)), 5: ((3, 13), (1, 1)),
             6: ((3, 3), (1, 4))}
T_ETHER, T_VLAN, T_IPV4, T_IPV6, T_ICMP, T_UDP, T_VXLAN = (schema.HDR_ID[k] for k in
                                                           ("Ether", "Vlan", "IPv4", "IPv6", "ICMP", "UDP", "Vxlan"))
MAXH = schema.MAX_HDRS
r16 = G.r16
be16 = G.be16
layout = G.layout
cached = G.cached

SRC4, SRC6 = "192.0.2.1", "2001:db8::1"


def cfg(src4=SRC4, src6=SRC6, max4=0, max6=0, ident=0, ttl=0, tos=0):
    """The cfg as the model reads it (addresses as wire bytes, None = all zero) and as pkt_icmp_cfg_t takes it."""
    a4 = socket.inet_pton(socket.AF_INET, src4) if isinstance(src4, str) else bytes(src4 or 4)
    a6 = socket.inet_pton(socket.AF_INET6, src6) if isinstance(src6, str) else bytes(src6 or 16)
    return dict(src4=a4, src6=a6, max4=max4, max6=max6, ident=ident, ttl=ttl, tos=tos)


# ------------------------------------------------------------------ the yardstick
def decide(p, hdrs, r, which, selected, cf):
    """(status, geo) of packet bytes `p` with the chain `hdrs` (already cut to 16 entries) and reason r; for SENT
    geo = (e_eth, eth_off, e_ip, ip_off, v4, Q)."""
    if not selected or r == 0:
        return SKIPPED, None
    if r > 6:
        return BAD_REASON, None
    ips = [j for j, (t, _) in enumerate(hdrs) if t in (T_IPV4, T_IPV6)]
    ips = ips[-1:] if which == LAST else ips[which:which + 1]
    if not ips:
        return NO_IP, None
    e = ips[0]
    t, ip = hdrs[e]
    v4 = t == T_IPV4
    H = 20 if v4 else 40
    if ip + H > len(p):
        return SPAN, None
    eths = [j for j in range(e) if hdrs[j][0] == T_ETHER]
    if not eths:
        return NO_ETHER, None
    ee = eths[-1]
    eth = hdrs[ee][1]
    if eth + 14 > ip:
        return SPAN, None
    if not any(cf["src4"] if v4 else cf["src6"]):
        return NO_SRC, None
    if v4:
        L = be16(p, ip + 2)
        if p[ip] != 0x45 or L < 20:
            return BAD_HDR, None
        if be16(p, ip + 6) & 0x1FFF:
            return FRAGMENT, None
        sa, da0 = p[ip + 12:ip + 16], p[ip + 16]
        if sa[0] in (0, 127) or sa[0] >= 224:
            return BAD_SRC, None
        mc = da0 >= 224
    else:
        if p[ip] >> 4 != 6:
            return BAD_HDR, None
        L = 40 + be16(p, ip + 4)
        sa, da0 = p[ip + 8:ip + 24], p[ip + 24]
        if not any(sa) or sa[0] == 0xFF:
            return BAD_SRC, None
        mc = da0 == 0xFF
    if (mc or p[eth] & 1) and not (not v4 and r == R_TOO_BIG):
        return MCAST, None
    end = min(len(p), ip + L)
    if v4 and p[ip + 9] == 1 and (ip + 20 >= end or p[ip + 20] in (3, 4, 5, 11, 12)):
        return ICMP_ERR, None
    if not v4 and p[ip + 6] == 58 and (ip + 40 >= end or p[ip + 40] < 128 or p[ip + 40] == 137):
        return ICMP_ERR, None
    mx = (cf["max4"] or 576) if v4 else (cf["max6"] or 1280)
    return SENT, (ee, eth, e, ip, v4, min(end - ip, mx - H - 8))


def build(p, geo, r, m, q, cf):
    """Output q for a SENT packet: the swapped L2 prefix, the new IP header, the ICMP header, the quote."""
    _, eth, _, ip, v4, Q = geo
    l2 = bytearray(p[eth:ip])
    l2[0:6], l2[6:12] = p[eth + 6:eth + 12], p[eth:eth + 6]
    quote = bytes(p[ip:ip + Q])
    ttl = cf["ttl"] or 64
    ty, co = TYPE_CODE[r][0 if v4 else 1]
    if v4:
        rest = struct.pack(">HH", 0, m) if r == R_TOO_BIG else bytes(4)
        msg = bytearray(struct.pack(">BBH", ty, co, 0) + rest + quote)
        msg[2:4] = struct.pack(">H", ~rfc1071_sum(msg) & 0xFFFF)
        hd = bytearray(struct.pack(">BBHHHBBH4s4s", 0x45, cf["tos"], 28 + Q, (cf["ident"] + q) & 0xFFFF, 0, ttl, 1, 0,
                                   cf["src4"], bytes(p[ip + 12:ip + 16])))
        hd[10:12] = struct.pack(">H", ~rfc1071_sum(hd) & 0xFFFF)
    else:
        rest = struct.pack(">I", m) if r == R_TOO_BIG else bytes(4)
        msg = bytearray(struct.pack(">BBH", ty, co, 0) + rest + quote)
        dst = bytes(p[ip + 8:ip + 24])
        pseudo = cf["src6"] + dst + struct.pack(">IHBB", len(msg), 0, 0, 58)
        c = ~rfc1071_sum(pseudo + bytes(msg)) & 0xFFFF
        msg[2:4] = struct.pack(">H", c or 0xFFFF)
        hd = struct.pack(">IHBB", 6 << 28 | cf["tos"] << 20, len(msg), 58, ttl) + cf["src6"] + dst
    return bytes(l2) + bytes(hd) + bytes(msg)


def rows_of(hdrs, geo):
    ee, eth, e, ip, v4, _ = geo
    rows = [(t, o - eth) for t, o in hdrs[ee:e + 1]] + [(T_ICMP, ip - eth + (20 if v4 else 40))]
    return rows[:MAXH]


def expect(b, chain, code, cf, mtu=0, cmap=None, select=None, which=0):
    """The model's whole result for batch `b`: status / out_index / hits, n_out, bytes_out, and per output: pkts
    (bytes), src_index, rows ([(type, offset)])."""
    n = b["n"]
    out = dict(status=np.zeros(n, np.uint8), out_index=np.full(n, NONE, np.uint32), hits=np.zeros(NSTATUS, np.uint64),
               pkts=[], src_index=[], rows=[])
    for i, (off, ln) in enumerate(C.extents(b)):
        p = b["slab"][off:off + ln].tobytes()
        nh = min(int(chain["n_hdrs"][i]), MAXH)
        hdrs = [(int(chain["hdr_type"][j, i]), int(chain["hdr_off"][j, i])) for j in range(nh)]
        c = int(code) if np.isscalar(code) else int(code[i])
        r = c if cmap is None else int(cmap[c])
        m = int(mtu) if np.isscalar(mtu) else int(mtu[i])
        st, geo = decide(p, hdrs, r, which, select is None or select[i] != 0, cf)
        out["status"][i] = st
        out["hits"][st] += 1
        if st == SENT:
            q = len(out["pkts"])
            out["out_index"][i] = q
            out["pkts"].append(build(p, geo, r, m, q, cf))
            out["src_index"].append(i)
            out["rows"].append(rows_of(hdrs, geo))
    out["n_out"] = len(out["pkts"])
    out["bytes_out"] = sum(r16(len(q)) for q in out["pkts"])
    return out


def check(got, want, cap, label=""):
    """got: numpy arrays by name (dst = the whole destination) against the model: the per-source arrays, the totals,
    every output's bytes with its zero padding, the layout rule, the chain rows and the empty tail."""
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
            at = next(j for j in range(len(w)) if g[j] != w[j])
            raise AssertionError((label, "bytes of output", q, "source", want["src_index"][q], "first bad byte", at, g[at], w[at], len(p)))
        pos += r16(len(p))
    assert pos == want["bytes_out"]
    if got.get("src_index") is not None:
        assert np.array_equal(got["src_index"][:k], np.asarray(want["src_index"], np.uint32)), (label, "src_index")
        assert (got["src_index"][k:cap] == NONE).all(), (label, "src_index tail")
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
MAC_D, MAC_S = bytes([0x02, 0x11, 0x22, 0x33, 0x44, 0x55]), bytes([0x02, 0xAA, 0xBB, 0xCC, 0xDD, 0xEE])
A4S, A4D = bytes([10, 1, 2, 3]), bytes([198, 51, 100, 7])
A6S = socket.inet_pton(socket.AF_INET6, "2001:db8:1::5")
A6D = socket.inet_pton(socket.AF_INET6, "2001:db8:2::9")


def pkt(payload=b"", v6=False, vlans=0, proto=17, src=None, dst=None, dmac=MAC_D, w=0, b0=None, L=None, pad=0, ttl=64,
        trunc=0):
    """Ether / vlans x Vlan / IPv4 or IPv6 / payload (+ pad trailing bytes, or the last `trunc` bytes cut off):
    (bytes, hdrs as a parse lists them up to the L4 header).  L: the IP length field's value when it is to lie."""
    et = b"\x86\xdd" if v6 else b"\x08\x00"
    l2 = dmac + MAC_S + b"".join(b"\x81\x00" + struct.pack(">H", 100 + k) for k in range(vlans)) + et
    hdrs = [(T_ETHER, 0)] + [(T_VLAN, 14 + 4 * k) for k in range(vlans)]
    ip = len(l2)
    if v6:
        hd = struct.pack(">BBHHBB", 0x60 if b0 is None else b0, 0, 0, len(payload) if L is None else L, proto, ttl) + \
            (A6S if src is None else src) + (A6D if dst is None else dst)
        hdrs.append((T_IPV6, ip))
    else:
        hd = bytearray(struct.pack(">BBHHHBBH4s4s", 0x45 if b0 is None else b0, 0, 20 + len(payload) if L is None else L,
                                   0x1234, w, ttl, proto, 0, A4S if src is None else src, A4D if dst is None else dst))
        hd[10:12] = struct.pack(">H", ~rfc1071_sum(hd) & 0xFFFF)
        hdrs.append((T_IPV4, ip))
    H = len(hd)
    if proto == 17 and len(payload) >= 8:
        hdrs.append((T_UDP, ip + H))
    if proto == (58 if v6 else 1) and len(payload) >= 4:
        hdrs.append((T_ICMP, ip + H))
    p = l2 + bytes(hd) + bytes(payload) + bytes([0xEE]) * pad
    return p[:len(p) - trunc], hdrs


def udp(k, seed=0):
    """A UDP header and payload of k bytes in all (k >= 8), patterned."""
    return struct.pack(">HHHH", 4000 + seed % 1000, 53, k, 0) + G.pattern(k - 8, seed)


def icmp(ty, k=16, seed=0):
    return struct.pack(">BBHI", ty, 0, 0, seed) + G.pattern(k - 8, seed)


def vxlan(inner):
    """Ether / IPv4 / UDP / Vxlan / inner: the inner Ether header at 50."""
    p, hdrs = inner
    outer_l = 20 + 8 + 8 + len(p)
    u = struct.pack(">HHHH", 4789, 4789, outer_l - 20, 0)
    o, oh = pkt(u + b"\x08\0\0\0\0\0\x07\0" + p)
    return o, oh[:2] + [(T_UDP, 34), (T_VXLAN, 42)] + [(t, off + 50) for t, off in hdrs]


# codes of the mix: pkt_fwd_batch's statuses, read through MAP (ICMP_MAP_FWD plus one forged row, code 200 -> reason 9)
F = schema
MAP = np.array(schema.ICMP_MAP_FWD, np.uint8)
MAP[200] = 9


def mix(n, seed=5):
    """n packets of 60..1600 bytes and a few of 9000, IPv4 and IPv6, 0 / 1 / 2 VLAN tags and VXLAN, with per-packet
    pkt_fwd_batch codes (TTL, MTU, NO_ADJ, and OK / DROP that ask for nothing) and per-packet mtus, among them the
    packets that decide every status -> (items, code uint8 [n], mtu uint16 [n], select)."""
    rng = np.random.default_rng(seed)
    items, code, mtu = [], [], []
    for i in range(n):
        k = i % 41
        ln = int(rng.integers(60, 1601))
        v6 = int(rng.integers(0, 3)) == 0
        vl = int(rng.integers(0, 3))
        pay = udp(max(8, ln - 14 - 4 * vl - (40 if v6 else 20)), seed=i)
        c = (F.FWD_TTL, F.FWD_MTU, F.FWD_NO_ADJ, F.FWD_TTL, F.FWD_MTU, F.FWD_OK, F.FWD_DROP)[int(rng.integers(0, 7))]
        it = pkt(pay, v6=v6, vlans=vl, pad=int(rng.integers(0, 4)) if k == 30 else 0)
        if i % 211 == 100:
            it = pkt(udp(9000 - 34 - (20 if v6 else 0), seed=i), v6=v6)
        elif k == 1:
            it = (bytes(rng.integers(0, 256, 64, dtype=np.uint8)), [(T_ETHER, 0)])           # NO_IP
        elif k == 2:
            it = (it[0][14 + 4 * vl:], [(t, o - 14 - 4 * vl) for t, o in it[1][1 + vl:]])    # NO_ETHER: parsed from IP on
        elif k == 3:
            it = pkt(pay, v6=v6, vlans=vl, b0=0x50 if v6 else 0x46)                          # BAD_HDR
        elif k == 4:
            it = pkt(pay, vlans=vl, w=0x2000 | 37)                                           # FRAGMENT
        elif k == 5:
            it = pkt(pay, vlans=vl, w=0x2000)                                                # a first fragment: answered
        elif k == 6:
            it = pkt(pay, v6=v6, vlans=vl, src=bytes(16) if v6 else bytes([127, 0, 0, 1]))   # BAD_SRC
        elif k == 7:
            it = pkt(pay, v6=v6, vlans=vl, dmac=b"\x01\x00\x5e\x00\x00\x01")                 # MCAST (IPv6 + MTU: answered)
        elif k == 8:
            it = pkt(pay, v6=v6, vlans=vl, dst=bytes([0xFF, 2] + [0] * 13 + [1]) if v6 else bytes([224, 0, 0, 5]))
        elif k == 9:
            it = pkt(icmp(1 if v6 else 11, 40, i), v6=v6, vlans=vl, proto=58 if v6 else 1)   # ICMP_ERR
        elif k == 10:
            it = pkt(icmp(128 if v6 else 8, 40, i), v6=v6, vlans=vl, proto=58 if v6 else 1)  # an echo request: answered
        elif k in (11, 12):
            it = vxlan(pkt(udp(max(8, ln - 100), seed=i), v6=k == 12))
        elif k == 13:
            it = pkt(pay, v6=v6, vlans=vl, trunc=int(rng.integers(1, 20)))                   # a truncated capture record
        elif k == 14:
            it = pkt(udp(int(rng.integers(8, 60)), seed=i), v6=v6, vlans=vl, pad=int(rng.integers(0, 30)))  # short: not clipped
        items.append(it)
        code.append(c)
        mtu.append(int((576, 1280, 1500, 9000)[int(rng.integers(0, 4))]))
    code[7] = 200                                   # BAD_REASON, by the forged map row
    p, hdrs = pkt(udp(100, 1))
    items[8] = (p, [(T_ETHER, 0), (T_IPV4, len(p) - 10)])  # SPAN, by a forged row: the IP entry runs past the packet
    code[8] = F.FWD_TTL
    select = (np.arange(n) % 17 != 5).astype(np.uint8)
    return items, np.asarray(code, np.uint8), np.asarray(mtu, np.uint16), select


def mix_conditions(want, want_nosrc):
    """What the mix must meet, asserted on the CPU before any device call: at least 3 packets of every status but
    BAD_REASON and SPAN (1 each, from forged rows; NO_SRC from the second cfg, which has no IPv6 source), and quotes
    both clipped and not clipped for both IP versions."""
    counts = np.bincount(want["status"], minlength=NSTATUS)
    for s in range(NSTATUS):
        need = 1 if s in (BAD_REASON, SPAN) else 0 if s == NO_SRC else 3
        assert counts[s] >= need, (schema.ICMPE_STATUS[s], counts)
    assert np.bincount(want_nosrc["status"], minlength=NSTATUS)[NO_SRC] >= 3
    # the built datagrams' lengths: an output's IP entry is its row before the ICMP row
    lens4 = {len(p) - r[-2][1] for p, r in zip(want["pkts"], want["rows"]) if r[-2][0] == T_IPV4}
    lens6 = {len(p) - r[-2][1] for p, r in zip(want["pkts"], want["rows"]) if r[-2][0] == T_IPV6}
    assert 576 in lens4 and min(lens4) < 576, sorted(lens4)[:4]
    assert 1280 in lens6 and min(lens6) < 1280, sorted(lens6)[:4]


# ------------------------------------------------------------------ the host twin, called through the C ABI
def lib_cfg(cf):
    from pktgpu import _lib
    c = _lib.PktIcmpCfg()
    c.src4[:] = cf["src4"]
    c.src6[:] = cf["src6"]
    c.max4, c.max6, c.ident, c.ttl, c.tos = cf["max4"], cf["max6"], cf["ident"], cf["ttl"], cf["tos"]
    return c


SHAPES = dict(status=np.uint8, out_index=np.uint32, out_off=np.uint64, out_len=np.uint32, src_index=np.uint32,
              oc_n_hdrs=np.uint8, oc_hdr_type=np.uint8, oc_hdr_off=np.uint16, hits=np.uint64)
PER_OUTPUT = {"dst", "out_off", "out_len", "src_index", "oc_n_hdrs", "oc_hdr_type", "oc_hdr_off"}
# positions in pkt_icmp_err_host's argument list (for `over`)
A_BATCH, A_CHAIN, A_WHICH, A_FLAGS, A_CFG, A_CODE, A_CODE_ALL, A_MAP, A_MTU, A_MTU_ALL = range(10)
A_DST, A_DST_LEN, A_CAP, A_OUT_OFF, A_OUT_LEN = 13, 14, 15, 16, 17
A_HITS = 20


def host_call(b, chain, code, cf, mtu=0, cmap=None, select=None, which=0, flags=0, cap=None, dst_len=None, skip=(),
              guard=64, over=None):
    """pkt_icmp_err_host with caller-sized outputs -> (rc, got).  cap / dst_len default to what the model-free sizing
    pass says.  skip: names of outputs passed as NULL.  Every output array has `guard` extra elements filled with 0xA5
    that must come back unchanged (got["guards"])."""
    import ctypes

    import pktgpu
    from pktgpu import _lib
    L = _lib.load()
    pb, keep = pktgpu._host_batch(_lib, b)
    cols = [np.ascontiguousarray(chain[k]) for k in ("n_hdrs", "hdr_type", "hdr_off")]
    ch = _lib.PktChain(*[c.ctypes.data for c in cols])
    n = b["n"]
    cd = None if np.isscalar(code) else np.ascontiguousarray(code, np.uint8)
    mt = None if np.isscalar(mtu) else np.ascontiguousarray(mtu, np.uint16)
    mp = None if cmap is None else np.ascontiguousarray(cmap, np.uint8)
    sel = None if select is None else np.ascontiguousarray(select, np.uint8)
    cc = lib_cfg(cf)
    ad = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    tot, cnt = ctypes.c_uint64(0), ctypes.c_uint64(0)
    head = [ctypes.byref(pb), ctypes.byref(ch), which, flags, ctypes.byref(cc), ad(cd), 0 if cd is not None else int(code),
            ad(mp), ad(mt), 0 if mt is not None else int(mtu), ad(sel)]
    if cap is None or dst_len is None:
        sizing = list(head)
        sizing[A_FLAGS] = flags | NO_WRITE
        rc = L.pkt_icmp_err_host(*sizing, None, None, None, 0, 0, None, None, None, None, None, ctypes.byref(tot),
                                 ctypes.byref(cnt))
        assert rc == 0
        cap = max(1, cnt.value) if cap is None else cap
        dst_len = tot.value if dst_len is None else dst_len
    counts = dict(status=n, out_index=n, out_off=cap, out_len=cap, src_index=cap, oc_n_hdrs=cap, oc_hdr_type=MAXH * cap,
                  oc_hdr_off=MAXH * cap, hits=NSTATUS)
    shapes = {k: (counts[k], dt) for k, dt in SHAPES.items()}
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
    args = head + [p("status"), p("out_index"), p("dst"), dst_len, cap, p("out_off"), p("out_len"), p("src_index"),
                   ctypes.byref(oc), p("hits"), ctypes.byref(tot), ctypes.byref(cnt)]
    for k, v in dict(over or {}).items():
        args[k] = v
    rc = L.pkt_icmp_err_host(*args)
    got = {k: a[:shapes[k][0]] for k, a in bufs.items()}
    got["guards"] = all((a[shapes[k][0]:].view(np.uint8) == 0xA5).all() for k, a in bufs.items())
    got["n_out"], got["bytes_out"], got["cap"] = cnt.value, tot.value, cap
    return rc, got
