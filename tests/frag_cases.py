"""The yardstick and the case builders of pkt_frag_* (tests/test_frag_host.py, test_frag_device.py).

The yardstick is an independent pure-Python model written from the text of include/pktgpu.h (RFC 791's fragmentation
procedure, RFC 1624 for the checksum): it never calls pkt_frag_host.  Given a batch, chain columns, the mtu(s), the
select mask and the flags it returns the expected status / nfrag / first / counters, the output packets byte for byte
and their chain rows.

A case is a list of items (packet bytes, [(type, offset)]); layout() puts them into an indexed or a fixed-stride batch.
"""
import numpy as np

from pktgpu import schema

import compare_cases as C

(FITS, SPLIT, SKIPPED, NO_IP, SPAN, IPV6, BAD_HDR, TRUNC, DF, MTU) = range(10)
NSTATUS = 10
NONE = 0xFFFFFFFF
LAST = 0xFF
ONLY_SPLIT, NO_WRITE = 1, 2
T_ETHER, T_VLAN, T_IPV4, T_IPV6, T_UDP, T_VXLAN = (schema.HDR_ID[k] for k in ("Ether", "Vlan", "IPv4", "IPv6", "UDP", "Vxlan"))
MAXH = schema.MAX_HDRS


def r16(x):
    return (x + 15) // 16 * 16


# ------------------------------------------------------------------ the yardstick
def be16(p, at):
    return p[at] << 8 | p[at + 1]


def fold2(s):
    s = (s & 0xFFFF) + (s >> 16)
    return (s & 0xFFFF) + (s >> 16)


def one(p, hdrs, m, which, selected):
    """(status, e, [output packets]) of packet bytes `p` with the chain `hdrs` (already cut to 16 entries) at mtu m;
    a FITS packet's single output is p itself; e is the IP entry's index (None: no entry)."""
    if not selected:
        return SKIPPED, None, []
    ips = [j for j, (t, _) in enumerate(hdrs) if t in (T_IPV4, T_IPV6)]
    ips = ips[-1:] if which == LAST else ips[which:which + 1]
    if not ips:
        return NO_IP, None, []
    e = ips[0]
    t, ip = hdrs[e]
    v4 = t == T_IPV4
    if ip + (20 if v4 else 40) > len(p):
        return SPAN, e, []
    L = be16(p, ip + 2) if v4 else 40 + be16(p, ip + 4)
    if m == 0 or L <= m:
        return FITS, e, [bytes(p)]
    if not v4:
        return IPV6, e, []
    if p[ip] != 0x45 or L < 20:
        return BAD_HDR, e, []
    if ip + L > len(p):
        return TRUNC, e, []
    if p[ip + 6] & 0x40:
        return DF, e, []
    if m < 28:
        return MTU, e, []
    per = (m - 20) & ~7
    P = L - 20
    k = -(-P // per)
    w = be16(p, ip + 6)
    o = w & 0x1FFF
    if o + (k - 1) * per // 8 > 0x1FFF:
        return BAD_HDR, e, []
    hc = be16(p, ip + 10)
    outs = []
    for j in range(k):
        sl = p[ip + 20 + j * per:ip + 20 + min((j + 1) * per, P)]
        L2 = 20 + len(sl)
        w2 = (w & 0xC000) | (0x2000 if j < k - 1 else w & 0x2000) | (o + j * per // 8)
        hc2 = ~fold2((~hc & 0xFFFF) + (~L & 0xFFFF) + L2 + (~w & 0xFFFF) + w2) & 0xFFFF
        h = bytearray(p[ip:ip + 20])
        h[2:4], h[6:8], h[10:12] = L2.to_bytes(2, "big"), w2.to_bytes(2, "big"), hc2.to_bytes(2, "big")
        outs.append(bytes(p[:ip]) + bytes(h) + bytes(sl))
    return SPLIT, e, outs


def expect(b, chain, mtu, select=None, which=0, flags=0):
    """The model's whole result for batch `b`: status / nfrag / first / hits, n_out, bytes_out, and per output: pkts
    (bytes), src_index, frag_index, rows ([(type, offset)])."""
    n = b["n"]
    out = dict(status=np.zeros(n, np.uint8), nfrag=np.zeros(n, np.uint32), first=np.full(n, NONE, np.uint32),
               hits=np.zeros(NSTATUS, np.uint64), pkts=[], src_index=[], frag_index=[], rows=[])
    for i, (off, ln) in enumerate(C.extents(b)):
        p = b["slab"][off:off + ln].tobytes()
        nh = min(int(chain["n_hdrs"][i]), MAXH)
        hdrs = [(int(chain["hdr_type"][j, i]), int(chain["hdr_off"][j, i])) for j in range(nh)]
        m = int(mtu[i]) if not np.isscalar(mtu) else int(mtu)
        st, e, outs = one(p, hdrs, m, which, select is None or select[i] != 0)
        if st == FITS and flags & ONLY_SPLIT:
            outs = []
        out["status"][i], out["nfrag"][i] = st, len(outs)
        out["hits"][st] += 1
        if outs:
            out["first"][i] = len(out["pkts"])
        for j, q in enumerate(outs):
            out["pkts"].append(q)
            out["src_index"].append(i)
            out["frag_index"].append(j)
            out["rows"].append(hdrs if st == FITS else hdrs[:e + 1])
    out["n_out"] = len(out["pkts"])
    out["bytes_out"] = sum(r16(len(q)) for q in out["pkts"])
    return out


def check(got, want, cap, label=""):
    """got: numpy arrays by name (dst = the whole destination, [0, dst_len)) against the model: the per-source arrays,
    the totals, every output's bytes with its zero padding, the layout rule, the chain rows and the empty tail."""
    for name in ("status", "nfrag", "first", "hits"):
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
        assert g == p + bytes(r16(len(p)) - len(p)), (label, "bytes of output", q, want["src_index"][q], want["frag_index"][q])
        pos += r16(len(p))
    assert pos == want["bytes_out"]
    for name, empty in (("src_index", NONE), ("frag_index", 0)):
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
def rfc1071(h):
    s = sum(be16(h, k) for k in range(0, len(h), 2))
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return s


def ip4_hdr(L, w=0, ident=0x1234, ttl=64, proto=17, b0=0x45):
    h = bytearray(20)
    h[0], h[1] = b0, 0
    h[2:4], h[4:6], h[6:8] = (L & 0xFFFF).to_bytes(2, "big"), ident.to_bytes(2, "big"), w.to_bytes(2, "big")
    h[8], h[9] = ttl, proto
    h[12:16], h[16:20] = bytes([10, 1, 2, 3]), bytes([11, 4, 5, 6])
    h[10:12] = (~rfc1071(h) & 0xFFFF).to_bytes(2, "big")
    return bytes(h)


def pattern(k, seed=0):
    return ((np.arange(k, dtype=np.uint32) * 131 + seed * 17 + 7) % 251).astype(np.uint8).tobytes()


ETH4 = bytes(range(1, 13)) + b"\x08\x00"
ETH6 = bytes(range(1, 13)) + b"\x86\xdd"


def v4(payload_len, w=0, vlan=False, pad=0, seed=0, b0=0x45, L=None, udp=True):
    """Ether / [Vlan] / IPv4 / payload (+ pad trailing bytes): (bytes, hdrs); ip_off 14 or 18."""
    l2 = bytes(range(1, 13)) + b"\x81\x00\x00\x0a\x08\x00" if vlan else ETH4
    L = 20 + payload_len if L is None else L
    p = l2 + ip4_hdr(L, w, b0=b0) + pattern(payload_len, seed) + bytes([0xEE]) * pad
    hdrs = [(T_ETHER, 0)] + ([(T_VLAN, 14)] if vlan else []) + [(T_IPV4, len(l2))]
    if udp and payload_len >= 8:
        hdrs.append((T_UDP, len(l2) + 20))
    return p, hdrs


def v6(payload_len, seed=0):
    h = bytearray(40)
    h[0] = 0x60
    h[4:6] = payload_len.to_bytes(2, "big")
    h[6], h[7] = 17, 64
    p = ETH6 + bytes(h) + pattern(payload_len, seed)
    return p, [(T_ETHER, 0), (T_IPV6, 14)] + ([(T_UDP, 54)] if payload_len >= 8 else [])


def vxlan(payload_len, seed=0, w=0):
    """Ether / IPv4 / UDP / Vxlan / Ether / IPv4 / payload: the inner IP header at 64."""
    inner = ETH4 + ip4_hdr(20 + payload_len, w, ident=0x4321) + pattern(payload_len, seed)
    outer_l = 20 + 8 + 8 + len(inner)
    udp = (4789).to_bytes(2, "big") * 2 + (outer_l - 20).to_bytes(2, "big") + b"\0\0"
    p = ETH4 + ip4_hdr(outer_l) + udp + b"\x08\0\0\0\0\0\x07\0" + inner
    return p, [(T_ETHER, 0), (T_IPV4, 14), (T_UDP, 34), (T_VXLAN, 42), (T_ETHER, 50), (T_IPV4, 64)] + \
        ([(T_UDP, 84)] if payload_len >= 8 else [])


def corrupt(item, by=1):
    """The item with its first IPv4 header's checksum off by `by`."""
    p, hdrs = item
    ip = [o for t, o in hdrs if t == T_IPV4][0]
    q = bytearray(p)
    q[ip + 10:ip + 12] = ((be16(p, ip + 10) + by) & 0xFFFF).to_bytes(2, "big")
    return bytes(q), hdrs


def chain_from(n, rows):
    """Chain columns from per-packet [(type, offset)] lists."""
    ch = dict(n_hdrs=np.zeros(n, np.uint8), hdr_type=np.zeros((MAXH, n), np.uint8), hdr_off=np.zeros((MAXH, n), np.uint16))
    for i, hd in enumerate(rows):
        ch["n_hdrs"][i] = len(hd)
        for j, (t, o) in enumerate(hd[:MAXH]):
            ch["hdr_type"][j, i], ch["hdr_off"][j, i] = t, o
    return ch


def layout(items, kind="indexed", seed=3, stride=None):
    """(batch, chain): "indexed": back to back, packet i at alignment i % 16, the last one ending at the slab's last
    byte; "stride": fixed-stride slots with lens."""
    n = len(items)
    chain = chain_from(n, [h for _, h in items])
    if kind == "indexed":
        return C.indexed([p for p, _ in items], np.random.default_rng(seed), align=[i % 16 for i in range(n)]), chain
    stride = stride or r16(max(len(p) for p, _ in items))
    slab = np.random.default_rng(seed).integers(0, 256, n * stride, dtype=np.uint8)
    for i, (p, _) in enumerate(items):
        slab[i * stride:i * stride + len(p)] = np.frombuffer(p, np.uint8)
    return C.batch(slab, lens=[len(p) for p, _ in items], stride=stride, n=n), chain


def tiled(items, n, stride=64):
    """(batch, chain) of n fixed-stride packets with lens: the few `items`, which share one header list, repeated in
    turn.  Built with numpy alone: layout()'s per-packet loops are too slow at the sizes where the tile scan and the
    counting grid take their other paths."""
    hdrs = items[0][1]
    assert all(h == hdrs for _, h in items) and all(len(p) <= stride for p, _ in items)
    rows = np.full((len(items), stride), 0xEE, np.uint8)
    for j, (p, _) in enumerate(items):
        rows[j, :len(p)] = np.frombuffer(p, np.uint8)
    reps = -(-n // len(items))
    slab = np.tile(rows, (reps, 1))[:n].reshape(-1)
    lens = np.tile(np.array([len(p) for p, _ in items], np.uint32), reps)[:n]
    chain = dict(n_hdrs=np.full(n, len(hdrs), np.uint8), hdr_type=np.zeros((MAXH, n), np.uint8),
                 hdr_off=np.zeros((MAXH, n), np.uint16))
    for j, (t, o) in enumerate(hdrs):
        chain["hdr_type"][j], chain["hdr_off"][j] = t, o
    return C.batch(slab, lens=lens, stride=stride, n=n), chain


MTUS = (28, 68, 576, 1500)


def mix(n, seed=11, big=True):
    """n packets of 60..1600 bytes at ip_off 14 / 18 / 64, a few of 9000 and (big) two of 65535, IPv6 and DF and
    already-fragmented ones among them, with a per-packet mtu from MTUS -> (items, mtu uint16 [n], select)."""
    rng = np.random.default_rng(seed)
    items, mtu = [], []
    for i in range(n):
        r = int(rng.integers(0, 20))
        ln = int(rng.integers(60, 1601))
        m = int(MTUS[int(rng.integers(0, 4))])
        if big and i in (n // 3, 2 * n // 3):
            it = v4(65535 - 34, seed=i, pad=0)
            m = 1500 if i == n // 3 else 576
        elif i % 97 == 50:
            it = v4(9000 - 34, seed=i)
        elif r == 1:
            it = v6(ln - 54, seed=i)
        elif r == 2:
            it = v4(ln - 34, w=0x4000, seed=i)
        elif r == 3:
            it = v4(ln - 34, w=0x2000 | int(rng.integers(0, 200)), seed=i)
        elif r in (4, 5):
            it = vxlan(max(ln - 84, 1), seed=i)
        elif r in (6, 7, 8):
            it = v4(ln - 38, vlan=True, seed=i, pad=int(rng.integers(0, 7)))
        elif r == 9:
            it = (bytes(rng.integers(0, 256, 60, dtype=np.uint8)), [(T_ETHER, 0)])
        else:
            it = v4(ln - 34, seed=i, pad=int(rng.integers(0, 5)) if r == 10 else 0)
        items.append(it)
        mtu.append(m)
    select = (np.arange(n) % 13 != 5).astype(np.uint8)
    return items, np.asarray(mtu, np.uint16), select


_CACHE = {}


def cached(key, build):
    if key not in _CACHE:
        _CACHE[key] = build()
    return _CACHE[key]


# ------------------------------------------------------------------ the host twin, called through the C ABI
def host_call(b, chain, mtu, select=None, which=0, flags=0, cap=None, dst_len=None, skip=(), guard=64, over=None):
    """pkt_frag_host with caller-sized outputs -> (rc, got).  cap / dst_len default to what the model-free sizing pass
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
    per = not np.isscalar(mtu)
    mt = np.ascontiguousarray(mtu, np.uint16) if per else None
    sel = None if select is None else np.ascontiguousarray(select, np.uint8)
    tot, cnt = ctypes.c_uint64(0), ctypes.c_uint64(0)
    if cap is None or dst_len is None:
        rc = L.pkt_frag_host(ctypes.byref(pb), ctypes.byref(ch), which, flags | NO_WRITE, mt.ctypes.data if per else None,
                             0 if per else int(mtu), sel.ctypes.data if sel is not None else None, None, None, None, None, 0, 0,
                             None, None, None, None, None, None, ctypes.byref(tot), ctypes.byref(cnt))
        assert rc == 0
        cap = max(1, cnt.value) if cap is None else cap
        dst_len = tot.value if dst_len is None else dst_len
    shapes = dict(status=(n, np.uint8), nfrag=(n, np.uint32), first=(n, np.uint32), dst=(r16(dst_len) + 16, np.uint8),
                  out_off=(cap, np.uint64), out_len=(cap, np.uint32), src_index=(cap, np.uint32),
                  frag_index=(cap, np.uint16), oc_n_hdrs=(cap, np.uint8), oc_hdr_type=(MAXH * cap, np.uint8),
                  oc_hdr_off=(MAXH * cap, np.uint16), hits=(NSTATUS, np.uint64))
    if flags & NO_WRITE:
        skip = set(skip) | {"dst", "out_off", "out_len", "src_index", "frag_index", "oc_n_hdrs", "oc_hdr_type", "oc_hdr_off"}
    bufs = {}
    for k, (sz, dt) in shapes.items():
        if k in skip:
            continue
        a = np.full(sz + guard, 0xA5, np.uint8).view(np.uint8) if dt == np.uint8 else np.full(sz + guard, 0xA5A5A5A5A5A5A5A5 & (256 ** np.dtype(dt).itemsize - 1), dt)
        if k == "hits":
            a[:sz] = 0
        bufs[k] = a
    p = lambda k: bufs[k].ctypes.data if k in bufs else None  # noqa: E731
    oc = _lib.PktChain(p("oc_n_hdrs"), p("oc_hdr_type"), p("oc_hdr_off"))
    args = [ctypes.byref(pb), ctypes.byref(ch), which, flags, mt.ctypes.data if per else None, 0 if per else int(mtu),
            sel.ctypes.data if sel is not None else None, p("status"), p("nfrag"), p("first"), p("dst"), dst_len, cap,
            p("out_off"), p("out_len"), p("src_index"), p("frag_index"), ctypes.byref(oc), p("hits"), ctypes.byref(tot),
            ctypes.byref(cnt)]
    for k, v in dict(over or {}).items():
        args[k] = v
    rc = L.pkt_frag_host(*args)
    got = {k: a[:shapes[k][0]] for k, a in bufs.items()}
    got["guards"] = all((a[shapes[k][0]:].view(np.uint8) == 0xA5).all() for k, a in bufs.items())
    if "dst" in bufs:
        got["dst_rest"] = bufs["dst"]
    got["n_out"], got["bytes_out"], got["cap"] = cnt.value, tot.value, cap
    return rc, got
