"""pkt_tunnel_create_host / pkt_tunnel_encap_host / pkt_tunnel_decap_host (Tunnels(None, entries)): the host twins against
tunnel_cases' yardstick (an independent Python model) and against the reference's own tunnel builders as pktgpu/gen.py
restates them.  The twins run the inline code of pktgpu_tunnel.hpp that the kernels share, so the table's checks and
lookup, every decision step, the header words and the rows are covered here on the CPU; test_tunnel_device.py adds the
loads, the scan and the chunk walk."""
import ctypes

import numpy as np
import pytest

import pktgpu
from pktgpu import gen, schema

import tunnel_cases as T

INVALID = -1
ENTS = T.table()
M1, M2 = "00:01:02:03:04:05", "00:06:07:08:09:0a"


@pytest.fixture(scope="module")
def HT():
    return T.HostTable(ENTS)


def emix(kind):
    def build():
        items, tun, ent, sel = T.encap_mix(300)
        b, ch = T.layout(items, kind)
        return b, ch, tun, ent, sel
    return T.cached(("emix", kind), build)


def dmix(kind):
    def build():
        items, sel = T.decap_mix(300)
        b, ch = T.layout(items, kind)
        return b, ch, sel
    return T.cached(("dmix", kind), build)


# ------------------------------------------------------------------ the reference's builders
def builder_cases():
    """(name, source item, entry, ident, the builder's packet, excluded byte ranges, compared length)."""
    ref = gen.reference_22_packets()
    tcp, udp_, udp6, tcp6 = ref[0], ref[1], ref[4], ref[3]
    ip = lambda p: (lambda q: (q.remove(0), q)[1])(p.clone())  # noqa: E731
    item = lambda p: (bytes(p.to_vec()), T.L4.hdrs_of(bytes(p.to_vec())))  # noqa: E731
    A4, B4, A6, B6 = "192.168.0.199", "192.168.0.1", "AAAA::1", "BBBB::1"
    m1, m2 = bytes.fromhex(M1.replace(":", "")), bytes.fromhex(M2.replace(":", ""))
    out = []
    g = gen.create_gre_packet(M1, M2, False, 10, 3, 5, A4, B4, 0x14, 61, 777, 0x4000, [], 0, 0, 1, 0, 0, 0, 0, 0, 0,
                              0xCAFEF00D, 0, b"", ip(tcp))
    out.append(("gre", item(tcp), T.entry(T.GRE, A4, B4, ttl=61, tos=0x14, id=0xCAFEF00D, flags=T.F_KEY | T.F_DF), 777, g, [], None))
    g = gen.create_gre_packet(M1, M2, False, 10, 3, 5, A4, B4, 0, 64, 5, 0, [], 0, 0, 1, 0, 0, 0, 0, 0, 0, 9, 0, b"", ip(udp6))
    out.append(("gre_v6_inner", item(udp6), T.entry(T.GRE, A4, B4, id=9, flags=T.F_KEY), 5, g, [], None))
    for name, src in (("ipv4ip_4", tcp), ("ipv4ip_6", udp6)):
        g = gen.create_ipv4ip_packet(M1, M2, False, 10, 3, 5, A4, B4, 0, 64, 65535, 0x4000, [], ip(src))
        out.append((name, item(src), T.entry(T.IPIP, A4, B4, flags=T.F_DF), 65535, g, [], None))
    for name, src in (("ipv6ip_4", udp_), ("ipv6ip_6", tcp6)):
        g = gen.create_ipv6ip_packet(M1, M2, False, 10, 3, 0x2E, 0, 64, A6, B6, ip(src))
        out.append((name, item(src), T.entry(T.IPIP, A6, B6, tos=0x2E), 0, g, [], None))
    g = gen.create_vxlan_packet(M1, M2, False, 10, 3, 5, A4, B4, 0, 64, 4242, 0x4000, [], gen.VXLAN_PORT, 9090, False, 2000,
                                udp_.clone())
    e = T.entry(T.VXLAN, A4, B4, id=2000, sport=(9090, 9090), eth_dst=m1, eth_src=m2, flags=T.F_DF)
    out.append(("vxlan", item(udp_), e, 4242, g, [(24, 26)], None))
    g = gen.create_vxlanv6_packet(M1, M2, False, 10, 3, 5, 0, 64, A6, B6, gen.VXLAN_PORT, 9090, False, 2000, tcp.clone())
    e = T.entry(T.VXLAN, A6, B6, tos=5, id=2000, sport=(9090, 9090), eth_dst=m1, eth_src=m2)
    out.append(("vxlanv6", item(tcp), e, 0, g, [(60, 62)], 70))
    return out


BUILDERS = builder_cases()


@pytest.mark.parametrize("case", BUILDERS, ids=[c[0] for c in BUILDERS])
def test_encap_equals_the_references_builders(case):
    """One packet per case with ip_id = ident.  create_gre_packet (k = 1), create_ipv4ip_packet and create_ipv6ip_packet
    equal the output byte for byte; create_vxlan_packet but for bytes 24..25, where the builder's checksum is stale (Q9)
    and the output holds gen.ipv4_checksum of its 20 header bytes; create_vxlanv6_packet over the first 70 bytes but for
    the UDP checksum's two (it stores 0xFFFF and appends the inner headers twice, Q12).  The model is held to the same."""
    name, src, e, ident, built, excl, upto = case
    built = bytes(built.to_vec())
    b, ch = T.layout([src], "indexed")
    rc, got = T.host_call("encap", T.HostTable([e]), b, ch, 0, None, ident)
    assert rc == 0 and got["n_out"] == 1 and got["status"][0] == T.E_OK
    model = T.expect("encap", b, ch, [e], 0, None, ident)["pkts"][0]
    for out in (T.outputs(got)[0], model):
        n = upto or len(built)
        assert upto or len(out) == len(built), name
        bad = [k for k in range(n) if out[k] != built[k] and not any(a <= k < z for a, z in excl)]
        assert not bad, (name, bad[:8])
        if name == "vxlan":
            assert T.be16(out, 24) == gen.ipv4_checksum(out[14:34]) != T.be16(built, 24)
        if name == "vxlanv6":
            assert out[60:62] == b"\0\0" and built[60:62] == b"\xff\xff"


# ------------------------------------------------------------------ the model, both layouts
@pytest.mark.parametrize("kind", ["indexed", "stride"])
def test_encap_mix_against_the_model(HT, kind):
    """The 22 reference packets, 0..2 VLAN tags, MPLS, raw IP, both inner versions, every flag, per-packet tunnels over 3
    kinds x 2 outer versions and entropy over full and one-port ranges; indexed with packet i at alignment i % 16 and the
    last packet ending on the slab's last byte, and fixed stride.  Every status but TOO_BIG (test_outer_length_edges)."""
    b, ch, tun, ent, sel = emix(kind)
    want = T.expect("encap", b, ch, ENTS, tun, ent, 65530, sel)
    assert all(np.bincount(want["status"], minlength=10)[s] for s in range(10) if s != T.E_TOO_BIG)
    rc, got = T.host_call("encap", HT, b, ch, tun, ent, 65530, sel)
    assert rc == 0 and got["guards"]
    T.check_all(got, want, got["cap"], kind)
    assert got["hits"].sum() == b["n"]


@pytest.mark.parametrize("kind", ["indexed", "stride"])
def test_decap_mix_against_the_model(HT, kind):
    b, ch, sel = dmix(kind)
    want = T.expect("decap", b, ch, ENTS, select=sel)
    assert np.bincount(want["status"], minlength=11).all(), np.bincount(want["status"], minlength=11)
    rc, got = T.host_call("decap", HT, b, ch, select=sel)
    assert rc == 0 and got["guards"]
    T.check_all(got, want, got["cap"], kind)
    assert got["hits"].sum() == b["n"]


@pytest.mark.parametrize("n", [0, 1, 64, 65, 256, 257])
@pytest.mark.parametrize("tunnel", [0, 3, "array"])
def test_sizes_and_tunnel_all(HT, n, tunnel):
    """The wave and tile edges, with `tunnel` as an array and as tunnel_all."""
    items, tun, ent, _ = T.encap_mix(257)
    b, ch = T.layout(items[:n], "indexed") if n else (T.C.batch(np.zeros(16, np.uint8), [], []), T.G.chain_from(0, []))
    tn = tun[:n] if tunnel == "array" else tunnel
    want = T.expect("encap", b, ch, ENTS, tn, ent[:n], 7)
    rc, got = T.host_call("encap", HT, b, ch, tn, ent[:n], 7)
    assert rc == 0 and got["guards"]
    T.check_all(got, want, got["cap"], (n, tunnel))


def test_entropy_spreads_over_the_port_range(HT):
    """sport_lo == sport_hi gives that port whatever the entropy; the full range gives entropy % 65536; no entropy sport_lo."""
    it = T.pkt(T.udp(30, 1))
    ent = np.array([0, 1, 65535, 65536, 0xFFFFFFFF, 123456789], np.uint32)
    b, ch = T.layout([it] * len(ent), "indexed")
    for t, ports in ((0, [9090] * 6), (6, [int(e) % 65536 for e in ent]), (9, [1024 + int(e) % 4 for e in ent])):
        rc, got = T.host_call("encap", HT, b, ch, t, ent)
        H = 20 if ENTS[t]["ipver"] == 4 else 40
        assert [T.be16(p, 14 + H) for p in T.outputs(got)] == ports
        T.check_all(got, T.expect("encap", b, ch, ENTS, t, ent), got["cap"], t)
    rc, got = T.host_call("encap", HT, b, ch, 9, None)
    assert [T.be16(p, 54) for p in T.outputs(got)] == [1024] * 6


def test_outer_length_edges(HT):
    """Inner lengths that put the outer length field at exactly 65535 (OK) and at 65536 (TOO_BIG), per kind."""
    items = [T.big(65535 - 36 - 14), T.big(65536 - 36 - 14),           # VXLAN / IPv4: 36 + len
             T.big(65535 - 16 - 14), T.big(65536 - 16 - 14),           # VXLAN / IPv6: 16 + len
             T.big(65535 - 24), T.big(65536 - 24),                     # GRE / IPv4, no key: 24 + L
             T.big(65535 - 28), T.big(65536 - 28),                     # GRE / IPv4 with the key
             T.big(65535 - 20, v6=True), T.big(65536 - 20, v6=True)]   # IPIP / IPv4 around IPv6
    tun = np.array([0, 0, 9, 9, 2, 2, 7, 7, 4, 4], np.uint32)
    b, ch = T.layout(items, "indexed")
    want = T.expect("encap", b, ch, ENTS, tun)
    assert list(want["status"]) == [T.E_OK, T.E_TOO_BIG] * 5
    rc, got = T.host_call("encap", HT, b, ch, tun)
    assert rc == 0 and got["guards"]
    T.check_all(got, want, got["cap"], "edges")


def test_rows_at_16_and_17(HT):
    """n_hdrs plus the added rows landing on exactly 16 (OK) and 17 (DEPTH), and n_hdrs 255 taken as 16."""
    items = [T.deep(12), T.deep(13), T.deep(15), T.deep(16), T.deep(13), T.deep(14), T.deep(14), T.deep(15)]
    tun = np.array([0, 0, 4, 4, 3, 3, 2, 2], np.uint32)  # VXLAN + 4, IPIP + 1, GRE with key + 3, GRE + 2
    b, ch = T.layout(items, "indexed")
    want = T.expect("encap", b, ch, ENTS, tun)
    assert list(want["status"]) == [T.E_OK, T.E_DEPTH] * 4
    assert [len(r) for r in want["rows"]] == [16] * 4
    rc, got = T.host_call("encap", HT, b, ch, tun)
    T.check_all(got, want, got["cap"], "depth")
    ch2 = dict(ch, n_hdrs=np.full(8, 255, np.uint8))
    rc, got = T.host_call("encap", HT, b, ch2, tun)
    assert rc == 0 and got["guards"]
    T.check_all(got, T.expect("encap", b, ch2, ENTS, tun), got["cap"], "n_hdrs 255")


# ------------------------------------------------------------------ properties
def test_decap_of_encap_returns_the_packets(HT):
    """decap(encap(x)) is x exactly for VXLAN, and x cut to its IP length for the L3 kinds, with x's chain."""
    items, tun, ent, _ = T.encap_mix(200)
    b, ch = T.layout(items, "indexed")
    rc, e = T.host_call("encap", HT, b, ch, tun % 14, ent)
    src = e["src_index"][:e["n_out"]]
    eb, ech = T.layout(T.out_items(e), "stride")
    rc, d = T.host_call("decap", HT, eb, ech)
    assert rc == 0 and (d["status"] == T.D_OK).all() and d["n_out"] == e["n_out"] > 100
    back = T.out_items(d)
    for q, i in enumerate(src):
        p, hdrs = items[i]
        t = int(tun[i] % 14)
        if ENTS[t]["kind"] != T.VXLAN:
            j = T.pick_ip(hdrs, 0)
            ip = hdrs[j][1]
            L = T.be16(p, ip + 2) if hdrs[j][0] == T.T_IPV4 else 40 + T.be16(p, ip + 4)
            p = p[:ip + L]
        assert back[q] == (p, hdrs[:T.MAXH]), (q, i, t)
        assert d["tunnel_out"][q] == t + 14  # the other end's entry


def test_exact_entry_before_any_remote(HT):
    """Entries 12 (remote REM4B) and 13 (ANY_REMOTE) share local address and VNI: a packet from REM4B finds 12, one from
    REM4 (entry 28's packets) finds 13."""
    it = T.pkt(T.udp(40, 2))
    b, ch = T.layout([it, it], "indexed")
    rc, e = T.host_call("encap", HT, b, ch, np.array([26, 28], np.uint32))
    assert e["n_out"] == 2
    eb, ech = T.layout(T.out_items(e), "indexed")
    rc, d = T.host_call("decap", HT, eb, ech)
    assert list(d["status"]) == [T.D_OK] * 2 and list(d["tunnel_out"]) == [12, 13]


def test_forged_chains_give_a_status(HT):
    """Offsets past the packet and n_hdrs 255 end in a status; exact-size heap blocks under the sanitizers are
    tests/cpp/tunnel_host_san.cpp's."""
    items = T.forged()
    b, ch = T.layout(items, "indexed")
    ch = dict(ch, n_hdrs=np.where(np.arange(len(items)) % 2, 255, ch["n_hdrs"]).astype(np.uint8))
    for t in (0, 2, 5):
        rc, got = T.host_call("encap", HT, b, ch, t)
        assert rc == 0 and got["guards"]
        T.check_all(got, T.expect("encap", b, ch, ENTS, t), got["cap"], t)
    rc, got = T.host_call("decap", HT, b, ch)
    assert rc == 0 and got["guards"]
    T.check_all(got, T.expect("decap", b, ch, ENTS), got["cap"], "decap")


# ------------------------------------------------------------------ capacity
@pytest.mark.parametrize("op", ["encap", "decap"])
def test_plan_only_totals_and_one_too_small(HT, op):
    b, ch = (emix("indexed")[:2]) if op == "encap" else (dmix("indexed")[:2])
    args = dict(tunnel=emix("indexed")[2]) if op == "encap" else {}
    rc, full = T.host_call(op, HT, b, ch, **args)
    rc, plan = T.host_call(op, HT, b, ch, flags=T.NO_WRITE, **args)
    assert rc == 0 and (plan["n_out"], plan["bytes_out"]) == (full["n_out"], full["bytes_out"])
    assert np.array_equal(plan["status"], full["status"]) and np.array_equal(plan["out_index"], full["out_index"])
    for cap, dl in ((full["n_out"] - 1, full["bytes_out"]), (full["n_out"], full["bytes_out"] - 1)):
        rc, got = T.host_call(op, HT, b, ch, cap=cap, dst_len=dl, **args)
        assert rc == INVALID and (got["n_out"], got["bytes_out"]) == (full["n_out"], full["bytes_out"])
        assert got["guards"] and (got["dst"] == 0xA5).all() and (got["out_len"] == 0xA5A5A5A5).all()
    for skip in (("status",), ("out_index", "hits"), ("src_index", "oc_hdr_type"), ("oc_n_hdrs", "oc_hdr_type", "oc_hdr_off")):
        rc, got = T.host_call(op, HT, b, ch, skip=skip, **args)
        assert rc == 0 and got["guards"]
        assert np.array_equal(got["dst"][:full["bytes_out"]], full["dst"][:full["bytes_out"]])


# ------------------------------------------------------------------ refusals
CREATE_REFUSALS = [
    (lambda e: e.update(kind=3), "entry 1: unknown kind"),
    (lambda e: e.update(ipver=5), "entry 1: ipver is neither 4 nor 6"),
    (lambda e: e.update(flags=32), "entry 1: unknown flag bits"),
    (lambda e: e.update(id=1 << 24), "entry 1: VNI above 2^24 - 1"),
    (lambda e: e.update(sport=(2000, 1999)), "entry 1: sport_lo above sport_hi"),
    (lambda e: e.update(flags=T.F_KEY), "entry 1: PKT_TUN_F_KEY on an entry that is not GRE"),
    (lambda e: e.update(kind=T.GRE, id=0, flags=T.F_CSUM), "entry 1: PKT_TUN_F_UDP_CSUM on an entry that is not VXLAN"),
    (lambda e: e.update(dst=T.addr(T.REM4B), id=2000), "entries 0 and 1 have the same decap key"),
    (lambda e: e.update(flags=T.F_ANY, id=2000), None),  # an exact and an ANY_REMOTE key are two keys
]


def create(rec, n=None):
    from pktgpu import _lib
    L = _lib.load()
    h = ctypes.c_void_p()
    rc = L.pkt_tunnel_create_host(None if rec is None else rec.ctypes.data, len(rec) if n is None else n, ctypes.byref(h))
    msg = (L.pkt_tunnel_last_error(None) or b"").decode()
    if rc == 0:
        L.pkt_tunnel_destroy(h)
    return rc, msg


@pytest.mark.parametrize("k", range(len(CREATE_REFUSALS)))
def test_create_refusals(k):
    change, text = CREATE_REFUSALS[k]
    ents = [T.entry(T.VXLAN, T.LOC4, T.REM4B, id=2000), T.entry(T.VXLAN, T.LOC4, T.REM4, id=5)]
    change(ents[1])
    rc, msg = create(T.records(ents))
    if text is None:
        assert rc == 0
    else:
        assert rc == INVALID and msg == "pkt_tunnel_create: " + text


def test_create_refusals_of_the_table_itself():
    rec = T.records(ENTS)
    assert create(None, 3) == (INVALID, "pkt_tunnel_create: null entries")
    assert create(rec, 0) == (INVALID, "pkt_tunnel_create: count is 0 or above PKT_TUN_MAX_ENTRIES")
    assert create(rec, 65537) == (INVALID, "pkt_tunnel_create: count is 0 or above PKT_TUN_MAX_ENTRIES")
    rec["zero"][2] = 1
    assert create(rec) == (INVALID, "pkt_tunnel_create: entry 2: non-zero `zero`")
    from pktgpu import _lib
    assert _lib.load().pkt_tunnel_create_host(rec.ctypes.data, 1, None) == INVALID
    assert _lib.load().pkt_tunnel_last_error(None) == b"pkt_tunnel_create_host: null argument"
    assert _lib.load().pkt_sizeof_tunnel_entry() == 64 == schema.TUNNEL_ENTRY_DTYPE.itemsize


def test_a_table_of_65536_entries():
    """The largest table: every entry found again by its own key."""
    n = 65536
    rec = np.zeros(n, schema.TUNNEL_ENTRY_DTYPE)
    rec["kind"], rec["ipver"] = T.VXLAN, 4
    rec["id"] = np.arange(n)
    rec["src"][:, :4] = [192, 0, 2, 1]
    rec["dst"][:, 0] = 10
    rec["dst"][:, 2] = np.arange(n) >> 8
    rec["dst"][:, 3] = np.arange(n) & 255
    tun = pktgpu.Tunnels(None, rec)
    it = T.pkt(T.udp(20, 1))
    pick = np.array([0, 1, 255, 256, 40000, 65535], np.uint32)
    b, ch = T.layout([it] * len(pick), "indexed")
    e = tun.encap(b, ch, tunnel=pick)
    # the other end's view of those six tunnels, and the packets looped back to it
    rev = rec[pick].copy()
    rev["src"], rev["dst"] = rec[pick]["dst"], rec[pick]["src"]
    d = pktgpu.Tunnels(None, rev).decap(e.batch(), e.out_chain)
    assert list(d.status) == [T.D_OK] * 6 and list(d.tunnel_out) == list(range(6))
    assert [d.slab[int(o):int(o) + int(ln)].tobytes() for o, ln in zip(d.offsets, d.lens)] == [it[0]] * 6


# positions in pkt_tunnel_encap_host's argument list (for `over`)
A_BATCH, A_CHAIN, A_WHICH, A_FLAGS, A_TUN, A_TUNNEL, A_TUNNEL_ALL, A_ENTROPY = range(8)
A_DST, A_CAP, A_OUT_OFF, A_HITS = 12, 14, 15, 19


def test_call_refusals(HT):
    b, ch, tun, ent, sel = emix("indexed")
    odd = np.zeros(64, np.uint8)

    def refused(op, text, **kw):
        kw.setdefault("cap", 512)
        kw.setdefault("dst_len", 1 << 19)
        rc, got = T.host_call(op, HT, b, ch, **kw)
        assert rc == INVALID and HT.error() == f"pkt_tunnel_{op}_host: {text}", (HT.error(), text)

    for op in ("encap", "decap"):
        refused(op, "unknown flag bits", flags=2, cap=1, dst_len=16)
        refused(op, "which_ip is neither below 16 nor PKT_FLOW_LAST", which=16)
        refused(op, "null argument", over={A_CHAIN: None})
        refused(op, "null dst, out_off or out_len without PKT_TUN_NO_WRITE", skip=("dst",))
        rc, got = T.host_call(op, HT, b, ch, over={A_TUN: None}, cap=1, dst_len=16)
        from pktgpu import _lib
        assert rc == INVALID and _lib.load().pkt_tunnel_last_error(None).decode() == f"pkt_tunnel_{op}_host: null tunnel table"
    refused("encap", "a uint32_t array is not 4-byte aligned", over={A_TUNNEL: odd.ctypes.data + 2})
    refused("encap", "a uint32_t array is not 4-byte aligned", over={A_ENTROPY: odd.ctypes.data + 1})
    refused("encap", "dst not 16-byte aligned", over={A_DST: odd.ctypes.data + 8 - odd.ctypes.data % 16 + 16})
    refused("encap", "out_cap is 0 or >= 2^32", over={A_CAP: 0})
    refused("encap", "hits not 8-byte aligned", over={A_HITS: odd.ctypes.data + 4 - odd.ctypes.data % 8 + 8})
    # the wrapper carries the text
    with pytest.raises(ValueError, match="pkt_tunnel_encap_host: which_ip is neither below 16 nor PKT_FLOW_LAST"):
        pktgpu.Tunnels(None, T.records(ENTS)).encap(b, ch, tunnel=0, which_ip=77)


def test_python_wrapper(HT):
    """Parser-free Tunnels(None, entries) with dict entries, flow_keys-style entropy and _Produced's attributes."""
    tun = pktgpu.Tunnels(None, [dict(kind="vxlan", src=T.LOC4, dst=T.REM4, id=2000, sport=(1000, 1999), eth_dst=M1, eth_src=M2,
                                     flags=schema.TUN_F_UDP_CSUM),
                                dict(kind="gre", src=T.REM4, dst=T.LOC4), dict(kind=schema.TUN_VXLAN, src=T.REM4, dst=T.LOC4, id=2000)])
    assert len(tun) == 3 and tun.entries["ipver"].tolist() == [4, 4, 4]
    items = [T.pkt(T.udp(20 + k, k)) for k in range(5)]
    b, ch = T.layout(items, "indexed")
    h = np.arange(5, dtype=np.uint64) * 0x100000001 + 5000
    e = tun.encap(b, ch, tunnel=0, entropy={"rss": None, "hash": h}, hits=True)
    ports = [T.be16(e.slab[int(o):int(o) + 50].tobytes(), 34) for o in e.offsets]
    assert ports == [1000 + int(x & 0xFFFFFFFF) % 1000 for x in h]
    assert e.n_out == 5 and e.hits[0] == 5 and (e.status == 0).all()
    d = tun.decap(e.batch(), e.out_chain)
    assert list(d.tunnel_out) == [2] * 5
    assert [d.slab[int(o):int(o) + int(ln)].tobytes() for o, ln in zip(d.offsets, d.lens)] == [p for p, _ in items]
    assert tun.encap(b, ch, tunnel=0, plan_only=True).bytes_out == e.bytes_out
