"""pkt_lpm_create_host and the host handle's lookups (Parser.lpm(host=True) / pktgpu.Lpm(None, routes)) against
lpm_cases' yardstick: a dict of integer prefixes per (version, length), tried from the longest length down.  The host
handle runs the same compile and the same walk as the kernel (pktgpu_lpm.hpp), so this file covers both.  No device."""
import ctypes
import ipaddress

import numpy as np
import pytest

import pktgpu
from pktgpu import _lib, schema

import lpm_cases as X

INVALID, UNSUPPORTED = -1, -4


def host(routes, default=X.DEFAULT, max_bytes=0):
    return pktgpu.Lpm(None, X.to_array(routes) if not isinstance(routes, np.ndarray) else routes, default, max_bytes)


_H = {}


def handle(name):
    """One host handle per named case for the module."""
    if name not in _H:
        _H[name] = host(X.cached(name)[0])
    return _H[name]


def test_sizes_and_constants():
    L = _lib.load()
    assert L.pkt_sizeof_lpm_route() == ctypes.sizeof(_lib.PktLpmRoute) == schema.LPM_ROUTE_DTYPE.itemsize == 24
    assert ctypes.sizeof(_lib.PktLpmInfo) == 56
    assert (schema.LPM_OK, schema.LPM_NO_ROUTE, schema.LPM_NO_IP, schema.LPM_SPAN, schema.LPM_SKIPPED) == (0, 1, 2, 3, 4)
    assert pktgpu.LPM_NONE == schema.LPM_NONE == 0xFFFFFFFF and schema.LPM_SRC == 1 and schema.LPM_MAX_ROUTES == 1 << 24
    assert _lib.PktLpmRoute.nexthop.offset == 20 and _lib.PktLpmRoute.ipver.offset == 16


@pytest.mark.parametrize("name", X.SMALL + ["random", "large"])
def test_keys_against_the_model(name):
    routes, probes, model, want = X.cached(name)
    if name in ("random", "large"):
        X.assert_mix(want, name)  # on the model alone, before any comparison
    X.check(handle(name).lookup_keys(X.keys_of(probes)), want, name)


def test_large_table_passes_two_to_the_16_entries():
    routes, _, _, _ = X.cached("large")
    info = handle("large").info()
    assert len({a >> 16 for v, p, a, _ in routes if p == 24}) > 300
    assert info["nodes_v4"] * 256 > 1 << 16 and info["routes_v4"] == len(routes) > 70000 and info["depth_v4"] == 2


def test_routes_as_strings():
    routes, probes, _, want = X.cached("siblings")
    h = pktgpu.Lpm(None, X.to_strings(routes), X.DEFAULT)
    assert np.array_equal(h.routes, X.to_array(routes))
    X.check(h.lookup_keys(X.keys_of(probes)), want, "strings")
    nets = [(ipaddress.ip_network(s), nh) for s, nh in X.to_strings(routes)]  # stdlib networks pass as they are
    assert np.array_equal(pktgpu.lpm_routes(nets), X.to_array(routes))
    with pytest.raises(ValueError):
        pktgpu.lpm_routes([("10.0.0.1/8", 1)])  # host bits set: stdlib ipaddress refuses
    with pytest.raises(ValueError):
        pktgpu.lpm_routes(np.zeros(3, np.uint8))


def test_src_and_dict_form_of_lookup_keys():
    routes, probes, model, want = X.cached("random")
    keys = X.keys_of(probes)
    flipped = [(v, a ^ ((1 << X.W[v]) - 1)) for v, a in probes]  # keys_of stores the complement as src
    X.check(handle("random").lookup_keys(keys, src=True), X.expect_probes(model, flipped), "src")
    st = (np.arange(len(probes)) % 5 == 2).astype(np.uint8)
    got = handle("random").lookup_keys(dict(keys=keys, status=st))
    X.check(got, X.expect_probes(model, probes, st), "dict with status")


def test_skipped_keys():
    routes, probes, model, _ = X.cached("boundary")
    probes = list(probes[:40])
    for k, ver in ((3, 0), (9, 5), (17, 7), (21, 64)):
        probes[k] = (ver, probes[k][1] & 0xFFFFFFFF)
    st = np.zeros(len(probes), np.uint8)
    st[[1, 9, 30]] = (1, 2, 255)
    want = X.expect_probes(model, probes, st)
    assert (want["status"] == X.SKIPPED).sum() == 6
    sel = want["status"] == X.SKIPPED
    assert (want["route"][sel] == X.NONE).all() and (want["nexthop"][sel] == X.DEFAULT).all() and (want["plen"][sel] == 255).all()
    X.check(handle("boundary").lookup_keys(X.keys_of(probes), st), want, "skipped")


# ------------------------------------------------------------------ lookup_batch
@pytest.mark.parametrize("name", X.SMALL + ["random"])
@pytest.mark.parametrize("layout", ["indexed", 96])
def test_batch_against_the_model(name, layout):
    routes, probes, model, _ = X.cached(name)
    b, ch = X.batch_case(X.probe_items(probes[:600]), layout)
    for src in (False, True):
        X.check(handle(name).lookup(b, ch, src=src), X.expect_batch(model, b, ch, src=src), f"{name} {layout} src={src}")


def test_packet_kinds():
    """Ether/IPv4/UDP, Ether/Vlan/IPv6/TCP, an ARP packet (NO_IP), a packet cut inside its IP header (SPAN) and
    n_hdrs == 0, with dst and src."""
    routes, probes, model, _ = X.cached("random")
    b, ch = X.batch_case(X.mixed_items(probes[:300]), "indexed")
    for which in (0, X.LAST):
        for src in (False, True):
            want = X.expect_batch(model, b, ch, which, src)
            assert set(np.unique(want["status"])) == {X.OK, X.NO_ROUTE, X.NO_IP, X.SPAN}
            X.check(handle("random").lookup(b, ch, which_ip=which, src=src), want, f"kinds {which} {src}")
    want = X.expect_batch(model, b, ch, 1)  # no packet has a second IP header
    assert (want["status"] == X.NO_IP).all()
    X.check(handle("random").lookup(b, ch, which_ip=1), want, "which_ip 1")


def test_vxlan_which_ip():
    routes, probes, model, _ = X.cached("large")
    v4 = [a for v, a in probes if v == 4]
    items = [X.vxlan_for(v4[2 * k], v4[2 * k + 1]) for k in range(120)] + X.probe_items(probes[:30])
    b, ch = X.batch_case(items, "indexed")
    wants = {w: X.expect_batch(model, b, ch, w) for w in (0, 1, X.LAST)}
    assert not np.array_equal(wants[0]["route"], wants[1]["route"])
    assert np.array_equal(wants[1]["route"][:120], wants[X.LAST]["route"][:120])
    assert (wants[1]["status"][120:] == X.NO_IP).all() and (wants[X.LAST]["status"][120:] != X.NO_IP).all()
    for w, want in wants.items():
        X.check(handle("large").lookup(b, ch, which_ip=w), want, f"vxlan which_ip={w}")
        X.check(handle("large").lookup(b, ch, which_ip=w, src=True), X.expect_batch(model, b, ch, w, True), f"vxlan src {w}")


def test_clamped_lengths_and_wild_columns():
    """A lens entry that runs past the slab is clamped (the IP header then lies outside: SPAN), and chain columns
    that point anywhere never make the call read outside the packet."""
    routes, probes, model, _ = X.cached("random")
    b, ch = X.batch_case(X.probe_items(probes[:64]), "indexed")
    b["lens"] = b["lens"].copy()
    b["lens"][-1] = 1 << 20
    b["slab"] = b["slab"][:int(b["offsets"][-1]) + 30]  # the last packet is cut by the slab's end
    ch = {k: v.copy() for k, v in ch.items()}
    for i, o in ((5, 65535), (6, 40000)):  # the IP entry's offset
        j = int(np.flatnonzero(np.isin(ch["hdr_type"][:, i], (X.T_IPV4, X.T_IPV6)))[0])
        ch["hdr_off"][j, i] = o
    ch["n_hdrs"][7] = 200  # taken as 16
    want = X.expect_batch(model, b, ch)
    assert want["status"][-1] == X.SPAN and want["status"][5] == X.SPAN and want["status"][6] == X.SPAN
    X.check(handle("random").lookup(b, ch), want, "clamped")


# ------------------------------------------------------------------ raw calls: NULL outputs and refusals
def raw_batch(h, b, ch, r=(), outputs=(True,) * 4, which=0, flags=0):
    """pkt_lpm_lookup_batch with argument positions replaced -> (rc, outputs, keep)."""
    L = _lib.load()
    pb, keep = pktgpu._host_batch(_lib, b)
    cols = [np.ascontiguousarray(ch[k]) for k in ("n_hdrs", "hdr_type", "hdr_off")]
    pc = _lib.PktChain(*[c.ctypes.data for c in cols])
    out = [np.full(pb.n, 0x77, X.DT[k]) if w else None for k, w in zip(X.NAMES, outputs)]
    a = [h._t, ctypes.byref(pb), ctypes.byref(pc), which, flags, *[None if x is None else x.ctypes.data for x in out], None]
    for k, v in dict(r).items():
        a[k] = v
    return L.pkt_lpm_lookup_batch(*a), dict(zip(X.NAMES, out)), (pb, pc, keep, cols)


def raw_keys(h, keys, status=None, r=(), outputs=(True,) * 4, flags=0, n=None):
    L = _lib.load()
    keys = np.ascontiguousarray(keys, np.uint8)
    n = keys.shape[0] if n is None else n
    out = [np.full(keys.shape[0], 0x77, X.DT[k]) if w else None for k, w in zip(X.NAMES, outputs)]
    a = [h._t, keys.ctypes.data, None if status is None else status.ctypes.data, n, flags,
         *[None if x is None else x.ctypes.data for x in out], None]
    for k, v in dict(r).items():
        a[k] = v
    return L.pkt_lpm_lookup_keys(*a), dict(zip(X.NAMES, out)), keys


def err(h):
    return _lib.load().pkt_lpm_last_error(h._t).decode()


def test_null_outputs():
    routes, probes, model, want_k = X.cached("random")
    h = handle("random")
    b, ch = X.batch_case(X.mixed_items(probes[:200]), "indexed")
    want_b = X.expect_batch(model, b, ch)
    keys = X.keys_of(probes[:200])
    want_k = {k: v[:200] for k, v in want_k.items()}
    combos = [tuple(j == k for j in range(4)) for k in range(4)] + [tuple(j != k for j in range(4)) for k in range(4)]
    for outputs in combos:
        rc, got, _ = raw_batch(h, b, ch, outputs=outputs)
        assert rc == 0
        X.check(got, want_b, f"batch {outputs}")
        rc, got, _ = raw_keys(h, keys, outputs=outputs)
        assert rc == 0
        X.check(got, want_k, f"keys {outputs}")
    assert raw_batch(h, b, ch, outputs=(False,) * 4)[0] == 0
    assert raw_keys(h, keys, outputs=(False,) * 4)[0] == 0


def test_empty_calls_and_empty_table():
    routes, probes, model, _ = X.cached("random")
    h = handle("random")
    b, ch = X.batch_case(X.probe_items(probes[:8]), 96)
    pb, _ = pktgpu._host_batch(_lib, b)
    empty = _lib.PktBatch(pb.slab, pb.slab_len, None, None, 96, 0, 0)
    rc, got, _ = raw_batch(h, b, ch, {1: ctypes.byref(empty)})
    assert rc == 0 and all((x == 0x77).all() for x in got.values())
    rc, got, _ = raw_keys(h, X.keys_of(probes[:8]), n=0)
    assert rc == 0 and all((x == 0x77).all() for x in got.values())
    assert _lib.load().pkt_lpm_lookup_keys(h._t, None, None, 0, 0, None, None, None, None, None) == 0
    # nroutes == 0: every IP packet is NO_ROUTE
    e = host([])
    assert e.info() == dict(routes_v4=0, routes_v6=0, nodes_v4=0, nodes_v6=0, depth_v4=0, depth_v6=0, bytes=2 * 4 * 65536)
    m0 = X.Model([])
    b, ch = X.batch_case(X.mixed_items(probes[:50]), "indexed")
    want = X.expect_batch(m0, b, ch)
    assert not (want["status"] == X.OK).any() and (want["status"] == X.NO_ROUTE).any()
    X.check(e.lookup(b, ch), want, "empty table")
    X.check(e.lookup_keys(X.keys_of(probes[:50])), X.expect_probes(m0, probes[:50]), "empty table keys")


def test_lookup_refusals():
    routes, probes, model, _ = X.cached("random")
    h = handle("random")
    b, ch = X.batch_case(X.probe_items(probes[:16]), 96)
    rc, got, (pb, pc, keep, cols) = raw_batch(h, b, ch)
    assert rc == 0
    huge = _lib.PktBatch(pb.slab, pb.slab_len, None, None, 96, 0, 1 << 32)
    no_slab = _lib.PktBatch(None, pb.slab_len, None, None, 96, 0, 16)
    stride0 = _lib.PktBatch(pb.slab, pb.slab_len, None, None, 0, 0, 16)
    four = np.zeros(4, np.uint64)
    no_lens = _lib.PktBatch(pb.slab, pb.slab_len, four.ctypes.data, None, 0, 0, 4)
    no_col = _lib.PktChain(pc.n_hdrs, None, pc.hdr_off)
    bad = [({1: None}, "null argument"), ({2: None}, "null argument"), ({2: ctypes.byref(no_col)}, "null chain column"),
           ({1: ctypes.byref(huge)}, "n >= 2^32"), ({1: ctypes.byref(no_slab)}, "null slab"),
           ({1: ctypes.byref(stride0)}, "stride 0"), ({1: ctypes.byref(no_lens)}, "offsets without lens"),
           ({3: 16}, "which_ip"), ({3: 0xFE}, "which_ip"), ({4: 2}, "unknown flag bits"), ({4: 0x80000001}, "unknown flag bits")]
    for r, text in bad:
        rc, out, _ = raw_batch(h, b, ch, r)
        assert rc == INVALID, sorted(r)
        assert err(h).startswith("pkt_lpm_lookup_batch: ") and text in err(h), (sorted(r), err(h))
        assert all((x == 0x77).all() for x in out.values()), sorted(r)
    assert raw_batch(h, b, ch, {3: 15})[0] == 0 and raw_batch(h, b, ch, {0: None})[0] == INVALID
    keys = X.keys_of(probes[:16])
    odd = np.zeros(16 * 40 + 1, np.uint8)
    for r, text in [({3: 1 << 32}, "n >= 2^32"), ({4: 2}, "unknown flag bits"), ({1: None}, "null keys"),
                    ({1: odd.ctypes.data + 1}, "keys not 2-byte aligned")]:
        rc, out, _ = raw_keys(h, keys, r=r)
        assert rc == INVALID, sorted(r)
        assert err(h).startswith("pkt_lpm_lookup_keys: ") and text in err(h), (sorted(r), err(h))
        assert all((x == 0x77).all() for x in out.values()), sorted(r)
    assert raw_keys(h, keys, r={0: None})[0] == INVALID
    # keys at a 2-byte boundary are taken
    shifted = np.zeros(16 * 40 + 2, np.uint8)
    shifted[2:] = keys.reshape(-1)
    rc, out, _ = raw_keys(h, keys, r={1: shifted.ctypes.data + 2})
    assert rc == 0
    X.check(out, X.expect_probes(model, probes[:16]), "2-byte aligned keys")


# ------------------------------------------------------------------ create
def create_raw(arr, n=None, max_bytes=0, null_routes=False):
    L = _lib.load()
    arr = np.ascontiguousarray(arr)
    h = ctypes.c_void_p()
    rc = L.pkt_lpm_create_host(None if null_routes else arr.ctypes.data, arr.size if n is None else n, 0, max_bytes, ctypes.byref(h))
    text = L.pkt_lpm_last_error(None).decode()
    if rc == 0:
        L.pkt_lpm_destroy(h)
    else:
        assert not h.value
    return rc, text


def test_create_refusals():
    good = X.to_array([(4, 24, X.ip4("10.1.2.0"), 1), (6, 48, X.ip6("2001:db8:1::"), 2), (4, 8, X.ip4("10.0.0.0"), 3)])
    assert create_raw(good)[0] == 0

    def changed(i, **kw):
        a = good.copy()
        for k, v in kw.items():
            a[k][i] = v
        return a

    v4_tail = good.copy()
    v4_tail["addr"][0, 9] = 1
    host_bit4 = good.copy()
    host_bit4["addr"][0, 3] = 1
    partial = changed(2, plen=9)
    partial["addr"][2, 1] = 0x40  # bit 9 of a /9
    host_bit6 = good.copy()
    host_bit6["addr"][1, 15] = 0x80
    dup = np.concatenate([good, good[1:2]])
    dup["nexthop"][3] = 99
    same_prefix_other_len = np.concatenate([good, changed(0, plen=23)[0:1]])  # 10.1.2.0/23 beside 10.1.2.0/24: legal
    assert create_raw(same_prefix_other_len)[0] == 0
    cases = [(changed(1, ipver=5), "ipver"), (changed(0, ipver=0), "ipver"), (changed(0, plen=33), "plen above"),
             (changed(1, plen=129), "plen above"), (changed(2, zero=1), "zero"), (v4_tail, "address bit"),
             (host_bit4, "address bit"), (partial, "address bit"), (host_bit6, "address bit"), (dup, "same (ipver, plen, prefix)")]
    for arr, text in cases:
        rc, msg = create_raw(arr)
        assert rc == INVALID and msg.startswith("pkt_lpm") and text in msg, (text, rc, msg)
    rc, msg = create_raw(good, null_routes=True)
    assert rc == INVALID and msg.startswith("pkt_lpm") and "null routes" in msg
    rc, msg = create_raw(good, n=(1 << 24) + 1)
    assert rc == INVALID and msg.startswith("pkt_lpm") and "PKT_LPM_MAX_ROUTES" in msg
    assert create_raw(good, n=0, null_routes=True)[0] == 0
    assert _lib.load().pkt_lpm_create_host(good.ctypes.data, 3, 0, 0, None) == INVALID
    with pytest.raises(ValueError, match="pkt_lpm"):
        host(dup)


def test_max_bytes():
    routes = [(4, 24, (10 << 24) | (k << 16) | (3 << 8), k) for k in range(5)]
    need = 2 * 4 * 65536 + 5 * 1024 + 5 * 8
    assert host(routes).info()["bytes"] == need
    assert create_raw(X.to_array(routes), max_bytes=need)[0] == 0
    rc, msg = create_raw(X.to_array(routes), max_bytes=need - 1)
    assert rc == UNSUPPORTED and msg.startswith("pkt_lpm") and str(need) in msg, msg
    rc, msg = create_raw(X.to_array([]), max_bytes=1000)
    assert rc == UNSUPPORTED and str(2 * 4 * 65536) in msg


def test_info_counts():
    """Disjoint /24s in k distinct /16s need k nodes; a /32 below one of them one more; an IPv6 /128 alone 14."""
    rng = np.random.default_rng(11)
    tops = rng.permutation(1 << 16)[:37]
    routes = [(4, 24, int(t) << 16 | int(c) << 8, 1) for t in tops for c in rng.permutation(256)[:9]]
    i = host(routes).info()
    assert (i["routes_v4"], i["nodes_v4"], i["depth_v4"], i["routes_v6"], i["nodes_v6"], i["depth_v6"]) == (37 * 9, 37, 2, 0, 0, 0)
    assert i["bytes"] == 2 * 4 * 65536 + 37 * 1024 + 37 * 9 * 8
    routes.append((4, 32, routes[0][2] | 5, 2))
    routes.append((6, 128, X.ip6("2001:db8::1"), 3))
    routes.append((6, 16, X.ip6("2001::"), 4))
    i = host(routes).info()
    assert (i["nodes_v4"], i["depth_v4"], i["routes_v6"], i["nodes_v6"], i["depth_v6"]) == (38, 3, 2, 14, 15)
    for L, depth in ((0, 1), (16, 1), (17, 2), (24, 2), (25, 3), (32, 3)):
        assert host([(4, L, X.mask(4, L, X.A4), 1)]).info()["depth_v4"] == depth
    for L, depth in ((16, 1), (17, 2), (64, 7), (65, 8), (120, 14), (121, 15), (128, 15)):
        i = host([(6, L, X.mask(6, L, X.A6), 1)]).info()
        assert (i["depth_v6"], i["nodes_v6"]) == (depth, depth - 1)
