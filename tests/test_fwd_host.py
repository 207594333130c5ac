"""pkt_fwd_host and the host form of Forwarder (Parser.forwarder(host=True) / pktgpu.Forwarder(None, adj)) against
fwd_cases' yardstick, an independent Python model written from the text of include/pktgpu.h.  pkt_fwd_host runs the
decision, the checksum arithmetic and the refusals the kernel shares (pktgpu_fwd.hpp), so this file covers them for
both.  No device."""
import ctypes

import numpy as np
import pytest

import pktgpu
from pktgpu import _lib, schema

import l4_cases as L4
import lpm_cases as X
import fwd_cases as W

INVALID = -1


def run(c, b, chain, write=True, outputs=W.NAMES, hits=True, bytes=True, lpm=None, nexthop="case"):
    """Forwarder(None, adj).run over a copy of the batch -> the result dict with the slab after the call."""
    b = dict(b, slab=b["slab"].copy())
    nexthop = c["nexthop"] if isinstance(nexthop, str) else nexthop
    f = pktgpu.Forwarder(None, W.adj_array(c["adj"]))
    got = f.run(b, chain, nexthop=None if lpm is not None else nexthop, lpm=lpm, which_ip=c["which"], keep_l2=c["keep_l2"],
                write=write, select=c["select"], outputs=outputs, hits=hits, bytes=bytes)
    got["slab"] = b["slab"]
    return got


def host_lpm(c):
    return pktgpu.Lpm(None, X.to_array(c["routes"]), W.LPM_DEFAULT)


def test_sizes_and_constants():
    L = _lib.load()
    assert L.pkt_sizeof_fwd_adj() == 20 == ctypes.sizeof(_lib.PktFwdAdj) == schema.FWD_ADJ_DTYPE.itemsize
    assert _lib.PktFwdAdj.port.offset == 12 and _lib.PktFwdAdj.mtu.offset == 16 and _lib.PktFwdAdj.action.offset == 18
    assert (pktgpu.FWD_OK, pktgpu.FWD_SKIPPED, pktgpu.FWD_NO_IP, pktgpu.FWD_SPAN, pktgpu.FWD_NO_ETHER, pktgpu.FWD_TTL,
            pktgpu.FWD_NO_ADJ, pktgpu.FWD_DROP, pktgpu.FWD_PUNT, pktgpu.FWD_MTU) == tuple(range(10))
    assert schema.FWD_STATUS_COUNT == len(schema.FWD_STATUS) == 10 and pktgpu.FWD_NONE == 0xFFFFFFFF
    assert (schema.FWD_KEEP_L2, schema.FWD_NO_WRITE, schema.FWD_MAX_ADJ) == (1, 2, 1 << 20)
    assert (schema.FWD_ACT_FORWARD, schema.FWD_ACT_DROP, schema.FWD_ACT_PUNT) == (0, 1, 2)


def test_the_model_pins_the_named_cases():
    """On the model alone: every named case gives the statuses its name promises, in the capture layout."""
    for name in W.NAMED:
        c, want = W.named_cached()[name]
        b, ch = W.layout(c, "indexed")
        e = W.expect(c, b, ch)
        assert list(e["status"]) == want, name
        changed = np.flatnonzero(e["slab"] != b["slab"]).size
        assert (changed > 0) == (W.OK in want), name
    c, _ = W.named_cached()["vxlan_inner"]
    b, ch = W.layout(c, "indexed")
    e = W.expect(c, b, ch)
    off = int(b["offsets"][0])
    inner_eth = [o for t, o in c["items"][0][1] if t == W.T_ETHER][1]
    assert np.array_equal(e["slab"][off:off + inner_eth], b["slab"][off:off + inner_eth])  # the outer packet is untouched
    assert e["slab"][off + inner_eth:off + inner_eth + 12].tobytes() == c["adj"][1][0] + c["adj"][1][1]


@pytest.mark.parametrize("layout", W.LAYOUTS)
@pytest.mark.parametrize("name", W.NAMED)
def test_named_cases(name, layout):
    c, _ = W.named_cached()[name]
    b, ch = W.layout(c, layout)
    W.check(run(c, b, ch), W.expect(c, b, ch), f"{name} {layout}")


@pytest.mark.parametrize("layout", W.LAYOUTS)
def test_random_mix(layout):
    c = W.mix_cached()
    b, ch = W.layout(c, layout)
    want = W.expect(c, b, ch)
    if layout == "indexed":
        W.assert_mix(want, b, ch)  # on the model alone, before any comparison
    W.check(run(c, b, ch), want, f"mix {layout}")


def test_checksum_is_the_incremental_update():
    """Every OK IPv4 packet whose checksum was RFC 1071-valid before the call holds, after it, the plain RFC 1071
    checksum of the rewritten header (the sum is written out here: 16-bit big-endian words, end-around carry, the
    complement; it is not Packet::ipv4_checksum).  A checksum that was wrong stays wrong by the formula's amount."""
    def plain(hdr):
        hdr = [int(x) for x in hdr]
        s = 0
        for k in range(0, 20, 2):
            if k != 10:
                s += hdr[k] << 8 | hdr[k + 1]
        while s >> 16:
            s = (s & 0xFFFF) + (s >> 16)
        return ~s & 0xFFFF

    c = W.mix_cached()
    b, ch = W.layout(c, "indexed")
    got = run(c, b, ch)
    valid = wrong = 0
    for i in np.flatnonzero(got["status"] == W.OK):
        hdrs = c["items"][i][1]
        t, o = X.ip_slots(hdrs)[0]
        if t != W.T_IPV4:
            continue
        at = int(b["offsets"][i]) + o
        before, after = b["slab"][at:at + 20], got["slab"][at:at + 20]
        assert int(after[8]) == int(before[8]) - 1 and np.array_equal(np.delete(after, [8, 10, 11]), np.delete(before, [8, 10, 11]))
        new = int(after[10]) << 8 | int(after[11])
        if plain(before) == (int(before[10]) << 8 | int(before[11])):
            assert new == plain(after), i
            valid += 1
        else:
            assert new != plain(after) and new == W.csum_1624(int(before[10]) << 8 | int(before[11]), int(before[8]) << 8 | int(before[9])), i
            wrong += 1
    assert valid > 300 and wrong > 50
    # one header with a deliberately wrong checksum: the new value is the formula's
    p, hdrs = W.v4(ttl=17)
    q = bytearray(p)
    q[24:26] = b"\xBE\xEF"
    one = W.case([(bytes(q), hdrs)])
    b, ch = W.layout(one, "indexed")
    got = run(one, b, ch)
    at = int(b["offsets"][0]) + 14
    assert got["status"][0] == W.OK and got["slab"][at + 8] == 16
    assert (int(got["slab"][at + 10]) << 8 | int(got["slab"][at + 11])) == W.csum_1624(0xBEEF, 17 << 8 | 17)
    # the extremes of the fold: m' = 0xFFxx - 0x100 with HC 0x0000 / 0xFFFF
    for hc in (0x0000, 0xFFFF, 0x0100, 0xFEFF):
        for ttl, proto in ((255, 255), (2, 0), (128, 6)):
            q = bytearray(p)
            q[22], q[23], q[24], q[25] = ttl, proto, hc >> 8, hc & 0xFF
            one = W.case([(bytes(q), hdrs)])
            b, ch = W.layout(one, "s64_lens")
            W.check(run(one, b, ch), W.expect(one, b, ch), f"hc {hc:#x} ttl {ttl}")


def test_no_write_and_keep_l2():
    c = W.mix_cached()
    b, ch = W.layout(c, "indexed")
    want = W.expect(c, b, ch)
    got = run(c, b, ch, write=False)
    assert np.array_equal(got["slab"], b["slab"])
    W.check({k: got[k] for k in W.NAMES + ("hits", "bytes")}, want, "NO_WRITE")
    k = dict(c, keep_l2=True)
    want = W.expect(k, b, ch)
    got = run(k, b, ch)
    W.check(got, want, "KEEP_L2")
    assert (want["status"] == W.NO_ETHER).sum() == 0 and (want["status"] == W.OK).sum() > 1000
    for i in np.flatnonzero(want["status"] == W.OK):  # no MAC is written
        at = int(b["offsets"][i])
        assert np.array_equal(got["slab"][at:at + 12], b["slab"][at:at + 12])


def test_counters_accumulate():
    c = W.mix_cached()
    b, ch = W.layout(c, "s64_lens")
    want = W.expect(c, b, ch)
    f = pktgpu.Forwarder(None, W.adj_array(c["adj"]))
    hits, byts = np.zeros(10, np.uint64), np.zeros(10, np.uint64)
    for k in range(2):
        r = f.run(dict(b, slab=b["slab"].copy()), ch, nexthop=c["nexthop"], select=c["select"], hits=hits, bytes=byts)
        assert r["hits"] is hits and int(hits.sum()) == (k + 1) * b["n"]
    assert np.array_equal(hits, 2 * want["hits"]) and np.array_equal(byts, 2 * want["bytes"])
    e = f.run(dict(b, slab=b["slab"].copy(), n=0, lens=b["lens"][:0]), ch, nexthop=c["nexthop"][:0], hits=hits, bytes=byts)
    assert e["status"].size == 0 and int(hits.sum()) == 2 * b["n"]


def raw(c, b, chain, r=(), outputs=(True,) * 5, flags=0, lpm=None, adj="case", nadj=None):
    """pkt_fwd_host with argument positions replaced -> (rc, outputs, slab after, keep)."""
    L = _lib.load()
    b = dict(b, slab=b["slab"].copy())
    pb, keep = pktgpu._host_batch(_lib, b)
    cols = [np.ascontiguousarray(chain[k]) for k in ("n_hdrs", "hdr_type", "hdr_off")]
    pc = _lib.PktChain(*[x.ctypes.data for x in cols])
    arr = W.adj_array(c["adj"]) if isinstance(adj, str) else adj
    dts = (np.uint8, np.uint32, np.uint32, np.uint64, np.uint64)
    sizes = (pb.n, pb.n, pb.n, 10, 10)
    out = [np.full(k * np.dtype(dt).itemsize, 0x77, np.uint8).view(dt) if w else None for k, dt, w in zip(sizes, dts, outputs)]
    nh = None if lpm is not None else c["nexthop"]
    sel = c["select"]
    a = [arr.ctypes.data if arr is not None and arr.size else None, (arr.size if arr is not None else 0) if nadj is None else nadj,
         ctypes.byref(pb), ctypes.byref(pc), c["which"], flags | (1 if c["keep_l2"] else 0), None if lpm is None else lpm._t,
         None if nh is None else nh.ctypes.data, None if sel is None else sel.ctypes.data,
         *[None if x is None else x.ctypes.data for x in out]]
    for k, v in dict(r).items():
        a[k] = v
    rc = L.pkt_fwd_host(*a)
    return rc, dict(zip(W.NAMES + ("hits", "bytes"), out)), b["slab"], (pb, pc, keep, cols, arr, nh, sel)


def test_null_outputs():
    c = W.head(W.mix_cached(), 300)
    b, ch = W.layout(c, "indexed")
    want = W.expect(c, b, ch)
    for mask in range(32):
        outputs = tuple(bool(mask >> k & 1) for k in range(5))
        rc, got, slab, _ = raw(c, b, ch, outputs=outputs)
        assert rc == 0, mask
        for k, name in enumerate(("hits", "bytes")):  # added to 0x77..77
            if got[name] is not None:
                got[name] = got[name] - np.uint64(0x7777777777777777)
        W.check(dict(got, slab=slab), want, f"outputs {outputs}")
        rc, got, slab, _ = raw(c, b, ch, outputs=outputs, flags=schema.FWD_NO_WRITE)
        assert rc == 0 and np.array_equal(slab, b["slab"])


def test_fused_lpm_equals_lookup_then_run():
    for name, kind in (("boundary", "probe"), ("short_after_long", "probe"), ("random", "probe"), ("random", "vxlan")):
        c = W.fused(name, kind)
        lpm = host_lpm(c)
        for layout in ("indexed", "s128_lens"):
            b, ch = W.layout(c, layout)
            want = W.expect(c, b, ch)
            fused = run(c, b, ch, lpm=lpm)
            W.check(fused, want, f"fused {name} {kind} {layout}")
            nh = lpm.lookup(b, ch, which_ip=c["which"], outputs=("nexthop",))["nexthop"]
            pair = run(c, b, ch, nexthop=nh)
            W.check(pair, want, f"unfused {name} {kind} {layout}")
            assert all(np.array_equal(fused[k], pair[k]) for k in W.NAMES + ("hits", "bytes", "slab"))
        assert {W.OK, W.NO_ADJ, W.DROP, W.PUNT, W.MTU} <= set(np.unique(want["status"])), (name, kind)


def test_refusals():
    c = W.head(W.mix_cached(), 16)
    b, ch = W.layout(c, "s64_lens")
    rc, got, slab, (pb, pc, keep, cols, arr, nh, sel) = raw(c, b, ch)
    assert rc == 0
    huge = _lib.PktBatch(pb.slab, pb.slab_len, None, None, 64, 0, 1 << 32)
    no_slab = _lib.PktBatch(None, pb.slab_len, None, None, 64, 0, 16)
    stride0 = _lib.PktBatch(pb.slab, pb.slab_len, None, None, 0, 0, 16)
    four = np.zeros(4, np.uint64)
    no_lens = _lib.PktBatch(pb.slab, pb.slab_len, four.ctypes.data, None, 0, 0, 4)
    no_col = _lib.PktChain(pc.n_hdrs, None, pc.hdr_off)
    odd = np.zeros(11, np.uint64)
    routes = [(4, 8, X.ip4("10.0.0.0"), 1)]
    lpm = pktgpu.Lpm(None, X.to_array(routes), 0)
    bad = [{2: None}, {3: None}, {3: ctypes.byref(no_col)}, {2: ctypes.byref(huge)}, {2: ctypes.byref(no_slab)},
           {2: ctypes.byref(stride0)}, {2: ctypes.byref(no_lens)}, {4: 16}, {4: 0xFE}, {5: 4}, {5: 0x80000001},
           {6: lpm._t}, {7: None}, {12: odd.ctypes.data + 4}, {13: odd.ctypes.data + 1}]
    for r in bad:
        rc, out, slab, _ = raw(c, b, ch, r)
        assert rc == INVALID, sorted(r)
        assert all((x.view(np.uint8) == 0x77).all() for x in out.values()) and np.array_equal(slab, b["slab"]), sorted(r)
    assert raw(c, b, ch, {4: 15})[0] == 0
    # the create refusals, which the host call makes on its adjacency array
    good = W.adj_array(c["adj"])
    act, zero = good.copy(), good.copy()
    act["action"][3] = 3
    zero["zero"][5] = 1
    for kw in (dict(adj=act), dict(adj=zero), dict(nadj=(1 << 20) + 1), dict(r={0: None})):
        rc, out, slab, _ = raw(c, b, ch, **kw)
        assert rc == INVALID and all((x.view(np.uint8) == 0x77).all() for x in out.values()), kw
    assert raw(c, b, ch, nadj=0, r={0: None})[0] == 0  # nadj == 0 is legal
    # the Python form names the call in what it raises
    with pytest.raises(ValueError, match="^pkt_fwd_host failed"):
        pktgpu.Forwarder(None, act).run(dict(b, slab=b["slab"].copy()), ch, nexthop=c["nexthop"])
    with pytest.raises(ValueError):
        pktgpu.Forwarder(None, good).run(dict(b, slab=b["slab"].copy()), ch, nexthop=c["nexthop"], outputs=("rank",))
    with pytest.raises(ValueError):
        pktgpu.fwd_adjacencies([("00:01:02:03:04", "00:01:02:03:04:05", 1)])


def test_python_forms():
    """Adjacencies as tuples with MAC strings or bytes, Parser-less host form, close() twice."""
    adj = [("02:00:00:00:00:01", "02:00:00:00:00:fe", 3), (b"\x02\0\0\0\0\x02", bytes(6), 9, 1500), (bytes(6), bytes(6), 1, 0, schema.FWD_ACT_PUNT)]
    arr = pktgpu.fwd_adjacencies(adj)
    assert arr.dtype == schema.FWD_ADJ_DTYPE and arr["dmac"][0].tobytes() == bytes([2, 0, 0, 0, 0, 1]) and arr["smac"][0][5] == 0xFE
    assert list(arr["port"]) == [3, 9, 1] and list(arr["mtu"]) == [0, 1500, 0] and list(arr["action"]) == [0, 0, 2]
    c = W.case([W.v4(), W.v6(), W.v4()], nexthop=[0, 1, 2], adj=[(bytes(a["dmac"]), bytes(a["smac"]), int(a["port"]), int(a["mtu"]), int(a["action"])) for a in arr])
    b, ch = W.layout(c, "indexed")
    f = pktgpu.Forwarder(None, adj)
    b2 = dict(b, slab=b["slab"].copy())
    r = f.run((b2["slab"], b2["offsets"], b2["lens"]), ch, nexthop=c["nexthop"], hits=True)
    assert all(isinstance(v, np.ndarray) for v in r.values()) and set(r) == {"status", "port", "adj_index", "hits"}
    W.check(dict(r, slab=b2["slab"]), W.expect(c, b, ch), "tuple batch")
    assert list(r["status"]) == [W.OK, W.OK, W.PUNT] and list(r["port"]) == [3, 9, W.NONE]
    f.close()
    f.close()
