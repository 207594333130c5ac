"""pkt_frag_host (the CPU twin of pktgpu_frag.hip: the decision, the fragment header and the refusals of
pktgpu_frag.hpp, which the kernels share) against frag_cases' yardstick, an independent Python model written from the
text of include/pktgpu.h, and against properties that need no model."""
import ctypes

import numpy as np
import pytest

import pktgpu
from pktgpu import schema

import frag_cases as G

INVALID = -1
# argument positions of pkt_frag_host
A_BATCH, A_CHAIN, A_WHICH, A_FLAGS, A_MTU, A_MTU_ALL, A_SELECT, A_STATUS, A_NFRAG, A_FIRST, A_DST, A_DST_LEN, A_CAP, A_OFF, \
    A_LEN, A_SRC, A_FRAG, A_OCHAIN, A_HITS = range(19)


def run(items, mtu, select=None, which=0, flags=0, kind="indexed", **kw):
    b, ch = G.layout(items, kind)
    want = G.expect(b, ch, mtu, select, which, flags)
    rc, got = G.host_call(b, ch, mtu, select, which, flags, **kw)
    return rc, got, want, b, ch


def outputs(got):
    """[(bytes, src, frag)] of a call's outputs."""
    return [(got["dst"][int(o):int(o) + int(ln)].tobytes(), int(s), int(f)) for o, ln, s, f in
            zip(got["out_off"][:got["n_out"]], got["out_len"], got["src_index"], got["frag_index"])]


# ------------------------------------------------------------------ 1. RFC 791's example
def test_rfc791_example_known_answer():
    """A 472-byte datagram (452 data bytes) at MTU 280: two fragments of total length 276 and 216 at offsets 0 and 32,
    more-fragments 1 and 0 (per = 256, 452 = 256 + 196)."""
    item = G.v4(452)
    assert G.be16(item[0], 16) == 472
    rc, got, want, _, _ = run([item], 280)
    assert rc == 0 and got["guards"]
    assert got["status"].tolist() == [G.SPLIT] and got["nfrag"].tolist() == [2] and got["first"].tolist() == [0]
    outs = outputs(got)
    assert [(G.be16(p, 16), G.be16(p, 20) & 0x1FFF, G.be16(p, 20) >> 13 & 1) for p, _, _ in outs] == [(276, 0, 1), (216, 32, 0)]
    assert [len(p) for p, _, _ in outs] == [14 + 276, 14 + 216]
    assert outs[0][0][34:] + outs[1][0][34:] == item[0][34:]
    assert got["n_out"] == 2 and got["bytes_out"] == G.r16(290) + G.r16(230)
    assert got["out_off"].tolist() == [0, G.r16(290)]
    G.check(got, want, got["cap"])


# ------------------------------------------------------------------ 2. properties, without the model
def property_items():
    return [G.v4(452), G.v4(1466), G.v4(3000, vlan=True, pad=3), G.v4(999, w=0x2000 | 100), G.v4(64, w=7),
            G.vxlan(1400), G.corrupt(G.v4(1000)), G.corrupt(G.v4(777, vlan=True), 0x1FF), G.v4(8 * 50), G.v4(8 * 50 + 1)]


@pytest.mark.parametrize("m", [28, 68, 69, 576, 1500])
@pytest.mark.parametrize("which", [0, G.LAST])
def test_properties_of_split_packets(m, which):
    items = property_items()
    b, ch = G.layout(items)
    rc, got = G.host_call(b, ch, m, which=which)
    assert rc == 0 and got["guards"]
    outs = outputs(got)
    nsplit = 0
    for i, (p, hdrs) in enumerate(items):
        if got["status"][i] != G.SPLIT:
            continue
        nsplit += 1
        ips = [o for t, o in hdrs if t == G.T_IPV4]
        ip = ips[-1] if which == G.LAST else ips[0]
        L = G.be16(p, ip + 2)
        mine = [x for x in outs if x[1] == i]
        assert [f for _, _, f in mine] == list(range(len(mine))) and len(mine) == got["nfrag"][i] >= 2
        assert b"".join(q[ip + 20:] for q, _, _ in mine) == p[ip + 20:ip + L]
        src_sum = G.rfc1071(p[ip:ip + 20])
        w = G.be16(p, ip + 6)
        at = w & 0x1FFF
        for j, (q, _, _) in enumerate(mine):
            pay = len(q) - ip - 20
            assert G.be16(q, ip + 2) == 20 + pay
            if j < len(mine) - 1:
                assert pay % 8 == 0 and pay > 0 and 20 + pay <= m
                assert G.be16(q, ip + 6) & 0x2000
            else:
                assert 0 < 20 + pay <= m and G.be16(q, ip + 6) & 0x2000 == w & 0x2000
            assert G.be16(q, ip + 6) & 0x1FFF == at and G.be16(q, ip + 6) & 0xC000 == w & 0xC000
            at += pay // 8
            assert q[:ip] == p[:ip]
            for k in (0, 1, 4, 5, 8, 9, 12, 13, 14, 15, 16, 17, 18, 19):
                assert q[ip + k] == p[ip + k]
            # RFC 1071: a header that summed to 0xFFFF still does; one that was off stays off by as much
            assert G.rfc1071(q[ip:ip + 20]) == src_sum
    assert nsplit >= (5 if m <= 576 else 1)
    assert G.rfc1071(items[0][0][14:34]) == 0xFFFF and G.rfc1071(items[6][0][14:34]) != 0xFFFF


# ------------------------------------------------------------------ 3. every status, and the order of the tests
def status_cases():
    """name -> (items, mtu, kwargs, the statuses wanted)."""
    S = G
    t = {}
    a = G.v4(1000)
    t["every_status"] = ([a, a, a, (a[0], [(G.T_ETHER, 0)]), (a[0][:30], a[1]), G.v6(1000), G.v4(1000, b0=0x46), (a[0][:900], a[1]),
                          G.v4(1000, w=0x4000), a],
                         np.asarray([1500, 576, 576, 576, 576, 576, 576, 576, 576, 27], np.uint16),
                         dict(select=np.asarray([1, 1, 0, 1, 1, 1, 1, 1, 1, 1], np.uint8)),
                         [S.FITS, S.SPLIT, S.SKIPPED, S.NO_IP, S.SPAN, S.IPV6, S.BAD_HDR, S.TRUNC, S.DF, S.MTU])
    # several things at once: the first test that applies
    df46 = G.v4(1000, w=0x4000, b0=0x46)
    t["order"] = ([df46, df46, (df46[0][:900], df46[1]), (G.v4(1000, w=0x4000)[0][:900], a[1]), G.v4(1000, w=0x4000),
                   G.v4(1000, b0=0x65), (G.v6(1000)[0][:50], G.v6(1000)[1]), (G.v6(1000)[0][:100], G.v6(1000)[1])],
                  np.asarray([2000, 100, 100, 100, 20, 0, 100, 100], np.uint16), {},
                  [S.FITS, S.BAD_HDR, S.BAD_HDR, S.TRUNC, S.DF, S.FITS, S.SPAN, S.IPV6])
    # byte 0; L < 20 (above an mtu of 10); the last offset: 7 * 69 = 483 more eighths, 8191 - 483 = 0x1E1C
    t["bad_hdr_causes"] = ([G.v4(1000, b0=0x46), G.v4(1000, b0=0x55), G.v4(100, L=19), G.v4(4000, w=0x1FF0), G.v4(4000, w=0x1E1C),
                            G.v4(4000, w=0x1E1D)], np.asarray([576, 576, 10, 576, 576, 576], np.uint16), {},
                           [S.BAD_HDR, S.BAD_HDR, S.BAD_HDR, S.BAD_HDR, S.SPLIT, S.BAD_HDR])
    t["fragment_of_fragment"] = ([G.v4(1000, w=0x2000 | 185), G.v4(1000, w=185), G.v4(1000, w=0x8000 | 185)], 576, {}, [S.SPLIT] * 3)
    t["mtu_28_and_0"] = ([G.v4(100), G.v4(9), G.v4(8), G.v4(5000), G.v4(100)], np.asarray([28, 28, 28, 0, 27], np.uint16), {},
                         [S.SPLIT, S.SPLIT, S.FITS, S.FITS, S.MTU])
    t["L_at_the_mtu"] = ([G.v4(556), G.v4(557), G.v4(555)], 576, {}, [S.FITS, S.SPLIT, S.FITS])
    t["P_multiple_of_per"] = ([G.v4(552 * 2), G.v4(552 * 2 + 1), G.v4(552 * 3)], 576, {}, [S.SPLIT] * 3)
    # 65535 bytes: L = 65521, 8188 fragments, the last one 8187 eighths on
    t["max_packet"] = ([G.v4(65535 - 34), G.v4(65535 - 34, w=4), G.v4(65535 - 34, w=5), G.v4(65535 - 34, w=0x2000 | 9)], 28, {},
                       [S.SPLIT, S.SPLIT, S.BAD_HDR, S.BAD_HDR])
    t["ipv6"] = ([G.v6(100), G.v6(1461), G.v6(1460)], 1500, {}, [S.FITS, S.IPV6, S.FITS])
    vl, vx = G.v4(1000, vlan=True), G.vxlan(1000)
    for which in (0, 1, G.LAST):
        t[f"vlan_vxlan_which_{which}"] = ([vl, vx, G.v4(100, vlan=True), vx], np.asarray([576, 576, 576, 1060], np.uint16), dict(which=which),
                                         [S.NO_IP if which == 1 else S.SPLIT, S.SPLIT, S.NO_IP if which == 1 else S.FITS,
                                          S.SPLIT if which == 0 else S.FITS])
    t["padding"] = ([G.v4(1000, pad=7), G.v4(30, pad=16), G.v4(1000, vlan=True, pad=1)], 576, {}, [S.SPLIT, S.FITS, S.SPLIT])
    return t


STATUS_CASES = sorted(status_cases())


@pytest.mark.parametrize("kind", ["indexed", "stride"])
@pytest.mark.parametrize("name", STATUS_CASES)
def test_status_cases(name, kind):
    items, mtu, kw, statuses = G.cached("status_cases", status_cases)[name]
    rc, got, want, _, _ = run(items, mtu, kind=kind, **kw)
    assert rc == 0 and got["guards"]
    assert want["status"].tolist() == statuses, (name, "the model", want["status"].tolist())
    G.check(got, want, got["cap"], name)
    if name == "padding":  # the bytes past ip_off + L go nowhere; a FITS output keeps them
        assert got["out_len"][:5].tolist() == [14 + 20 + 552, 14 + 20 + 448, 14 + 50 + 16, 18 + 20 + 552, 18 + 20 + 448]
    if name == "fragment_of_fragment":
        o = outputs(got)
        assert [G.be16(p, 20) for p, _, _ in o] == [0x2000 | 185, 0x2000 | 254, 0x2000 | 185, 254, 0xA000 | 185, 0x8000 | 254]


# ------------------------------------------------------------------ 4. call-level behaviour
def mixed():
    return G.cached("mix600", lambda: G.mix(600, big=False))


def test_mix_against_the_model_with_select_and_per_packet_mtu():
    items, mtu, sel = mixed()
    rc, got, want, _, _ = run(items, mtu, sel)
    assert rc == 0 and got["guards"]
    counts = np.bincount(want["status"], minlength=G.NSTATUS)
    assert all(counts[s] >= 3 for s in (G.FITS, G.SPLIT, G.SKIPPED, G.NO_IP, G.IPV6, G.DF)), counts
    G.check(got, want, got["cap"], "mix")
    assert int(got["hits"].sum()) == len(items)


def test_mtu_all_is_the_per_packet_array_with_one_value():
    items, _, sel = mixed()
    b, ch = G.layout(items)
    rc1, g1 = G.host_call(b, ch, 576, sel)
    rc2, g2 = G.host_call(b, ch, np.full(len(items), 576, np.uint16), sel)
    assert rc1 == rc2 == 0
    for k in g1:
        assert np.array_equal(g1[k], g2[k]), k
    G.check(g1, G.expect(b, ch, 576, sel), g1["cap"])


def test_only_split_and_no_write_totals():
    items, mtu, sel = mixed()
    for flags in (0, G.ONLY_SPLIT):
        rc, got, want, b, ch = run(items, mtu, sel, flags=flags)
        assert rc == 0
        G.check(got, want, got["cap"], f"flags {flags}")
        rc, plan = G.host_call(b, ch, mtu, sel, flags=flags | G.NO_WRITE)
        assert rc == 0 and plan["guards"] and "dst" not in plan
        assert (plan["n_out"], plan["bytes_out"]) == (got["n_out"], got["bytes_out"])
        for k in ("status", "nfrag", "first", "hits"):
            assert np.array_equal(plan[k], got[k]), k
    assert (want["nfrag"][want["status"] == G.FITS] == 0).all()


NULLABLE = ["status", "nfrag", "first", "src_index", "frag_index", "oc_n_hdrs", "oc_hdr_type", "oc_hdr_off", "hits"]


@pytest.mark.parametrize("mask", list(range(0, 512, 37)) + [511])
def test_null_output_combinations(mask):
    items, mtu, sel = G.cached("mix150", lambda: G.mix(150, seed=5, big=False))
    skip = [k for j, k in enumerate(NULLABLE) if mask >> j & 1]
    rc, got, want, _, _ = run(items, mtu, sel, skip=skip)
    assert rc == 0 and got["guards"]
    G.check(got, want, got["cap"], str(skip))


def test_every_null_output_alone():
    items, mtu, sel = G.cached("mix150", lambda: G.mix(150, seed=5, big=False))
    for k in NULLABLE:
        rc, got, want, _, _ = run(items, mtu, sel, skip=[k])
        assert rc == 0 and got["guards"], k
        G.check(got, want, got["cap"], k)


def test_empty_tail_up_to_out_cap_and_dst_untouched_past_the_total():
    items, mtu, sel = G.cached("mix150", lambda: G.mix(150, seed=5, big=False))
    b, ch = G.layout(items)
    want = G.expect(b, ch, mtu, sel)
    cap, room = want["n_out"] + 77, want["bytes_out"] + 4096
    rc, got = G.host_call(b, ch, mtu, sel, cap=cap, dst_len=room)
    assert rc == 0 and got["guards"]
    G.check(got, want, cap)
    assert (got["dst_rest"][want["bytes_out"]:] == 0xA5).all()


def test_overflow_returns_both_totals_for_each_cause():
    items, mtu, sel = G.cached("mix150", lambda: G.mix(150, seed=5, big=False))
    b, ch = G.layout(items)
    want = G.expect(b, ch, mtu, sel)
    for cap, room in ((want["n_out"] - 1, want["bytes_out"]), (want["n_out"], want["bytes_out"] - 1), (want["n_out"], want["bytes_out"] - 16)):
        rc, got = G.host_call(b, ch, mtu, sel, cap=cap, dst_len=room)
        assert rc == INVALID and got["guards"]
        assert (got["n_out"], got["bytes_out"]) == (want["n_out"], want["bytes_out"])
        for k in ("status", "nfrag", "hits"):
            assert np.array_equal(got[k], want[k]), k
    rc, got = G.host_call(b, ch, mtu, sel, cap=want["n_out"], dst_len=want["bytes_out"])
    assert rc == 0
    G.check(got, want, want["n_out"])


def test_a_count_above_out_cap_overflows_with_room_to_spare():
    """(n_out >= 2^32, the third cause, cannot be reached with the memory a test has: out_cap itself is below 2^32,
    so it is covered by n_out > out_cap in the shared predicate.)"""
    b, ch = G.layout([G.v4(100)] * 4)
    rc, got = G.host_call(b, ch, 28, cap=4 * 13 - 1, dst_len=1 << 20)
    assert rc == INVALID and got["n_out"] == 4 * 13 and got["guards"]


def test_n_out_of_2_pow_32_and_more_overflows_with_exact_totals():
    """The third cause: 524,417 batch entries that all point at one 65535-byte datagram (a source may be read more
    than once), 8190 fragments each at mtu 28: 2^32 + 5,254 outputs.  The totals come back whole, in 64 bits."""
    n = (1 << 32) // 8190 + 1
    p = G.ip4_hdr(65535) + G.pattern(65515, 1)
    b = dict(slab=np.frombuffer(p, np.uint8).copy(), offsets=np.zeros(n, np.uint64), lens=np.full(n, 65535, np.uint32), stride=None, n=n)
    ch = dict(n_hdrs=np.ones(n, np.uint8), hdr_type=np.zeros((G.MAXH, n), np.uint8), hdr_off=np.zeros((G.MAXH, n), np.uint16))
    ch["hdr_type"][0] = G.T_IPV4
    rc, got = G.host_call(b, ch, 28, cap=(1 << 32) - 1, dst_len=1 << 62, skip=["dst", "out_off", "out_len", "src_index", "frag_index",
                                                                             "oc_n_hdrs", "oc_hdr_type", "oc_hdr_off"],
                          over={A_DST: b["slab"].ctypes.data & ~15, A_OFF: ch["hdr_off"].ctypes.data & ~7, A_LEN: ch["hdr_off"].ctypes.data & ~7})
    assert rc == INVALID and got["guards"]
    assert got["n_out"] == n * 8190 >= 1 << 32 and got["bytes_out"] == n * 8190 * 32
    assert (got["status"] == G.SPLIT).all() and (got["nfrag"] == 8190).all() and got["hits"][G.SPLIT] == n


def test_n_0():
    b, ch = G.layout([G.v4(100)])
    b = dict(b, n=0, offsets=b["offsets"][:0], lens=b["lens"][:0])
    ch = {k: v[..., :0] for k, v in ch.items()}
    rc, got = G.host_call(b, ch, 576, cap=5, dst_len=64)
    assert rc == 0 and got["guards"] and (got["n_out"], got["bytes_out"]) == (0, 0)
    assert (got["out_off"] == 0).all() and (got["out_len"] == 0).all() and (got["src_index"] == G.NONE).all()
    assert (got["frag_index"] == 0).all() and (got["oc_n_hdrs"] == 0).all() and (got["dst_rest"] == 0xA5).all()
    rc, got = G.host_call(b, ch, 576, flags=G.NO_WRITE)
    assert rc == 0 and (got["n_out"], got["bytes_out"]) == (0, 0)


def refusals():
    from pktgpu import _lib
    odd = np.zeros(64, np.uint8)
    base = odd.ctypes.data
    r = {"null_batch": {A_BATCH: None}, "null_chain": {A_CHAIN: None}, "which_16": {A_WHICH: 16}, "which_0xFE": {A_WHICH: 0xFE},
         "flag_bit_4": {A_FLAGS: 4}, "flag_bit_31": {A_FLAGS: 1 << 31}, "mtu_all_65536": {A_MTU: None, A_MTU_ALL: 65536},
         "dst_misaligned": {A_DST: base + 8}, "hits_misaligned": {A_HITS: base + 4}, "out_off_misaligned": {A_OFF: base + 4},
         "mtu_misaligned": {A_MTU: base + 1}, "null_dst": {A_DST: None}, "null_out_off": {A_OFF: None}, "null_out_len": {A_LEN: None},
         "out_cap_0": {A_CAP: 0}, "out_cap_2_32": {A_CAP: 1 << 32}}
    for col in ("n_hdrs", "hdr_type", "hdr_off"):
        ch = _lib.PktChain(base, base, base)
        setattr(ch, col, None)
        r[f"null_chain_{col}"] = {A_CHAIN: ctypes.byref(ch)}
    return r, (odd,)


REFUSALS = sorted(refusals()[0])


@pytest.mark.parametrize("name", REFUSALS)
def test_refusals(name):
    over, keep = refusals()
    b, ch = G.layout([G.v4(1000), G.v4(100)])
    rc, got = G.host_call(b, ch, np.asarray([576, 576], np.uint16), over=over[name], cap=8, dst_len=4096)
    assert rc == INVALID and got["guards"]
    assert (got["status"] == 0xA5).all() and (got["dst_rest"] == 0xA5).all() and (got["hits"] == 0).all()


@pytest.mark.parametrize("form", ["n_2_32", "offsets_without_lens", "stride_0", "null_slab"])
def test_batch_refusals(form):
    from pktgpu import _lib
    L = _lib.load()
    b, ch = G.layout([G.v4(1000), G.v4(100)])
    pb, keep = pktgpu._host_batch(_lib, b)
    if form == "n_2_32":
        pb.n = 1 << 32
    elif form == "offsets_without_lens":
        pb.lens = None
    elif form == "stride_0":
        pb.offsets, pb.stride = None, 0
    else:
        pb.slab = None
    cols = [np.ascontiguousarray(ch[k]) for k in ("n_hdrs", "hdr_type", "hdr_off")]
    pc = _lib.PktChain(*[c.ctypes.data for c in cols])
    tot, cnt = ctypes.c_uint64(7), ctypes.c_uint64(7)
    rc = L.pkt_frag_host(ctypes.byref(pb), ctypes.byref(pc), 0, schema.FRAG_NO_WRITE, None, 576, None, None, None, None, None, 0, 0,
                         None, None, None, None, None, None, ctypes.byref(tot), ctypes.byref(cnt))
    assert rc == INVALID and (tot.value, cnt.value) == (0, 0)


def test_no_write_takes_null_and_zero_for_every_output():
    b, ch = G.layout([G.v4(1000), G.v4(100)])
    rc, got = G.host_call(b, ch, 576, flags=G.NO_WRITE, skip=["status", "nfrag", "first", "hits"])
    assert rc == 0 and (got["n_out"], got["bytes_out"]) == (3, G.r16(14 + 20 + 552) + G.r16(14 + 20 + 448) + G.r16(134))


# ------------------------------------------------------------------ 5. out_chain feeds the next calls
def test_out_chain_feeds_fwd_and_flow_key():
    """pkt_fwd_host and pkt_flow_key_host over the output batch with out_chain: every output forwards at the
    fragments' mtu, and the fragments key without ports."""
    items = [G.v4(1466), G.v4(100), G.v4(3000, vlan=True), G.vxlan(1400), G.v4(600)]
    m = 576
    b, ch = G.layout(items)
    r = pktgpu.Parser.fragment(None, b, ch, mtu=m, host=True)
    assert r.n_out == 3 + 1 + 6 + 3 + 2 and r.status.tolist() == [G.SPLIT, G.FITS, G.SPLIT, G.SPLIT, G.SPLIT]
    k = r.n_out
    ob = dict(slab=r.slab, offsets=r.offsets, lens=r.lens)
    oc = r.out_chain
    fwd = pktgpu.Forwarder(None, [("02:00:00:00:00:01", "02:00:00:00:00:02", 9, m)])
    f = fwd.run(ob, oc, nexthop=np.zeros(k, np.uint32), write=False)
    assert (f["status"][:k] == pktgpu.FWD_OK).all() and (f["port"][:k] == 9).all()
    assert (f["status"][k:] == pktgpu.FWD_NO_IP).all()
    fk = pktgpu.flow_keys(r.slab, oc, which_ip=0, offsets=r.offsets, lens=r.lens)
    keys = fk["keys"].view(schema.FLOW_KEY_DTYPE).reshape(-1)
    frag = r.nfrag[r.src_index[:k]] > 1
    assert (keys["sport"][:k][frag] == 0).all() and (keys["dport"][:k][frag] == 0).all()
    assert (keys["ipver"][:k] == 4).all() and (keys["proto"][:k] == 17).all()
    assert not (keys["sport"][:k][~frag] == 0).all()
