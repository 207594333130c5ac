"""pkt_nat_* on a host handle (pkt_nat_create_host: the sequential twin, no device) against nat_cases' model, byte for
byte on the slab and exactly on status, entry, created, hits, bytes and sessions().  The twin runs the decision, the
arithmetic and the stores of pktgpu_nat.hpp, which the kernels share."""
import ctypes
import re
import struct

import numpy as np
import pytest

import pktgpu
from pktgpu import schema

import nat_cases as N

PORTS = (40000, 40999)


def pair(pool=N.POOL1, ports=PORTS, slots=1024, static=()):
    return pktgpu.Nat(None, pool, ports, slots, static), N.Model(pool, ports, static)


def run_both(nat, model, items, kind="indexed", label="", **kw):
    """One call on the twin and on the model over the same batch -> (got, want, batch); the two are compared."""
    b, ch = N.layout(items, kind)
    want = model.run(b, ch, **kw)
    slab = b["slab"].copy()
    r = nat.run(dict(b, slab=slab), ch, counters=True, **kw)
    got = dict(status=r.status, entry=r.entry, created=r.created, hits=r.hits, bytes=r.bytes, slab=slab)
    N.check(got, want, label)
    assert int(got["hits"].sum()) == b["n"]
    N.same_sessions(nat.sessions(), model.sessions(), label)
    assert nat.count() == model.count()
    return got, want, b


def test_verifier_is_rfc_1071():
    assert N.ones_sum(bytes.fromhex("0001f203f4f5f6f7")) == 0xDDF2  # RFC 1071 section 3
    assert N.ones_sum(b"\xff\xff\x00\x01") == 1 and N.ones_sum(b"\x01") == 0x0100
    for l4 in ("TCP", "UDP", "ICMP"):
        item = N.mk(l4, "10.0.0.1", 5, N.REMOTE, 6, payload=b"odd")
        ipo, l4o = N.offsets(item)
        assert N.ip_valid(item[0], ipo) and N.l4_valid(item[0], ipo, l4o)
        assert not N.l4_valid(N.mk(l4, "10.0.0.1", 5, N.REMOTE, 6, good=False)[0], ipo, l4o)


def test_every_status():
    nat, m = pair()
    cases = N.statuses_items()
    got, want, _ = run_both(nat, m, [c[0] for c in cases], dir=np.array([c[1] for c in cases], np.uint8),
                            select=np.array([c[2] for c in cases], np.uint8), now=5)
    assert list(want["status"]) == list(range(10))
    # EXHAUSTED and TABLE_FULL have tests of their own; a dir above 1 skips
    got, want, _ = run_both(nat, m, [cases[0][0]] * 3, dir=np.array([2, 255, 0], np.uint8))
    assert list(want["status"]) == [N.SKIPPED, N.SKIPPED, N.OK]


@pytest.mark.parametrize("l4", ["TCP", "UDP", "ICMP"])
def test_l4_bytes_end_at_the_packets_last_byte_and_one_short(l4):
    nat, m = pair()
    item = N.mk(l4, "10.0.0.1", 700, N.REMOTE, 80, payload=b"")
    ipo, l4o = N.offsets(item)
    need = l4o + N.L4_NEED[("TCP", "UDP", "ICMP").index(l4)]
    got, want, _ = run_both(nat, m, [N.cut(item, need), N.cut(item, need - 1), N.cut(item, ipo + 20), N.cut(item, ipo + 19)])
    assert list(want["status"]) == [N.OK, N.SPAN, N.SPAN, N.SPAN]


def test_fragments_options_and_icmp_types():
    nat, m = pair()
    base = N.mk("UDP", "10.0.0.1", 700, N.REMOTE, 80)
    ipo, l4o = N.offsets(base)

    def patched(at, data):
        q = bytearray(base[0])
        q[at:at + len(data)] = data
        return bytes(q), base[1]
    first, later, df = patched(ipo + 6, b"\x20\x00"), patched(ipo + 6, b"\x00\x10"), patched(ipo + 6, b"\x40\x00")
    icmp = [N.mk("ICMP", "10.0.0.1", 9, N.REMOTE, 0, icmp_type=t) for t in (8, 0, 3)]
    got, want, _ = run_both(nat, m, [first, later, df, patched(ipo, b"\x46"), patched(ipo, b"\x44")] + icmp)
    assert list(want["status"]) == [N.FRAGMENT, N.FRAGMENT, N.OK, N.BAD_HDR, N.BAD_HDR, N.OK, N.OK, N.NO_L4]


@pytest.mark.parametrize("l4,stored", [("UDP", 0xFFFF), ("TCP", 0)])
def test_an_update_that_lands_on_zero(l4, stored):
    nat, m = pair()
    d = N.dport_landing_on_zero(l4, N.POOL1[0], PORTS[0])
    item = N.mk(l4, "10.0.0.1", 700, N.REMOTE, d)
    got, want, b = run_both(nat, m, [item, N.mk(l4, "10.0.0.1", 700, N.REMOTE, d + 1)])
    p = N.packet_after(b, got["slab"], 0)
    ipo, l4o = N.offsets(item)
    ck = l4o + (16 if l4 == "TCP" else 6)
    assert struct.unpack_from(">H", p, ck)[0] == stored
    assert N.l4_valid(p, ipo, l4o) and N.ip_valid(p, ipo)
    assert struct.unpack_from(">H", N.packet_after(b, got["slab"], 1), ck)[0] not in (0, 0xFFFF)


def test_udp_without_a_checksum_stays_without():
    nat, m = pair()
    item = N.mk("UDP", "10.0.0.1", 700, N.REMOTE, 53, udp_none=True)
    got, want, b = run_both(nat, m, [item])
    p = N.packet_after(b, got["slab"], 0)
    ipo, l4o = N.offsets(item)
    assert p[l4o + 6:l4o + 8] == b"\0\0" and N.l4_valid(p, ipo, l4o) is None and N.ip_valid(p, ipo)
    assert p[ipo + 12:ipo + 16] == N.ip(N.POOL1[0]) and struct.unpack_from(">H", p, l4o)[0] == PORTS[0]


@pytest.mark.parametrize("vlans", [0, 1, 2])
def test_valid_stays_valid_and_wrong_stays_as_wrong(vlans):
    nat, m = pair(static=N.STATICS)
    items, dirs = [], []
    for k, l4 in enumerate(("TCP", "UDP", "ICMP")):
        for good in (True, False):
            items.append(N.mk(l4, "10.0.0.%d" % (k + 1), 900 + k, N.REMOTE, 443, vlans=vlans, payload=b"x" * (k + 5), good=good))
            dirs.append(N.OUT)
    items.append(N.mk("TCP", N.REMOTE, 443, "192.0.2.200", 80, vlans=vlans))          # a static, inbound
    dirs.append(N.IN)
    items.append(N.mk("TCP", "10.9.9.9", 8080, N.REMOTE, 443, vlans=vlans, good=False))  # and outbound
    dirs.append(N.OUT)
    got, want, b = run_both(nat, m, items, dir=np.array(dirs, np.uint8), now=3)
    assert (want["status"] == N.OK).all()
    for i, item in enumerate(items):
        before, after = item[0], N.packet_after(b, got["slab"], i)
        ipo, l4o = N.offsets(item)
        assert before != after
        assert N.ip_error(after, ipo) == N.ip_error(before, ipo), i
        assert N.l4_error(after, ipo, l4o) == N.l4_error(before, ipo, l4o), i
        if N.ip_error(before, ipo) == 0:
            assert N.ip_valid(after, ipo) and N.l4_valid(after, ipo, l4o), i


def test_a_capture_cut_by_snaplen_translates_as_the_whole_packet_does():
    nat, m = pair()
    whole = [N.mk(l4, "10.0.0.1", 900 + k, N.REMOTE, 443, payload=bytes(range(200))) for k, l4 in enumerate(("TCP", "UDP", "ICMP"))]
    got_w, _, bw = run_both(nat, m, whole)
    nat2, m2 = pair()
    got_c, _, bc = run_both(nat2, m2, [N.cut(it, 60) for it in whole])
    for i, item in enumerate(whole):
        full, short = N.packet_after(bw, got_w["slab"], i), N.packet_after(bc, got_c["slab"], i)
        assert len(short) == 60 and short == full[:60]
        ipo, l4o = N.offsets(item)
        assert N.l4_valid(full, ipo, l4o) and N.ip_valid(short, ipo)


def test_round_trip_restores_the_inside_endpoint():
    nat, m = pair(static=N.STATICS)
    out = [N.flow_item(k, vlans=k % 3) for k in range(9)] + [N.mk("TCP", "10.9.9.9", 8080, N.REMOTE, 443)]
    # IN before any OUT: no session (the static answers at once)
    probe = [N.mk("TCP", N.REMOTE, 443, N.POOL1[0], PORTS[0]), N.mk("TCP", N.REMOTE, 443, "192.0.2.200", 80)]
    got, want, _ = run_both(nat, m, probe, dir=N.IN)
    assert list(want["status"]) == [N.NO_SESSION, N.OK]
    got, want, b = run_both(nat, m, out, dir=N.OUT, now=10)
    assert (want["status"] == N.OK).all() and want["created"].sum() == 9
    translated = [(N.packet_after(b, got["slab"], i), out[i][1]) for i in range(len(out))]
    back = [N.reply(t) for t in translated]
    got, want, b2 = run_both(nat, m, back, dir=N.IN, now=20)
    assert (want["status"] == N.OK).all() and not want["created"].any()
    for i, item in enumerate(out):
        p = N.packet_after(b2, got["slab"], i)
        ipo, l4o = N.offsets(item)
        assert p[ipo + 16:ipo + 20] == item[0][ipo + 12:ipo + 16], i
        idp = l4o + (4 if p[ipo + 9] == 1 else 2)
        src = l4o + (4 if p[ipo + 9] == 1 else 0)
        assert p[idp:idp + 2] == item[0][src:src + 2], i
        assert N.ip_valid(p, ipo) and N.l4_valid(p, ipo, l4o), i
    assert (nat.sessions()["last_seen"][:9] == 20).all()


def test_an_in_packet_before_its_sessions_creator_in_one_batch():
    nat, m = pair()
    o = N.mk("UDP", "10.0.0.1", 5000, N.REMOTE, 53)
    i_ = N.mk("UDP", N.REMOTE, 53, N.POOL1[0], PORTS[0])  # the entry the first creator gets
    got, want, _ = run_both(nat, m, [i_, o, i_], dir=np.array([N.IN, N.OUT, N.IN], np.uint8), now=1)
    assert list(want["status"]) == [N.OK, N.OK, N.OK] and list(want["created"]) == [0, 1, 0]


@pytest.mark.parametrize("which,ok", [(0, True), (1, True), (N.LAST, True), (2, False)])
def test_vxlan_which_ip(which, ok):
    nat, m = pair()
    item = N.vxlan()
    got, want, b = run_both(nat, m, [item, N.mk("TCP", "10.0.0.1", 1, N.REMOTE, 2)], which_ip=which)
    assert want["status"][0] == (N.OK if ok else N.NO_IP)
    if ok:
        k = 0 if which == 0 else 1
        ipo, l4o = N.offsets(item, k)
        p = N.packet_after(b, got["slab"], 0)
        assert p[ipo + 12:ipo + 16] == N.ip(N.POOL1[0]) and N.ip_valid(p, ipo)
        other = N.offsets(item, 1 - k)[0]
        assert p[other:other + 20] == item[0][other:other + 20] or k == 1  # (the outer UDP checksum covers the inner bytes)


def test_statics_in_both_directions_and_beside_dynamic_sessions():
    nat, m = pair(static=N.STATICS)
    items = [N.mk("TCP", "10.9.9.9", 8080, N.REMOTE, 1), N.mk("UDP", "10.9.9.9", 5353, N.REMOTE, 1),
             N.mk("ICMP", "10.9.9.8", 77, N.REMOTE, 0), N.mk("TCP", "10.9.9.9", 8081, N.REMOTE, 1),
             N.mk("TCP", N.REMOTE, 1, "192.0.2.200", 80), N.mk("UDP", N.REMOTE, 1, "192.0.2.1", 53),
             N.mk("ICMP", N.REMOTE, 77, "192.0.2.201", 0, icmp_type=0), N.mk("UDP", N.REMOTE, 1, "192.0.2.200", 80),
             N.mk("UDP", N.REMOTE, 1, "192.0.2.1", 54)]
    dirs = np.array([0, 0, 0, 0, 1, 1, 1, 1, 1], np.uint8)
    got, want, _ = run_both(nat, m, items, dir=dirs, now=9)
    assert list(want["status"]) == [N.OK] * 7 + [N.NOT_OURS, N.NOT_OURS]
    assert list(want["entry"][:3]) == [N.STATIC | 0, N.STATIC | 1, N.STATIC | 2] and want["entry"][3] == 0
    assert nat.expire(10 ** 6, 1) == 1 and m.expire(10 ** 6, (1, 1, 1)) == 1
    N.same_sessions(nat.sessions(), m.sessions())
    assert len(nat.sessions()) == 3


REFUSALS = [
    (dict(pool=[]), "naddr not in 1..64"),
    (dict(pool=["192.0.2.%d" % k for k in range(65)]), "naddr not in 1..64"),
    (dict(ports=(0, 10)), "ports not 1 <= port_lo <= port_hi <= 65535"),
    (dict(ports=(11, 10)), "ports not 1 <= port_lo <= port_hi <= 65535"),
    (dict(ports=(1, 65536)), "ports not 1 <= port_lo <= port_hi <= 65535"),
    (dict(slots=32), "slots not a power of two in 64..2^26"),
    (dict(slots=96), "slots not a power of two in 64..2^26"),
    (dict(slots=1 << 27), "slots not a power of two in 64..2^26"),
    (dict(pool=["192.0.2.1", "192.0.2.2", "192.0.2.1"]), "duplicate pool address"),
    (dict(static=[(47, "10.0.0.1", 1, "192.0.2.9", 1)]), "a static's proto is not 6, 17 or 1"),
    (dict(static=[("tcp", "10.0.0.1", 1, "192.0.2.9", 1), ("tcp", "10.0.0.1", 1, "192.0.2.9", 2)]), "duplicate inside endpoint"),
    (dict(static=[("tcp", "10.0.0.1", 1, "192.0.2.9", 1), ("tcp", "10.0.0.2", 1, "192.0.2.9", 1)]), "duplicate outside endpoint"),
    (dict(static=[("udp", "10.0.0.1", 1, "192.0.2.1", 40500)]), "a static's outside endpoint is a dynamic pool entry"),
    (dict(slots=64, static=[("udp", "10.0.0.1", 1 + k, "192.0.2.9", 1 + k) for k in range(33)]), "nstatic above slots / 2"),
]


@pytest.mark.parametrize("kw,text", REFUSALS, ids=[f"{k}-{t[:24]}" for k, (_, t) in enumerate(REFUSALS)])
def test_create_refusals(kw, text):
    args = dict(pool=N.POOL1, ports=PORTS, slots=1024, static=())
    args.update(kw)
    with pytest.raises(ValueError, match=re.escape("pkt_nat_create_host: " + text)):
        pktgpu.Nat(None, **args)


def test_create_accepts_what_is_next_to_the_refusals():
    st = np.zeros(1, schema.NAT_STATIC_DTYPE)
    st["proto"], st["in_port"], st["out_port"] = 6, 1, 39999  # the pool's address, a port just below the range
    st["in_addr"][0], st["out_addr"][0] = np.frombuffer(N.ip("10.0.0.1"), np.uint8), np.frombuffer(N.ip(N.POOL1[0]), np.uint8)
    pktgpu.Nat(None, N.POOL1, PORTS, 64, st).close()
    st["zero"][0, 2] = 1
    with pytest.raises(ValueError, match="non-zero `zero`"):
        pktgpu.Nat(None, N.POOL1, PORTS, 64, st)
    pktgpu.Nat(None, ["192.0.2.%d" % k for k in range(64)], (1, 65535), 64).close()
    too_many = np.zeros(4097, schema.NAT_STATIC_DTYPE)
    with pytest.raises(ValueError, match="nstatic above PKT_NAT_MAX_STATIC"):
        pktgpu.Nat(None, N.POOL1, PORTS, 1 << 14, too_many)


def test_allocation_order_with_creators_interleaved_over_the_protocols():
    nat, m = pair(pool=["192.0.2.1", "192.0.2.2"], ports=(5000, 5006))
    rng = np.random.default_rng(11)
    flows = [N.flow_item(k) for k in range(18)]
    order = [int(x) for x in rng.integers(0, 18, 120)]  # many packets per new flow, the flows interleaved
    got, want, _ = run_both(nat, m, [flows[k] for k in order], now=4)
    assert want["created"].sum() == len(set(order)) and (want["status"] == N.OK).all()
    first = {}
    for i, k in enumerate(order):
        first.setdefault(k, i)
    for px in range(3):  # per protocol, the creators in index order take entries 0, 1, 2, ...
        creators = sorted(i for k, i in first.items() if k % 3 == px)
        assert [int(want["entry"][i]) for i in creators] == [px * m.E + j for j in range(len(creators))]
    got, want, _ = run_both(nat, m, [flows[k] for k in order[::-1]], now=5)
    assert not want["created"].any()


def test_exhaustion_and_the_retry_after_expire():
    nat, m = pair(ports=(6000, 6003))
    flows = [N.mk("UDP", "10.0.0.%d" % (k + 1), 100, N.REMOTE, 53) for k in range(6)]
    items = [flows[k] for k in (0, 1, 2, 3, 4, 0, 4, 5, 4)] + [N.mk("TCP", "10.0.0.1", 100, N.REMOTE, 53)]
    got, want, _ = run_both(nat, m, items, now=100)
    assert list(want["status"]) == [N.OK] * 4 + [N.EXHAUSTED, N.OK, N.EXHAUSTED, N.EXHAUSTED, N.EXHAUSTED, N.OK]
    assert nat.count() == (1, 4, 0)
    got, want, _ = run_both(nat, m, [flows[4], flows[1]], now=150)  # still full; flow 1 is refreshed
    assert list(want["status"]) == [N.EXHAUSTED, N.OK]
    assert nat.expire(200, (0, 100, 0)) == 3 == m.expire(200, (0, 100, 0))  # flow 1 was seen at 150
    got, want, _ = run_both(nat, m, [flows[4], flows[5], flows[4]], now=201)
    assert list(want["status"]) == [N.OK] * 3 and list(want["created"]) == [1, 1, 0]


def test_expire_per_protocol_idle_and_statics():
    nat, m = pair(static=N.STATICS)
    run_both(nat, m, [N.flow_item(k) for k in range(12)], now=100)
    run_both(nat, m, [N.flow_item(k) for k in (0, 1, 2)], now=160)
    for now, idle, gone in ((159, (60, 60, 60), 0), (160, (60, 0, 61), 3), (161, (0, 61, 0), 3), (2 ** 32 - 1, (0, 0, 2 ** 32 - 1), 0),
                            (220, (60, 60, 60), 6)):
        assert nat.expire(now, idle) == gone == m.expire(now, idle), (now, idle)
        N.same_sessions(nat.sessions(), m.sessions(), str(now))
    assert nat.count() == (0, 0, 0) and len(nat.sessions()) == len(N.STATICS)
    got, want, _ = run_both(nat, m, [N.flow_item(k) for k in range(12)], now=300)  # the cursors stayed where they were
    assert list(want["entry"][:3]) == [4, m.E + 4, 2 * m.E + 4]


def test_allocation_wraps_past_the_cursor_into_freed_entries():
    nat, m = pair(pool=["192.0.2.1", "192.0.2.2", "192.0.2.3"], ports=(2000, 3036), slots=1 << 13)
    assert m.E == 3 * 1037 and m.E % 32 and m.E % 1024
    udp = [N.mk("UDP", N.INSIDE + 1 + k // 50000, 1 + k % 50000, N.REMOTE, 53) for k in range(m.E - 3)]
    run_both(nat, m, udp[:1500], now=10)
    run_both(nat, m, udp[1500:], now=20)
    assert m.cursor[1] == m.E - 3
    assert nat.expire(30, (0, 20, 0)) == 1500 == m.expire(30, (0, 20, 0))  # entries 0..1499 are free again
    fresh = [N.mk("UDP", "10.200.0.1", 1 + k, N.REMOTE, 53) for k in range(40)]
    got, want, _ = run_both(nat, m, fresh, now=31)
    assert [int(e) - m.E for e in want["entry"]] == [m.E - 3, m.E - 2, m.E - 1] + list(range(37))
    assert m.cursor[1] == 37


def test_table_full_by_invariants():
    args = (N.POOL1, PORTS, ())
    nat = pktgpu.Nat(None, N.POOL1, PORTS, 64)
    m = N.Model(*args)
    early = [N.flow_item(k) for k in range(10)]
    run_both(nat, m, early, now=1)
    flows = [N.mk("UDP", "10.77.0.%d" % (1 + k % 200), 3000 + k, N.REMOTE, 53) for k in range(100)]
    items = flows + flows[::3]
    b, ch = N.layout(items)
    slab = b["slab"].copy()
    r = nat.run(dict(b, slab=slab), ch, counters=True, now=2)
    got = dict(status=r.status, entry=r.entry, slab=slab)
    by_key, by_ent = N.invariants(got, b, ch, args, [N.OUT] * len(items))
    assert (r.status == N.TABLE_FULL).any() and (r.status == N.OK).any()
    assert int(r.hits.sum()) == len(items) and r.hits[N.OK] + r.hits[N.TABLE_FULL] == len(items)
    assert sum(nat.count()) <= 64 and sum(nat.count()) == 10 + len(by_ent)
    assert not set(by_ent) & {int(e) for e in m.run(*N.layout(early), now=1)["entry"]}
    assert r.created.sum() == len(by_ent)
    # the sessions of the earlier call still translate exactly: the records' first ten, and the packets
    rec = nat.sessions()
    want = m.sessions()
    for row in want:
        assert row.tobytes() in {x.tobytes() for x in rec}
    b2, ch2 = N.layout(early)
    slab2 = b2["slab"].copy()
    r2 = nat.run(dict(b2, slab=slab2), ch2, now=1)
    N.check(dict(status=r2.status, entry=r2.entry, created=r2.created, slab=slab2), m.run(b2, ch2, now=1))


def test_no_write_creates_and_refreshes_and_stores_nothing():
    nat, m = pair()
    items = [N.flow_item(k) for k in range(5)]
    got, want, b = run_both(nat, m, items, now=7, write=False)
    assert np.array_equal(got["slab"], b["slab"]) and want["created"].sum() == 5
    got, want, b = run_both(nat, m, items, now=8)
    assert not want["created"].any() and not np.array_equal(got["slab"], b["slab"])


def test_every_null_output_combination():
    items = [N.flow_item(k) for k in range(4)] + [N.statuses_items()[2][0]]
    b, ch = N.layout(items)
    for mask in range(8):
        outs = tuple(nm for k, nm in enumerate(N.NAMES) if mask >> k & 1)
        for counters in (None, True):
            nat, m = pair()
            want = m.run(b, ch, now=1)
            slab = b["slab"].copy()
            r = nat.run(dict(b, slab=slab), ch, now=1, outputs=outs, counters=counters)
            got = dict(status=r.status, entry=r.entry, created=r.created, hits=r.hits, bytes=r.bytes, slab=slab)
            assert [nm for nm in N.NAMES if got[nm] is not None] == list(outs)
            N.check(got, want, f"{outs} {counters}")
            N.same_sessions(nat.sessions(), m.sessions())
    nat, m = pair()
    h = np.full(12, 5, np.uint64)
    nat.run(dict(b, slab=b["slab"].copy()), ch, counters=(h, None))
    assert h.sum() == 60 + len(items)


def raw_call(nat, b, ch, which_ip=0, flags=0, dir_all=0, dirp=None, hits=None, chain_null=None, null_batch=False):
    lib = nat._lib
    pb, keep = pktgpu._host_batch(lib, b)
    cols = [np.ascontiguousarray(ch[k]) for k in ("n_hdrs", "hdr_type", "hdr_off")]
    ptrs = [c.ctypes.data for c in cols]
    if chain_null is not None:
        ptrs[chain_null] = None
    pc = lib.PktChain(*ptrs)
    rc = nat._L.pkt_nat_batch(nat._t, None if null_batch else ctypes.byref(pb), ctypes.byref(pc), which_ip, flags, dir_all,
                              dirp, None, 0, None, None, None, hits, None, None)
    return rc, nat._L.pkt_nat_last_error(nat._t).decode()


def test_call_refusals_and_n_0():
    nat, m = pair()
    b, ch = N.layout([N.flow_item(0)])
    h = np.zeros(13, np.uint64)
    for kw, text in ((dict(null_batch=True), "null argument"), (dict(which_ip=16), "which_ip is neither below 16 nor PKT_FLOW_LAST"),
                     (dict(which_ip=0xFE), "which_ip is neither below 16 nor PKT_FLOW_LAST"), (dict(flags=2), "unknown flag bits"),
                     (dict(dir_all=2), "dir_all is neither PKT_NAT_OUT nor PKT_NAT_IN"),
                     (dict(hits=h.ctypes.data + 4), "hits / bytes not 8-byte aligned"),
                     (dict(chain_null=0), "null chain column"), (dict(chain_null=2), "null chain column")):
        rc, msg = raw_call(nat, b, ch, **kw)
        assert rc != 0 and msg == "pkt_nat_batch: " + text, (kw, msg)
    rc, msg = raw_call(nat, dict(b, offsets=None, lens=None, stride=0, n=1), ch)
    assert rc != 0 and msg == "pkt_nat_batch: stride 0"
    assert nat.count() == (0, 0, 0)  # nothing ran
    rc, _ = raw_call(nat, b, ch, dir_all=2, dirp=np.zeros(1, np.uint8).ctypes.data)  # dir given: dir_all is not looked at
    assert rc == 0 and nat.count()[0] + nat.count()[1] + nat.count()[2] == 1
    empty = dict(slab=np.zeros(0, np.uint8), offsets=np.zeros(0, np.uint64), lens=np.zeros(0, np.uint32), stride=None, n=0)
    r = nat.run(empty, {k: v[..., :0] for k, v in ch.items()}, counters=True)
    assert r.status.size == 0 and r.hits.sum() == 0
    assert nat._L.pkt_nat_expire(nat._t, 0, None, None) != 0
    nat.clear()
    assert nat.count() == (0, 0, 0)
    run_both(nat, N.Model(N.POOL1, PORTS), [N.flow_item(3)])  # cleared: the cursors are 0 again
