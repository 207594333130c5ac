"""pkt_nat_create / pkt_nat_batch / pkt_nat_expire on the device (Parser.nat / Nat.run): the kernels of pktgpu_nat.hip
against nat_cases' sequential model, exactly: status, entry, created, hits, bytes, the whole slab and sessions().  The
decision and the arithmetic are covered on the CPU (test_nat_host.py: the host twin runs the same inline code); here it
is the claim, the ranking of the creators across waves, blocks and chunks, the selection of the free entries, the
stores at every alignment and the counters.  The slab lies between two guard regions filled with 0xA5 and is compared
whole, so that a byte the call must not write is seen."""
import ctypes

import numpy as np
import pytest

import pktgpu
from pktgpu import schema

import compare_cases as C
import fwd_cases as W
import nat_cases as N

pytestmark = pytest.mark.gpu
GUARD = 4096
PORTS = (40000, 40999)
BLOCK = 256  # the claim kernel's block


@pytest.fixture(scope="module")
def P():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible")
    return pktgpu.Parser(0)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def dev_batch(b):
    """The batch on the device, its slab in the middle of a 0xA5-filled allocation -> (batch dict, the allocation)."""
    import torch
    nbytes = b["slab"].size
    big = torch.full((GUARD + (nbytes + 15) // 16 * 16 + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    slab = big[GUARD:GUARD + nbytes]
    slab.copy_(dev(b["slab"]))
    kw = dict(slab=slab, n=b["n"], stride=b["stride"], offsets=None if b["offsets"] is None else dev(b["offsets"]),
              lens=None if b["lens"] is None else dev(b["lens"]))
    return kw, big


def guards_intact(big, nbytes):
    return bool((big[:GUARD] == 0xA5).all()) and bool((big[GUARD + nbytes:] == 0xA5).all())


def launch(nat, b, ch, stream=None, **kw):
    """Queue one call over a fresh device copy of the batch -> what collect() needs."""
    db, big = dev_batch(b)
    dch = {k: dev(v) for k, v in ch.items()}
    for k in ("dir", "select"):
        if isinstance(kw.get(k), np.ndarray):
            kw[k] = dev(kw[k])
    r = nat.run(db, dch, counters=True, stream=stream, **kw)
    return r, db, big, dch, kw


def collect(q, b):
    import torch
    r, db, big, _, _ = q
    torch.cuda.synchronize()
    got = {k: None if getattr(r, k) is None else getattr(r, k).cpu().numpy() for k in N.NAMES + ("hits", "bytes")}
    got["slab"] = db["slab"].cpu().numpy()
    assert guards_intact(big, b["slab"].size), "a byte outside the slab was written"
    return got


def pair(P, pool=N.POOL1, ports=PORTS, slots=1024, static=()):
    return P.nat(pool, ports, slots, static), N.Model(pool, ports, static)


def run_both(nat, model, items, kind="indexed", label="", sessions=True, **kw):
    b, ch = N.layout(items, kind) if isinstance(items, list) else items
    want = model.run(b, ch, **kw)
    got = collect(launch(nat, b, ch, **kw), b)
    N.check(got, want, label)
    assert int(got["hits"].sum()) == b["n"]
    if sessions:
        N.same_sessions(nat.sessions(), model.sessions(), label)
        assert nat.count() == model.count()
    return got, want, b


# ------------------------------------------------------------------ the host suite's cases, on the device
def test_every_status_and_forged_columns(P):
    nat, m = pair(P)
    cases = N.statuses_items()
    got, want, _ = run_both(nat, m, [c[0] for c in cases], dir=np.array([c[1] for c in cases], np.uint8),
                            select=np.array([c[2] for c in cases], np.uint8), now=5)
    assert list(want["status"]) == list(range(10))
    # offsets that point out of the packet give SPAN, never an access: the IP entry, then the L4 entry
    p = N.mk("UDP", "10.0.0.1", 1, N.REMOTE, 2)[0][14:]
    forged = [(p, [(N.T_IPV4, 65535), (N.T_UDP, 20)]), (p, [(N.T_IPV4, 0), (N.T_UDP, 65535)]),
              (p, [(N.T_IPV4, len(p) - 19), (N.T_UDP, 0)]), (p, [(N.T_IPV4, 0), (N.T_UDP, len(p) - 7)]),
              (p, [(N.T_IPV4, 0), (N.T_UDP, len(p) - 8)]), (p, [(N.T_IPV4, 0), (N.T_UDP, 20)])]
    got, want, _ = run_both(nat, m, forged)
    assert list(want["status"]) == [N.SPAN] * 4 + [N.OK, N.OK]
    nat.close()


@pytest.mark.parametrize("kind", ["indexed", "stride"])
def test_checksums_boundaries_and_every_alignment(P, kind):
    """Every protocol, 0-2 tags, good and bad checksums, the L4 boundary cuts, fragments, ICMP types, UDP without a
    checksum and the updates that land on zero, each at alignments 0..15 ("indexed": packet i at i % 16, the last one
    ending at the slab's last byte) and in fixed-stride slots."""
    nat, m = pair(P, static=N.STATICS)
    items, dirs = [], []
    for rep in range(2):
        for k, l4 in enumerate(("TCP", "UDP", "ICMP")):
            for vlans in (0, 1, 2):
                it = N.mk(l4, "10.0.%d.%d" % (rep, k + 1), 900 + vlans, N.REMOTE, 443, vlans=vlans, payload=b"y" * (3 * k + rep),
                          good=bool(vlans != 1))
                ipo, l4o = N.offsets(it)
                items += [it, N.cut(it, l4o + N.L4_NEED[k]), N.cut(it, l4o + N.L4_NEED[k] - 1)]
                dirs += [N.OUT] * 3
    for l4 in ("UDP", "TCP"):  # flows 10.1.0.1: their entries are whatever comes next; the model says which
        items.append(N.mk(l4, "10.1.0.1", 5, N.REMOTE, N.dport_landing_on_zero(l4, N.POOL1[0], PORTS[0] + 6)))
        dirs.append(N.OUT)
    items += [N.mk("UDP", "10.1.0.2", 5, N.REMOTE, 53, udp_none=True), N.mk("ICMP", "10.1.0.2", 5, N.REMOTE, 0, icmp_type=3),
              N.mk("TCP", N.REMOTE, 443, "192.0.2.200", 80), N.mk("TCP", "10.9.9.9", 8080, N.REMOTE, 443),
              N.mk("UDP", N.REMOTE, 1, N.POOL1[0], PORTS[0]), N.mk("UDP", N.REMOTE, 1, N.POOL1[0], PORTS[1])]
    dirs += [N.OUT, N.OUT, N.IN, N.OUT, N.IN, N.IN]
    got, want, b = run_both(nat, m, items, kind=kind, dir=np.array(dirs, np.uint8), now=3)
    assert set(want["status"]) == {N.OK, N.SPAN, N.NO_L4, N.NO_SESSION}
    for i, item in enumerate(items):  # the verifier, on the device's bytes
        if want["status"][i] != N.OK or len(item[0]) < 60:
            continue
        before, after = item[0], N.packet_after(b, got["slab"], i)
        ipo, l4o = N.offsets(item)
        assert N.ip_error(after, ipo) == N.ip_error(before, ipo) and N.l4_error(after, ipo, l4o) == N.l4_error(before, ipo, l4o), i
    nat.close()


def test_round_trip_and_in_before_out_in_one_batch(P):
    nat, m = pair(P, static=N.STATICS)
    out = [N.flow_item(k, vlans=k % 3) for k in range(9)] + [N.mk("TCP", "10.9.9.9", 8080, N.REMOTE, 443)]
    got, want, _ = run_both(nat, m, [N.mk("TCP", N.REMOTE, 443, N.POOL1[0], PORTS[0])], dir=N.IN)
    assert list(want["status"]) == [N.NO_SESSION]
    # the replies to what the OUT packets will become stand before them in the batch
    m2 = N.Model(N.POOL1, PORTS, N.STATICS)
    b0, ch0 = N.layout(out)
    pre = m2.run(b0, ch0, now=10)
    back = [N.reply((N.packet_after(b0, pre["slab"], i), out[i][1])) for i in range(len(out))]
    dirs = np.array([N.IN] * len(back) + [N.OUT] * len(out), np.uint8)
    got, want, b = run_both(nat, m, back + out, dir=dirs, now=10)
    assert (want["status"] == N.OK).all() and want["created"].sum() == 9
    for i, item in enumerate(out):
        p = N.packet_after(b, got["slab"], i)
        ipo, l4o = N.offsets(item)
        assert p[ipo + 16:ipo + 20] == item[0][ipo + 12:ipo + 16] and N.ip_valid(p, ipo) and N.l4_valid(p, ipo, l4o), i
    nat.close()


@pytest.mark.parametrize("which", [0, 1, N.LAST])
def test_vxlan_which_ip(P, which):
    nat, m = pair(P)
    got, want, _ = run_both(nat, m, [N.vxlan(), N.mk("TCP", "10.0.0.1", 1, N.REMOTE, 2)], which_ip=which)
    assert want["status"][0] == N.OK
    nat.close()


def test_exhaustion_expire_and_the_wrap_past_the_cursor(P):
    nat, m = pair(P, ports=(6000, 6003))
    flows = [N.mk("UDP", "10.0.0.%d" % (k + 1), 100, N.REMOTE, 53) for k in range(6)]
    items = [flows[k] for k in (0, 1, 2, 3, 4, 0, 4, 5, 4)] + [N.mk("TCP", "10.0.0.1", 100, N.REMOTE, 53)]
    got, want, _ = run_both(nat, m, items, now=100)
    assert list(want["status"]) == [N.OK] * 4 + [N.EXHAUSTED, N.OK, N.EXHAUSTED, N.EXHAUSTED, N.EXHAUSTED, N.OK]
    got, want, _ = run_both(nat, m, [flows[4], flows[1]], now=150)
    assert list(want["status"]) == [N.EXHAUSTED, N.OK]
    assert nat.expire(200, (0, 100, 0)) == 3 == m.expire(200, (0, 100, 0))
    got, want, _ = run_both(nat, m, [flows[4], flows[5], flows[4]], now=201)
    assert list(want["status"]) == [N.OK] * 3 and list(want["created"]) == [1, 1, 0]
    nat.close()
    # E = 3 x 1037, a multiple of neither 32 nor 1024; the cursor three entries before E; 1500 entries freed below it
    nat, m = pair(P, pool=["192.0.2.1", "192.0.2.2", "192.0.2.3"], ports=(2000, 3036), slots=1 << 13, static=N.STATICS[:1])
    udp = [N.mk("UDP", N.INSIDE + 1 + k // 50000, 1 + k % 50000, N.REMOTE, 53) for k in range(m.E - 3)]
    run_both(nat, m, udp[:1500], now=10, sessions=False)
    run_both(nat, m, udp[1500:] + [N.flow_item(0), N.flow_item(2)], now=20)
    assert m.cursor[1] == m.E - 3
    for now, idle, gone in ((29, (0, 20, 0), 0), (30, (0, 20, 20), 1500), (30, (0, 0, 0), 0), (2 ** 32 - 1, (2 ** 32 - 1, 0, 0), 0)):
        assert nat.expire(now, idle) == gone == m.expire(now, idle), (now, idle)
        N.same_sessions(nat.sessions(), m.sessions(), str(now))
    fresh = [N.mk("UDP", "10.200.0.1", 1 + k, N.REMOTE, 53) for k in range(40)]
    got, want, _ = run_both(nat, m, fresh + [N.mk("TCP", "10.9.9.9", 8080, N.REMOTE, 1), udp[1500], N.flow_item(0)], now=31)
    assert [int(e) - m.E for e in want["entry"][:40]] == [m.E - 3, m.E - 2, m.E - 1] + list(range(37))
    assert want["entry"][40] == N.STATIC and not want["created"][40:].any()
    nat.clear()
    m.clear()
    run_both(nat, m, fresh[:5], now=1)
    nat.close()


def test_table_full_by_invariants(P):
    args = (N.POOL1, PORTS, ())
    nat, m = pair(P, slots=64)
    early = [N.flow_item(k) for k in range(10)]
    run_both(nat, m, early, now=1)
    flows = [N.mk("UDP", "10.77.0.%d" % (1 + k % 200), 3000 + k, N.REMOTE, 53) for k in range(100)]
    items = flows + flows[::3]
    b, ch = N.layout(items)
    got = collect(launch(nat, b, ch, now=2), b)
    by_key, by_ent = N.invariants(got, b, ch, args, [N.OUT] * len(items))
    assert (got["status"] == N.TABLE_FULL).any() and (got["status"] == N.OK).any()
    assert int(got["hits"].sum()) == len(items) and got["hits"][N.OK] + got["hits"][N.TABLE_FULL] == len(items)
    assert sum(nat.count()) <= 64 and sum(nat.count()) == 10 + len(by_ent) and got["created"].sum() == len(by_ent)
    rec = {x.tobytes() for x in nat.sessions()}
    assert all(row.tobytes() in rec for row in m.sessions())
    b2, ch2 = N.layout(early)
    N.check(collect(launch(nat, b2, ch2, now=1), b2), m.run(b2, ch2, now=1))
    nat.close()


def test_no_write_and_null_outputs(P):
    items = [N.flow_item(k) for k in range(5)] + [N.statuses_items()[2][0]]
    b, ch = N.layout(items)
    nat, m = pair(P)
    got, want, _ = run_both(nat, m, items, now=7, write=False)
    assert np.array_equal(got["slab"], b["slab"]) and want["created"].sum() == 5
    for outs in ((), ("status",), ("entry", "created"), ("created",)):
        for counters in (None, True):
            nat.clear()
            m.clear()
            want = m.run(b, ch, now=1)
            db, big = dev_batch(b)
            r = nat.run(db, {k: dev(v) for k, v in ch.items()}, now=1, outputs=outs, counters=counters)
            import torch
            torch.cuda.synchronize()
            got = {k: None if getattr(r, k) is None else getattr(r, k).cpu().numpy() for k in N.NAMES + ("hits", "bytes")}
            got["slab"] = db["slab"].cpu().numpy()
            assert [nm for nm in N.NAMES if got[nm] is not None] == list(outs) and (got["hits"] is not None) == bool(counters)
            N.check(got, want, f"{outs} {counters}")
            N.same_sessions(nat.sessions(), m.sessions())
    nat.close()


# ------------------------------------------------------------------ the shapes where the kernels can go wrong
SHAPES = [1, 63, 64, 65, 3 * BLOCK + 1]


def new_flows(n, base=0):
    """n packets, every one a flow of its own, the three protocols interleaved unevenly (so that the per-protocol ranks
    cross waves and blocks at different places)."""
    return [N.mk(("TCP", "UDP", "UDP", "ICMP", "TCP", "UDP", "UDP")[k % 7], N.INSIDE + 1 + (base + k) // 60000, 1 + (base + k) % 60000,
                 N.REMOTE, 443, payload=b"") for k in range(n)]


@pytest.mark.parametrize("n", SHAPES)
def test_every_packet_its_own_new_flow(P, n):
    nat, m = pair(P, pool=["192.0.2.1", "192.0.2.2"], ports=(1000, 1299), slots=4096)
    run_both(nat, m, new_flows(7), now=1)  # the cursors do not start at 0
    got, want, _ = run_both(nat, m, new_flows(n, base=100), now=2)
    assert want["created"].sum() == n
    got, want, _ = run_both(nat, m, new_flows(n, base=100)[::-1], now=3)  # and they all hit
    assert not want["created"].any() and (want["status"] == N.OK).all()
    nat.close()


@pytest.mark.parametrize("n", SHAPES)
def test_all_packets_one_new_flow(P, n):
    nat, m = pair(P)
    got, want, _ = run_both(nat, m, [N.flow_item(1)] * n, kind="stride", now=2)
    assert list(want["created"]) == [1] + [0] * (n - 1) and (want["entry"] == m.E).all()
    nat.close()


def test_creators_only_in_the_last_block(P):
    nat, m = pair(P, slots=4096)
    old = new_flows(50)
    run_both(nat, m, old, now=1)
    n = 3 * BLOCK + 40
    items = [old[k % 50] for k in range(3 * BLOCK)] + new_flows(40, base=500)
    dirs = np.zeros(n, np.uint8)
    dirs[5:700:9] = 2  # some skipped ones among the hits
    got, want, _ = run_both(nat, m, items, dir=dirs, now=2)
    assert want["created"][:3 * BLOCK].sum() == 0 and want["created"][3 * BLOCK:].sum() == 40
    nat.close()


def test_two_calls_on_one_stream_with_no_sync_between(P):
    import torch
    nat, m = pair(P, slots=4096)
    a, b_ = new_flows(300), new_flows(300)[::-1] + new_flows(20, base=900)
    ba, ca = N.layout(a)
    bb, cb = N.layout(b_)
    wa, wb = m.run(ba, ca, now=1), m.run(bb, cb, now=2)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        qa = launch(nat, ba, ca, stream=s, now=1)
        qb = launch(nat, bb, cb, stream=s, now=2)
    ga, gb = collect(qa, ba), collect(qb, bb)
    N.check(ga, wa, "first")
    N.check(gb, wb, "second")
    assert wb["created"].sum() == 20 and not wb["created"][:300].any()
    N.same_sessions(nat.sessions(), m.sessions())
    nat.close()


def test_dir_given_and_dir_all(P):
    nat, m = pair(P)
    items = [N.flow_item(k) for k in range(6)]
    run_both(nat, m, items, dir=N.OUT, now=1)
    run_both(nat, m, items, dir=N.IN, now=2)  # the inside hosts' addresses are not ours
    run_both(nat, m, items, dir=np.array([0, 1, 2, 3, 0, 1], np.uint8), select=np.array([1, 1, 1, 1, 0, 1], np.uint8), now=3)
    nat.close()


_BIG = {}


def big_case():
    """2 x 10^4 packets over 3000 flows, both directions: built and modelled once."""
    if not _BIG:
        rng = np.random.default_rng(77)
        pool, ports = ["192.0.2.1", "192.0.2.2", "192.0.2.3"], (1024, 2100)
        flows = new_flows(3000)
        m = N.Model(pool, ports, N.STATICS)
        b0, ch0 = N.layout(flows, kind="stride")
        first = m.run(b0, ch0, now=0)  # what each flow becomes, for the replies
        replies = [N.reply((N.packet_after(b0, first["slab"], k), flows[k][1])) for k in range(0, 3000, 3)]
        m.clear()
        pick = rng.integers(0, 3000, 20000)
        inbound = rng.random(20000) < 0.25
        items, dirs = [], np.zeros(20000, np.uint8)
        for i in range(20000):
            if inbound[i]:
                items.append(replies[int(pick[i]) // 3])
                dirs[i] = N.IN
            else:
                items.append(flows[int(pick[i])])
        b, ch = N.layout(items)
        # (the model allocates in the batch's own order, so most replies find their flow under another entry or none:
        # OK, NO_SESSION and created all come up)
        want = m.run(b, ch, dir=dirs, now=9)
        _BIG.update(pool=pool, ports=ports, b=b, ch=ch, dirs=dirs, want=want, sessions=m.sessions())
    return _BIG


def test_20000_packets_over_3000_flows_twice_from_clear(P):
    c = big_case()
    nat = P.nat(c["pool"], c["ports"], 1 << 13, N.STATICS)
    seen = []
    for rep in range(2):
        got = collect(launch(nat, c["b"], c["ch"], dir=c["dirs"], now=9), c["b"])
        N.check(got, c["want"], f"run {rep}")
        seen.append(nat.sessions())
        N.same_sessions(seen[-1], c["sessions"], f"run {rep}")
        nat.clear()
    assert seen[0].tobytes() == seen[1].tobytes()
    assert {N.OK, N.NO_SESSION} <= set(c["want"]["status"]) and c["want"]["created"].sum() > 2000
    nat.close()


def chunk_case(reps, extra=300, stride=64):
    """16 * reps + extra packets: 16 flows tiled reps times, then `extra` new flows.  The expected outputs are the
    model's over the 16 + extra distinct packets, tiled the same way -> (batch, chain, want, the model)."""
    head, tail = new_flows(16), new_flows(extra, base=1000)
    m = N.Model(N.POOL1, PORTS)
    bs, chs = N.layout(head + tail, kind="stride", stride=stride)
    small = m.run(bs, chs, now=4)
    n = 16 * reps + extra

    def tiled(a, axis=-1):  # the first 16 columns reps times, then the rest
        a = np.asarray(a)
        h, t = np.take(a, range(16), axis), np.take(a, range(16, 16 + extra), axis)
        return np.concatenate([np.concatenate([h] * reps, axis), t], axis)
    rows = lambda a: tiled(a.reshape(-1, stride), 0).reshape(-1)  # noqa: E731
    b = C.batch(rows(bs["slab"]), lens=tiled(bs["lens"]), stride=stride, n=n)
    ch = {k: tiled(v) for k, v in chs.items()}
    want = {k: tiled(small[k]) for k in N.NAMES}
    want["created"][16:16 * reps] = 0
    want["slab"] = rows(small["slab"])
    want["hits"] = np.bincount(want["status"], minlength=N.NSTATUS).astype(np.uint64)
    want["bytes"] = np.bincount(want["status"], weights=b["lens"], minlength=N.NSTATUS).astype(np.uint64)
    return b, ch, want, m


def test_more_than_one_chunk(P):
    """2^20 + 300 packets: the first chunk of 2^20 holds 16 flows over and over, the second 300 new flows."""
    b, ch, want, m = chunk_case((1 << 20) // 16)
    nat = P.nat(N.POOL1, PORTS, 1 << 12)
    got = collect(launch(nat, b, ch, now=4), b)
    N.check(got, want, "two chunks")
    N.same_sessions(nat.sessions(), m.sessions())
    nat.close()


def test_a_chain_through_the_other_calls(P):
    """nat.run, then l4_checksum says L4_OK for every packet that was L4_OK before, and Forwarder.run and pcap_write
    take the batch with the same chain columns."""
    import torch
    nat, m = pair(P, slots=4096)
    items = new_flows(200) + [N.mk("UDP", "10.3.0.1", 9, N.REMOTE, 53, good=False), N.mk("UDP", "10.3.0.2", 9, N.REMOTE, 53, udp_none=True)]
    b, ch = N.layout(items)
    db, big = dev_batch(b)
    dch = {k: dev(v) for k, v in ch.items()}
    args = dict(offsets=db["offsets"], lens=db["lens"])
    before = P.l4_checksum(db["slab"], dch, which=pktgpu.L4_LAST, **args)["status"].cpu().numpy()
    r = nat.run(db, dch, now=1)
    after = P.l4_checksum(db["slab"], dch, which=pktgpu.L4_LAST, **args)["status"].cpu().numpy()
    assert (r.status.cpu().numpy() == N.OK).all()
    assert np.array_equal(before, after) and (before == schema.L4_OK).sum() == 200
    fwd = P.forwarder(W.adj_array([W.adjacency(0)]))
    f = fwd.run(db, dch, nexthop=torch.zeros(b["n"], dtype=torch.uint32, device="cuda"))
    assert (f["status"].cpu().numpy() == pktgpu.FWD_OK).all()
    out = P.pcap_write(db["slab"], offsets=db["offsets"], lens=db["lens"])
    torch.cuda.synchronize()
    assert out is not None and guards_intact(big, b["slab"].size)
    want = m.run(b, ch, now=1)
    ext = C.extents(b)
    slab = db["slab"].cpu().numpy()
    for i in (0, 1, 2, 199, 201):  # the translated source address survived the forwarder
        ipo = N.offsets(items[i])[0]
        o = ext[i][0] + ipo + 12
        assert bytes(slab[o:o + 4]) == bytes(want["slab"][o:o + 4]) == N.ip(N.POOL1[0])
    nat.close()


def test_refusal_texts_through_the_ctx(P):
    from pktgpu import _lib
    L = P._L
    err = lambda: L.pkt_ctx_last_error(P._ctx).decode()  # noqa: E731
    for kw, text in ((dict(pool=[]), "naddr not in 1..64"), (dict(slots=100), "slots not a power of two in 64..2^26"),
                     (dict(ports=(5, 4)), "ports not 1 <= port_lo <= port_hi <= 65535"),
                     (dict(static=[("udp", "10.0.0.1", 1, N.POOL1[0], PORTS[0])]), "a static's outside endpoint is a dynamic pool entry")):
        args = dict(pool=N.POOL1, ports=PORTS, slots=1024, static=())
        args.update(kw)
        with pytest.raises(RuntimeError):
            P.nat(**args)
        assert err() == "pkt_nat_create: " + text
    nat = P.nat(N.POOL1, PORTS, 64)
    b, ch = N.layout([N.flow_item(0)])
    db, big = dev_batch(b)
    dch = {k: dev(v) for k, v in ch.items()}
    pb = P._batch(db["slab"], db["n"], db["stride"], db["offsets"], db["lens"])
    pc = P._chain(dch)

    def call(batch=pb, chain=pc, which=0, flags=0, dir_all=0, hits=None):
        return L.pkt_nat_batch(nat._t, ctypes.byref(batch), ctypes.byref(chain), which, flags, dir_all, None, None, 0, None, None,
                               None, hits, None, None)
    odd = P._batch(db["slab"][1:], 1, None, db["offsets"], db["lens"])
    h = dev(np.zeros(13, np.uint64))
    for kw, text in ((dict(which=16), "which_ip is neither below 16 nor PKT_FLOW_LAST"), (dict(flags=4), "unknown flag bits"),
                     (dict(dir_all=2), "dir_all is neither PKT_NAT_OUT nor PKT_NAT_IN"), (dict(batch=odd), "slab not 16-byte aligned"),
                     (dict(hits=h.data_ptr() + 4), "hits / bytes not 8-byte aligned"),
                     (dict(chain=_lib.PktChain(None, pc.hdr_type, pc.hdr_off)), "null chain column")):
        assert call(**kw) != 0
        assert err() == "pkt_nat_batch: " + text == L.pkt_nat_last_error(nat._t).decode(), kw
    assert nat.count() == (0, 0, 0)
    assert call() == 0
    import torch
    torch.cuda.synchronize()
    assert nat.count() == (1, 0, 0)
    empty = P._batch(db["slab"], 0, 64, None, None)
    assert call(batch=empty) == 0
    nat.close()
