"""Every host twin that takes a pkt_batch_t, over packets that lie past 2^31 and 2^32 bytes into their slab (far_cases).
The slab is a view 2 GiB into an untouched anonymous mapping of about 6 GiB; only the pages of the packets, their decoys
and the guard bands are written (under 64 MiB).  Expected values are each call's own model over the same packets in
their compact layout: nothing here is compared with the code under test.  A truncated or sign-extended offset reads
or rewrites a decoy: a wrong output, or a decoy or guard band that changed."""
import numpy as np
import pytest

import pktgpu

import far_cases as FC

PLANS = ["indexed_ascending", "stride_1MiB"]
pytestmark = pytest.mark.parametrize("plan", PLANS)


def far(pl):
    """The placement written into a fresh mapping -> (alloc, far batch dict)."""
    assert FC.touched_bytes(pl) < 64 << 20
    keep, alloc = FC.host_alloc(pl)
    return alloc, pl.batch(FC.write(pl, alloc))


def kw(fb):
    return dict(stride=fb["stride"], n=fb["n"], offsets=fb["offsets"], lens=fb["lens"])


def test_pcap_write(plan):
    c = FC.build("pcap_write", plan)
    alloc, fb = far(c["pl"])
    pc = c["c"]
    cap, k, offs, lens, src = pktgpu.pcap_write(fb["slab"], select=pc["select"], snaplen=pc["snaplen"], ts=pc["ts"], **kw(fb))
    want, w_off, w_len, w_src = c["want"]
    assert cap.tobytes() == want and k == len(w_src)
    assert np.array_equal(offs, w_off) and np.array_equal(lens, w_len) and np.array_equal(src, w_src)
    FC.check(c["pl"], alloc)


@pytest.mark.parametrize("where", ["a_far", "b_far", "both_far"])
def test_compare(plan, where):
    import compare_cases as C
    c = FC.build("compare", plan)
    a, b = c["b"], c["b2"]
    checks = []
    if where != "b_far":
        alloc, a = far(c["pl"])
        checks.append((c["pl"], alloc))
    if where != "a_far":
        alloc, b = far(c["pl_b2"])
        checks.append((c["pl_b2"], alloc))
    C.check(pktgpu.compare(a, b, c["ignore"], c["chain"]), c["want"], where)
    for pl, alloc in checks:
        FC.check(pl, alloc)


@pytest.mark.parametrize("where", ["src_far", "both_far"])
def test_edit(plan, where):
    import edit_cases as E
    c = FC.build("edit", plan)
    ec, src = c["c"], c["b"]
    outs, w_len, w_status, w_chain = c["want"]
    alloc, src = far(c["pl"])
    if where == "src_far":
        dst, dst_offsets = np.full(ec["dst_len"], E.FILL, np.uint8), None
    else:
        pld = FC.slots(plan, FC.EDIT_SLOT)
        alloc_d, fd = far(pld)
        dst, dst_offsets = fd["slab"], np.array(pld.offs, np.uint64)
    got = pktgpu.edit(src["slab"], c["parsed"], ec["ops"], select=ec["select"], dst=dst, dst_offsets=dst_offsets,
                      slot=ec["slot"], **kw(src))
    if where == "src_far":
        E.check(ec, got, c["want"], where)
    else:
        E.check(dict(ec, dst_len=0), (dst[:0], got[1], got[2], got[3]), ([None] * pld.n, w_len, w_status, w_chain), where)
        FC.check(pld, alloc_d, after=[bytes(FC.EDIT_SLOT) if v is None else v + bytes(FC.EDIT_SLOT - len(v)) for v in outs], label=where)
    FC.check(c["pl"], alloc)


@pytest.mark.parametrize("update", [False, True], ids=["verify", "update"])
def test_l4_checksum(plan, update):
    import l4_cases as L4
    c = FC.build("l4_checksum", plan)
    alloc, fb = far(c["pl"])
    got = pktgpu.l4_checksum(fb["slab"], c["chain"], c["which"], update, **kw(fb))
    want = c["want_update"] if update else c["want"]
    L4.check(got, want, plan)
    after = FC.packets_of(c["b"], want["slab"])
    assert not update or after != FC.packets_of(c["b"])
    FC.check(c["pl"], alloc, after)


def test_flow_keys(plan):
    import flow_cases as F
    c = FC.build("flow_keys", plan)
    alloc, fb = far(c["pl"])
    o = c["opt"]
    F.check(pktgpu.flow_keys(fb["slab"], c["chain"], o["which_ip"], o["symmetric"], o["ports"], F.SEED, F.RSS_KEY, **kw(fb)),
            c["want"], plan)
    FC.check(c["pl"], alloc)


def test_match(plan):
    import match_cases as M
    c = FC.build("match", plan)
    alloc, fb = far(c["pl"])
    prog = c["prog"]
    got = pktgpu.match(fb["slab"], c["chain"], M.to_ctypes(prog), prog["default"], hits=True, bytes=True, **kw(fb))
    M.check(got, c["want"], plan)
    FC.check(c["pl"], alloc)


def test_reorder(plan):
    c = FC.build("reorder", plan)
    alloc, fb = far(c["pl"])
    r = pktgpu.reorder(c["perm"], fb["slab"], columns=c["cols"], slot=c["slot"], **kw(fb))
    FC.check_reorder(c, r["slab"], r["lens"], r["columns"], plan)
    FC.check(c["pl"], alloc)


def test_lpm_lookup(plan):
    import lpm_cases as X
    c = FC.build("lpm", plan)
    alloc, fb = far(c["pl"])
    X.check(pktgpu.Lpm(None, X.to_array(c["routes"]), X.DEFAULT).lookup(fb, c["chain"]), c["want"], plan)
    FC.check(c["pl"], alloc)


@pytest.mark.parametrize("call", ["fwd", "fwd_lpm"])
def test_fwd(plan, call):
    import fwd_cases as W
    import lpm_cases as X
    c = FC.build(call, plan)
    fc = c["c"]
    alloc, fb = far(c["pl"])
    lpm = pktgpu.Lpm(None, X.to_array(fc["routes"]), W.LPM_DEFAULT) if call == "fwd_lpm" else None
    got = pktgpu.Forwarder(None, W.adj_array(fc["adj"])).run(fb, c["chain"], nexthop=fc["nexthop"], lpm=lpm, which_ip=fc["which"],
                                                             keep_l2=fc["keep_l2"], select=fc["select"], outputs=W.NAMES,
                                                             hits=True, bytes=True)
    W.check(got, c["want"], call)
    after = FC.packets_of(c["b"], c["want"]["slab"])
    assert after != FC.packets_of(c["b"])
    FC.check(c["pl"], alloc, after)


def test_frag(plan):
    import frag_cases as G
    c = FC.build("frag", plan)
    alloc, fb = far(c["pl"])
    rc, got = G.host_call(fb, c["chain"], c["mtu"], c["select"])
    assert rc == 0 and got["guards"]
    G.check(got, c["want"], got["cap"], plan)
    FC.check(c["pl"], alloc)


def test_reasm(plan):
    import reasm_cases as R
    c = FC.build("reasm", plan)
    pl, want = c["pl"], c["want"]
    # some datagram is joined from members on both sides of 2^32
    sides = {}
    for i, q in enumerate(want["out_index"]):
        if want["status"][i] == R.JOINED:
            sides.setdefault(int(q), set()).add(pl.offs[i] >= FC.B32)
    assert any(len(s) == 2 for s in sides.values())
    alloc, fb = far(pl)
    rc, got = R.host_call(fb, c["chain"], c["select"])
    assert rc == 0 and got["guards"]
    R.check(got, want, got["cap"], plan)
    FC.check(pl, alloc)


def test_icmp_err(plan):
    import icmp_cases as I
    c = FC.build("icmp_err", plan)
    alloc, fb = far(c["pl"])
    rc, got = I.host_call(fb, c["chain"], c["code"], c["cf"], c["mtu"], c["cmap"], c["select"], 0)
    assert rc == 0 and got["guards"]
    I.check(got, c["want"], got["cap"], plan)
    FC.check(c["pl"], alloc)


@pytest.mark.parametrize("region", ["packet", "payload"])
def test_scan(plan, region):
    import scan_cases as S
    c = FC.build("scan_" + region, plan)
    sc_case = c["c"]
    alloc, fb = far(c["pl"])
    sc = pktgpu.Scanner(None, S.tables(sc_case["pats"]), default=sc_case["default"])
    r = sc.run(fb, c["chain"], region, sc_case["select"], hits=True)
    S.check({k: getattr(r, k) for k, _ in S.OUTPUTS + (("hits", None),)}, c["want"], region)
    assert (c["want"]["status"] == S.HIT).sum() > pl_n(c) // 4
    FC.check(c["pl"], alloc)


def pl_n(c):
    return c["pl"].n


def test_nat_out_then_in(plan):
    import nat_cases as NA
    c = FC.build("nat", plan)
    nat = pktgpu.Nat(None, NA.POOL1, FC.PORTS, 1024)
    for key, b, ch, want, args in (("pl", c["b"], c["chain"], c["want"], dict(dir=c["dir"], select=c["select"], now=5)),
                                   ("pl_b_in", c["b_in"], c["chain_in"], c["want_in"], dict(dir=NA.IN, now=9))):
        alloc, fb = far(c[key])
        r = nat.run(fb, ch, counters=True, **args)
        NA.check(dict(status=r.status, entry=r.entry, created=r.created, hits=r.hits, bytes=r.bytes), want, key)
        after = FC.packets_of(b, want["slab"])
        assert after != FC.packets_of(b)
        FC.check(c[key], alloc, after, key)
    NA.same_sessions(nat.sessions(), c["sessions"])
