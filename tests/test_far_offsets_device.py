"""Every device entry point that takes a pkt_batch_t, over packets that lie past 2^31 and 2^32 bytes into their slab
(far_cases: three plans).  The slab is a view 2 GiB into one module-wide device allocation of about 6 GiB, filled with
0xA5 before each test; a second one serves the calls with a far destination.  Expected values are each call's own
model (or the oracle) over the same packets in their compact layout.  After a call the packets and decoys are gathered
back by extent and compared (in-place calls: the packets rewritten, the decoys as written), then those extents are
overwritten with 0xA5 and the whole allocation, front area included, must be 0xA5 again, compared as 64-bit words on
the device: a stray store anywhere is seen.  A truncated or sign-extended offset lands on a decoy, inside the
allocation: a wrong answer, never a fault."""
import numpy as np
import pytest

import pktgpu

import far_cases as FC

pytestmark = [pytest.mark.gpu, pytest.mark.parametrize("plan", FC.PLANS)]
CAP = (FC.FRONT + (FC.N["stride_1MiB"] + 1) * FC.STRIDE + 15) // 16 * 16  # every plan's alloc_len fits
WORD = int.from_bytes(bytes([FC.FILL]) * 8, "little", signed=True)
CHUNK = 1 << 27  # words compared at a time


@pytest.fixture(scope="module")
def P():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible")
    return pktgpu.Parser(0)


@pytest.fixture(scope="module")
def mem(P):
    """The two allocations; freed at module end."""
    import torch
    bufs = []
    try:
        for _ in range(2):
            bufs.append(torch.empty(CAP, dtype=torch.uint8, device="cuda"))
    except Exception as e:  # no skip: a box that cannot hold them fails
        pytest.fail(f"allocating 2 x {CAP} bytes failed ({e}); torch.cuda.mem_get_info() = {torch.cuda.mem_get_info()}")
    assert all(t.data_ptr() % 16 == 0 for t in bufs)
    yield bufs
    del bufs[:]
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def refill(mem):
    for a in mem:
        a.fill_(FC.FILL)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def h(t):
    return None if t is None else t.cpu().numpy()


def hd(d):
    return {k: h(v) for k, v in d.items()}


def whole_is_fill(a, label):
    import torch
    v = a.view(torch.int64)
    for s in range(0, v.numel(), CHUNK):
        bad = (v[s:s + CHUNK] != WORD).nonzero()
        assert bad.numel() == 0, (label, "a byte outside the packets' and decoys' extents changed: first word", s + int(bad[0]))


class Far:
    """A placement written into allocation `a` -> .batch, the far batch of device tensors.  content=False writes
    nothing (a far destination: its extents start as fill)."""

    def __init__(self, a, pl, content=True):
        assert pl.alloc_len <= a.numel()
        self.a, self.pl = a, pl
        pos, val, self.pb, self.db = pl.index()
        if not content:  # the slots alone
            pos, val = pos[:self.pb[-1]], np.full(self.pb[-1], FC.FILL, np.uint8)
        self.pos, self.val = dev(pos), val
        if content:
            a[self.pos] = dev(val)
        self.slab = a[FC.FRONT:FC.FRONT + pl.slab_len]
        self.batch = dict(slab=self.slab, n=pl.n, stride=pl.stride, lens=dev(pl.lens),
                          offsets=None if pl.offsets is None else dev(pl.offsets))
        self.kw = {k: v for k, v in self.batch.items() if k != "slab"}

    def verify(self, after=None, label=""):
        """The packets' extents hold after[i] (default: what was written; a shorter after[i] is followed by what
        was there), the decoys theirs, and nothing else in the allocation changed."""
        import torch
        torch.cuda.synchronize()
        got, want = h(self.a[self.pos]), self.val.copy()
        for i, d in enumerate(after or ()):
            want[self.pb[i]:self.pb[i] + len(d)] = np.frombuffer(d, np.uint8)
        bad = np.flatnonzero(got != want)
        if bad.size:
            k = int(bad[0])
            if k < self.pb[-1]:
                raise AssertionError((label, self.pl.plan, "bytes of packet", int(np.searchsorted(self.pb, k, "right")) - 1))
            d = int(np.searchsorted(self.db, k, "right")) - 1
            raise AssertionError((label, self.pl.plan, "the decoy of packet", self.pl.decoy_of[d], "was written"))
        self.a[self.pos] = FC.FILL
        whole_is_fill(self.a, (label, self.pl.plan))


def chain_dev(ch):
    return None if ch is None else {k: dev(v) for k, v in ch.items()}


def compact_dev(b):
    return dict(slab=dev(b["slab"]), n=b["n"], stride=b["stride"], lens=None if b["lens"] is None else dev(b["lens"]),
                offsets=None if b["offsets"] is None else dev(b["offsets"]))


def kw(b):
    return {k: v for k, v in b.items() if k != "slab"}


# ------------------------------------------------------------------ parse
def same_columns(g, o, label):
    from pktgpu import schema
    for k, ov in o.items():
        gv = g[k]
        if k in ("hdr_type", "hdr_off"):
            valid = np.arange(schema.MAX_HDRS)[:, None] < o["n_hdrs"].astype(np.int64)[None, :]
            bad = np.nonzero(valid & (gv != ov))
            assert bad[0].size == 0, (label, k, "slot", bad[0][:5], "packet", bad[1][:5])
        else:
            bad = np.nonzero((gv != ov).reshape(len(ov), -1).any(axis=1))[0]
            assert bad.size == 0, (label, k, "first packets", bad[:8], gv[bad[:4]], ov[bad[:4]])


def oracle_columns(b):
    import oracle
    return oracle.parse_batch(b["slab"], b["n"], offsets=b["offsets"], lens=b["lens"], columns=pktgpu.resolve_columns("all"),
                              nthreads=8)


def test_parse_indexed_all_columns(P, mem, plan):
    c = FC.build("parse", plan)
    f = Far(mem[0], c["pl"])
    res = P.parse(f.slab, columns="all", **f.kw)
    same_columns(hd(res), oracle_columns(c["b"]), "parse")
    f.verify()


def test_parse_batches_one_far_among_near(P, mem, plan):
    c = FC.build("parse", plan)
    f = Far(mem[0], c["pl"])
    near = compact_dev(c["b"])
    tup = lambda b: (b["slab"], b["n"], b["stride"], b["offsets"], b["lens"])  # noqa: E731
    outs = [P.alloc(c["b"]["n"], "all") for _ in range(3)]
    P.parse_batches([tup(near), tup(f.batch), tup(near)], outs)
    want = oracle_columns(c["b"])
    for k, o in enumerate(outs):
        same_columns(hd(o), want, f"batch {k}")
    f.verify()


# ------------------------------------------------------------------ field and checksum rewrites
def test_extract_fields(P, mem, plan):
    c = FC.build("rewrite", plan)
    f = Far(mem[0], c["pl"])
    vals, found = P.extract_fields(f.slab, chain_dev(c["chain"]), c["specs"], **f.kw)
    w_vals, w_found = c["want_get"]
    for k, sp in enumerate(c["specs"]):
        assert np.array_equal(h(found[k]), w_found[k]), ("found", sp)
        assert np.array_equal(h(vals[k]), w_vals[k]), ("values", sp)
    assert sum(int(x.sum()) for x in w_found) > c["b"]["n"]
    f.verify()


@pytest.mark.parametrize("call", ["set_fields", "set_fields_csum", "ipv4_update_checksum"])
def test_setters(P, mem, plan, call):
    c = FC.build("rewrite", plan)
    f = Far(mem[0], c["pl"])
    ch = chain_dev(c["chain"])
    if call == "ipv4_update_checksum":
        P.ipv4_update_checksum(f.slab, ch, 0, **f.kw)
        want = c["want_update"]
    else:
        P.set_fields(f.slab, ch, c["specs"], [dev(v) for v in c["values"]], ipv4_checksum=0 if call.endswith("csum") else None,
                     **f.kw)
        want = c["want_csum"] if call.endswith("csum") else c["want_set"]
    after = FC.packets_of(c["b"], want)
    assert after != FC.packets_of(c["b"])
    f.verify(after, call)


# ------------------------------------------------------------------ whole-packet calls
WHERE = ["src_far", "dst_far", "both_far"]


def far_dst(mem, plan):
    """The destination slots of to_vec / edit in the second allocation -> (Far, dst view, dst_offsets)."""
    pld = FC.slots(plan, FC.EDIT_SLOT)
    d = Far(mem[1], pld, content=False)
    return d, d.slab, dev(np.array(pld.offs, np.uint64))


@pytest.mark.parametrize("where", WHERE)
def test_to_vec(P, mem, plan, where):
    import torch

    import oracle
    c = FC.build("parse", plan)
    b, n, slot = c["b"], c["b"]["n"], FC.EDIT_SLOT
    want, wl = oracle.round_trip_batch(b["slab"], n, offsets=b["offsets"], lens=b["lens"], slow=True, nthreads=8)
    outs = [want[int(o):int(o) + int(k)].tobytes() for o, k in zip(b["offsets"], wl)]
    assert max(len(v) for v in outs) <= slot and sum(len(v) for v in outs) > 40 * n
    f = Far(mem[0], c["pl"]) if where != "dst_far" else None
    src = f.batch if f else compact_dev(b)
    if where == "src_far":
        d, dst, doff = None, torch.full((n * slot,), 0xEE, dtype=torch.uint8, device="cuda"), dev(np.arange(n, dtype=np.uint64) * slot)
    else:
        d, dst, doff = far_dst(mem, plan)
    out, ln = P.to_vec(src["slab"], chain_dev(c["parsed"]), dst=dst, dst_offsets=doff, **kw(src))
    assert np.array_equal(h(ln), wl)
    if d is None:
        o = h(out).reshape(n, slot)
        for i, v in enumerate(outs):
            assert o[i, :len(v)].tobytes() == v and (o[i, len(v):] == 0xEE).all(), i
    else:
        d.verify(outs, where)
    if f:
        f.verify(None, where)


@pytest.mark.parametrize("where", WHERE)
def test_edit(P, mem, plan, where):
    import torch

    import edit_cases as E
    c = FC.build("edit", plan)
    ec, b = c["c"], c["b"]
    outs, w_len, w_status, w_chain = c["want"]
    f = Far(mem[0], c["pl"]) if where != "dst_far" else None
    src = f.batch if f else compact_dev(b)
    if where == "src_far":
        d, dst, doff = None, torch.full((ec["dst_len"],), E.FILL, dtype=torch.uint8, device="cuda"), None
    else:
        d, dst, doff = far_dst(mem, plan)
    got = P.edit(src["slab"], chain_dev(c["parsed"]), ec["ops"], select=dev(ec["select"]), dst=dst, dst_offsets=doff,
                 slot=ec["slot"], **kw(src))
    got = (h(got[0]) if d is None else np.zeros(0, np.uint8), h(got[1]), h(got[2]), hd(got[3]))
    if d is None:
        E.check(ec, got, c["want"], where)
    else:
        E.check(dict(ec, dst_len=0), got, ([None] * b["n"], w_len, w_status, w_chain), where)
        d.verify([v or b"" for v in outs], where)
    assert (w_status == E.OK).sum() > b["n"] // 2
    if f:
        f.verify(None, where)


@pytest.mark.parametrize("where", ["a_far", "b_far", "both_far"])
def test_compare(P, mem, plan, where):
    import compare_cases as C
    c = FC.build("compare", plan)
    fa = Far(mem[0], c["pl"]) if where != "b_far" else None
    fb = Far(mem[1], c["pl_b2"]) if where != "a_far" else None
    a = fa.batch if fa else compact_dev(c["b"])
    b = fb.batch if fb else compact_dev(c["b2"])
    res, mt, fd, sm = P.compare(a, b, c["ignore"], chain_dev(c["chain"]))
    C.check((h(res), h(mt), h(fd), sm), c["want"], where)
    assert {C.EQUAL, C.BYTES} <= set(c["want"][0].tolist())
    for f in (fa, fb):
        if f:
            f.verify(None, where)


def test_pcap_write(P, mem, plan):
    c = FC.build("pcap_write", plan)
    f = Far(mem[0], c["pl"])
    pc = c["c"]
    cap, k, offs, lens, src = P.pcap_write(f.slab, select=dev(pc["select"]), snaplen=pc["snaplen"],
                                           ts=(dev(pc["ts"][0]), dev(pc["ts"][1])), **f.kw)
    want, w_off, w_len, w_src = c["want"]
    assert h(cap).tobytes() == want and k == len(w_src)
    assert np.array_equal(h(offs), w_off) and np.array_equal(h(lens), w_len) and np.array_equal(h(src), w_src)
    f.verify()


@pytest.mark.parametrize("update", [False, True], ids=["verify", "update"])
def test_l4_checksum(P, mem, plan, update):
    import l4_cases as L4
    c = FC.build("l4_checksum", plan)
    f = Far(mem[0], c["pl"])
    got = P.l4_checksum(f.slab, chain_dev(c["chain"]), c["which"], update, **f.kw)
    want = c["want_update"] if update else c["want"]
    L4.check(hd(got), want, plan)
    after = FC.packets_of(c["b"], want["slab"])
    assert not update or after != FC.packets_of(c["b"])
    f.verify(after)


def test_flow_keys_with_rss(P, mem, plan):
    import flow_cases as F
    c = FC.build("flow_keys", plan)
    f = Far(mem[0], c["pl"])
    o = c["opt"]
    got = P.flow_keys(f.slab, chain_dev(c["chain"]), o["which_ip"], o["symmetric"], o["ports"], F.SEED, F.RSS_KEY, **f.kw)
    assert "rss" in got
    F.check(hd(got), c["want"], plan)
    f.verify()


def test_match_all_six_outputs(P, mem, plan):
    import match_cases as M
    c = FC.build("match", plan)
    f = Far(mem[0], c["pl"])
    prog = c["prog"]
    mp = P.match_program(M.to_ctypes(prog), prog["default"])
    got = hd(P.match(f.slab, chain_dev(c["chain"]), mp, hits=True, bytes=True, **f.kw))
    assert set(got) == set(M.OUT)
    M.check(got, c["want"], plan)
    f.verify()
    mp.close()


def test_reorder_far_source(P, mem, plan):
    c = FC.build("reorder", plan)
    f = Far(mem[0], c["pl"])
    r = P.reorder(dev(c["perm"]), f.slab, columns=chain_dev(c["cols"]), slot=c["slot"], **f.kw)
    FC.check_reorder(c, h(r["slab"]), h(r["lens"]), hd(r["columns"]), plan)
    f.verify()


# ------------------------------------------------------------------ the routing path
def test_lpm_lookup(P, mem, plan):
    import lpm_cases as X
    c = FC.build("lpm", plan)
    f = Far(mem[0], c["pl"])
    lpm = P.lpm(X.to_array(c["routes"]), X.DEFAULT)
    X.check(hd(lpm.lookup(f.batch, chain_dev(c["chain"]))), c["want"], plan)
    f.verify()
    lpm.close()


@pytest.mark.parametrize("call", ["fwd", "fwd_lpm"])
def test_forwarder(P, mem, plan, call):
    import fwd_cases as W
    import lpm_cases as X
    c = FC.build(call, plan)
    fc = c["c"]
    f = Far(mem[0], c["pl"])
    lpm = P.lpm(X.to_array(fc["routes"]), W.LPM_DEFAULT) if call == "fwd_lpm" else None
    fwd = P.forwarder(W.adj_array(fc["adj"]))
    got = fwd.run(f.batch, chain_dev(c["chain"]), nexthop=None if lpm else dev(fc["nexthop"]), lpm=lpm, which_ip=fc["which"],
                  keep_l2=fc["keep_l2"], select=None if fc["select"] is None else dev(fc["select"]), outputs=W.NAMES,
                  hits=True, bytes=True)
    W.check(hd(got), c["want"], call)
    after = FC.packets_of(c["b"], c["want"]["slab"])
    assert after != FC.packets_of(c["b"])
    f.verify(after, call)
    fwd.close()
    if lpm:
        lpm.close()


def produced(r, per_packet, extra=None):
    """A FragResult / ReasmResult / IcmpErrResult as the dict frag_cases.check and its kin take, and its out_cap."""
    got = {k: h(getattr(r, k)) for k in per_packet + ("hits",)}
    got.update(n_out=r.n_out, bytes_out=r.bytes_out, dst=h(r.slab), out_off=h(r.offsets), out_len=h(r.lens),
               src_index=h(r.src_index), oc_n_hdrs=h(r.out_chain["n_hdrs"]), oc_hdr_type=h(r.out_chain["hdr_type"]).reshape(-1),
               oc_hdr_off=h(r.out_chain["hdr_off"]).reshape(-1))
    if extra:
        got[extra] = h(getattr(r, extra))
    return got, r.offsets.numel()


def test_fragment(P, mem, plan):
    import frag_cases as G
    c = FC.build("frag", plan)
    f = Far(mem[0], c["pl"])
    r = P.fragment(f.batch, chain_dev(c["chain"]), mtu=dev(c["mtu"]), select=dev(c["select"]), hits=True)
    got, cap = produced(r, ("status", "nfrag", "first"), "frag_index")
    G.check(got, c["want"], cap, plan)
    assert (got["dst"][c["want"]["bytes_out"]:] == 0).all() and (c["want"]["status"] == G.SPLIT).sum() > 3
    f.verify()


def test_reassemble_members_on_both_sides_of_4gib(P, mem, plan):
    import reasm_cases as R
    c = FC.build("reasm", plan)
    pl, want = c["pl"], c["want"]
    sides = {}
    for i in np.flatnonzero(want["status"] == R.JOINED):
        sides.setdefault(int(want["out_index"][i]), set()).add(pl.offs[i] >= FC.B32)
    assert any(len(s) == 2 for s in sides.values())
    f = Far(mem[0], pl)
    r = P.reassemble(f.batch, chain_dev(c["chain"]), select=dev(c["select"]), hits=True)
    got, cap = produced(r, ("status", "out_index"), "nfrag")
    R.check(got, want, cap, plan)
    assert (got["dst"][want["bytes_out"]:] == 0).all()
    f.verify()


def test_icmp_errors(P, mem, plan):
    import icmp_cases as I
    c = FC.build("icmp_err", plan)
    cf = c["cf"]
    f = Far(mem[0], c["pl"])
    r = P.icmp_errors(f.batch, chain_dev(c["chain"]), fwd_status=dev(c["code"]), mtu=dev(c["mtu"]), src4=bytes(cf["src4"]),
                      src6=bytes(cf["src6"]), ttl=cf["ttl"], tos=cf["tos"], max4=cf["max4"], max6=cf["max6"], ident=cf["ident"],
                      select=dev(c["select"]), hits=True)
    got, cap = produced(r, ("status", "out_index"))
    I.check(got, c["want"], cap, plan)
    assert (got["dst"][c["want"]["bytes_out"]:] == 0).all() and c["want"]["n_out"] > c["b"]["n"] // 8
    f.verify()


@pytest.mark.parametrize("region", ["packet", "payload"])
def test_scanner(P, mem, plan, region):
    import scan_cases as S
    c = FC.build("scan_" + region, plan)
    sc_case = c["c"]
    f = Far(mem[0], c["pl"])
    sc = P.scanner(S.tables(sc_case["pats"]), default=sc_case["default"])
    r = sc.run(f.batch, chain_dev(c["chain"]), region, None, hits=True)
    S.check({k: h(getattr(r, k)) for k, _ in S.OUTPUTS + (("hits", None),)}, c["want"], region)
    assert (c["want"]["status"] == S.HIT).sum() > c["b"]["n"] // 4
    f.verify()
    sc.close()


def test_nat_out_then_in(P, mem, plan):
    import nat_cases as NA
    c = FC.build("nat", plan)
    nat = P.nat(NA.POOL1, FC.PORTS, 1024)
    for a, key, b, ch, want, args in ((mem[0], "pl", c["b"], c["chain"], c["want"], dict(dir=dev(c["dir"]), select=dev(c["select"]), now=5)),
                                      (mem[1], "pl_b_in", c["b_in"], c["chain_in"], c["want_in"], dict(dir=NA.IN, now=9))):
        f = Far(a, c[key])
        r = nat.run(f.batch, chain_dev(ch), counters=True, **args)
        NA.check({k: h(getattr(r, k)) for k in NA.NAMES + ("hits", "bytes")}, want, key)
        after = FC.packets_of(b, want["slab"])
        assert after != FC.packets_of(b)
        f.verify(after, key)
    NA.same_sessions(nat.sessions(), c["sessions"])
    nat.close()
