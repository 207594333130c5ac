"""pkt_fwd_create / pkt_fwd_batch (Parser.forwarder / Forwarder.run): the kernel of pktgpu_fwd.hip against fwd_cases'
yardstick (an independent Python model) and the host twin pkt_fwd_host.  The decision and the checksum arithmetic are
covered on the CPU (test_fwd_host.py: the host twin runs the same inline code); here it is the loads, the launch shape,
the stores and the counters.  The slab and every output lie between two guard regions filled with 0xA5, the outputs
start as 0x77 and the whole slab is compared, so that a byte the call must not write is seen."""
import ctypes

import numpy as np
import pytest

import pktgpu
from pktgpu import schema

import compare_cases as C
import lpm_cases as X
import fwd_cases as W

pytestmark = pytest.mark.gpu
GUARD = 4096
FILL = 0x77
FILL64 = 0x7777777777777777
SHAPES = [1, 63, 64, 65, 257, 4096]
OUTS = W.NAMES + ("hits", "bytes")
ODT = dict(W.DT, hits=np.uint64, bytes=np.uint64)


@pytest.fixture(scope="module")
def P():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible")
    return pktgpu.Parser(0)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def guarded(nbytes, fill=None, shift=0):
    """A 0xA5-filled allocation with `nbytes` in its middle (filled with `fill`) -> (all, middle)."""
    import torch
    big = torch.full((GUARD + shift + (nbytes + 15) // 16 * 16 + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    mid = big[GUARD + shift:GUARD + shift + nbytes]
    if fill is not None:
        mid.fill_(fill)
    return big, mid


def guards_intact(big, mid):
    lo = mid.data_ptr() - big.data_ptr()
    return bool((big[:lo] == 0xA5).all()) and bool((big[lo + mid.numel():] == 0xA5).all())


def dev_batch(b):
    big, slab = guarded(b["slab"].size)
    slab.copy_(dev(b["slab"]))
    kw = dict(slab=slab, n=b["n"], stride=b["stride"], offsets=None if b["offsets"] is None else dev(b["offsets"]),
              lens=None if b["lens"] is None else dev(b["lens"]))
    return kw, big


def dev_chain(ch):
    return {k: dev(v) for k, v in ch.items()}


_FWD = {}


def forwarder(P, c):
    """One device handle per adjacency table for the module: create is the only allocation."""
    key = id(c["adj"])
    if key not in _FWD:
        _FWD[key] = (c["adj"], P.forwarder(W.adj_array(c["adj"])))
    return _FWD[key][1]


def run(P, c, b, ch, outputs=OUTS, flags=0, lpm=None, nexthop="case", stream=None, f=None, over=None):
    """pkt_fwd_batch over a fresh device copy of the batch, the slab and every output between guards -> (rc, {name:
    numpy, "slab": the slab after the call}, guards intact).  The counters start as 0x77.. and come back less that."""
    import torch
    f = forwarder(P, c) if f is None else f
    kw, big = dev_batch(b)
    pb = P._batch(kw["slab"], kw["n"], kw["stride"], kw["offsets"], kw["lens"])
    dch = dev_chain(ch)  # (held until the call has run)
    pc = P._chain(dch)
    n = b["n"]
    nexthop = c["nexthop"] if isinstance(nexthop, str) else nexthop
    nh = None if lpm is not None or nexthop is None else dev(nexthop)
    sel = None if c["select"] is None else dev(c["select"])
    bufs = {k: guarded((10 if k in ("hits", "bytes") else n) * np.dtype(ODT[k]).itemsize, FILL) for k in outputs}
    ptr = lambda k: bufs[k][1].data_ptr() if k in bufs and bufs[k][1].numel() else None  # noqa: E731
    tp = lambda t: t.data_ptr() if t is not None and t.numel() else None  # noqa: E731
    a = [f._f, ctypes.byref(pb), ctypes.byref(pc), c["which"], flags | (schema.FWD_KEEP_L2 if c["keep_l2"] else 0),
         None if lpm is None else lpm._t, tp(nh), tp(sel), *[ptr(k) for k in OUTS], P._stream(stream)]
    for k, v in dict(over or {}).items():
        a[k] = v
    rc = P._L.pkt_fwd_batch(*a)
    torch.cuda.synchronize()
    got = {k: g[1].cpu().numpy().view(ODT[k]) for k, g in bufs.items()}
    for k in ("hits", "bytes"):
        if k in got:
            got[k] = got[k] - np.uint64(FILL64)
    got["slab"] = kw["slab"].cpu().numpy()
    intact = all(guards_intact(*g) for g in bufs.values()) and guards_intact(big, kw["slab"])
    return rc, got, intact


def host(c, b, ch, lpm=None, flags=0):
    """The host twin over a copy of the batch."""
    b = dict(b, slab=b["slab"].copy())
    r = pktgpu.Forwarder(None, W.adj_array(c["adj"])).run(
        b, ch, nexthop=None if lpm is not None else c["nexthop"], lpm=lpm, which_ip=c["which"], keep_l2=c["keep_l2"],
        write=not flags & schema.FWD_NO_WRITE, select=c["select"], hits=True, bytes=True)
    return dict(r, slab=b["slab"])


def same(got, twin, label):
    for k in got:
        assert np.array_equal(got[k], twin[k]), (label, k, "differs from the host twin")


_EXPECT = {}


def laid_out(key, c, layout):
    """(batch, chain, the model's result) of a case in a layout, computed once and left unchanged."""
    k = (key, layout)
    if k not in _EXPECT:
        b, ch = W.layout(c, layout)
        _EXPECT[k] = (b, ch, W.expect(c, b, ch))
    return _EXPECT[k]


# ------------------------------------------------------------------ layouts and sizes
@pytest.mark.parametrize("n", SHAPES)
@pytest.mark.parametrize("layout", W.LAYOUTS)
def test_mix_in_every_layout(P, layout, n):
    """The seeded mix's first n packets: fixed stride 64 / 128 with and without lens, and the capture layout with
    packet i at alignment i % 16 and the last packet ending at the slab's last byte."""
    c = W.head(W.mix_cached(), n)
    b, ch, want = laid_out(("mix", n), c, layout)
    if n == 4096 and layout == "indexed":
        W.assert_mix(want, b, ch)
    rc, got, intact = run(P, c, b, ch)
    assert rc == 0 and intact
    W.check(got, want, f"mix {layout} {n}")
    same(got, host(c, b, ch), f"mix {layout} {n}")
    if layout == "indexed":
        assert int(b["offsets"][-1]) + int(b["lens"][-1]) == b["slab"].size and {int(o) % 16 for o in b["offsets"][:16]} == set(range(min(n, 16)))


@pytest.mark.parametrize("layout", W.LAYOUTS)
def test_named_cases_in_every_layout(P, layout):
    for name in W.NAMED:
        c, _ = W.named_cached()[name]
        b, ch, want = laid_out(name, c, layout)
        rc, got, intact = run(P, c, b, ch)
        assert rc == 0 and intact, name
        W.check(got, want, f"{name} {layout}")
        same(got, host(c, b, ch), f"{name} {layout}")


def test_a_70000_entry_adjacency_table(P):
    c = W.cached("mix70000", lambda: W.mix(2048, nadj=70000, seed=20272))
    b, ch, want = laid_out("mix70000", c, "indexed")
    assert (want["adj_index"][want["status"] == W.OK] > 65536).sum() > 20 and (np.bincount(want["status"], minlength=10) >= 8).all()
    rc, got, intact = run(P, c, b, ch)
    assert rc == 0 and intact
    W.check(got, want, "70000 adjacencies")


# ------------------------------------------------------------------ flags, select, outputs, counters
def test_no_write_and_keep_l2(P):
    c = W.head(W.mix_cached(), 1025)
    for layout in ("indexed", "s64"):
        b, ch, want = laid_out(("mix", 1025), c, layout)
        rc, got, intact = run(P, c, b, ch, flags=schema.FWD_NO_WRITE)
        assert rc == 0 and intact and np.array_equal(got["slab"], b["slab"])
        W.check({k: got[k] for k in OUTS}, want, f"NO_WRITE {layout}")
        k = dict(c, keep_l2=True)
        kwant = W.expect(k, b, ch)
        rc, got, intact = run(P, k, b, ch)
        assert rc == 0 and intact
        W.check(got, kwant, f"KEEP_L2 {layout}")
        assert (kwant["status"] == W.NO_ETHER).sum() == 0 and (want["status"] == W.NO_ETHER).sum() > 0
        rc, got, intact = run(P, k, b, ch, flags=schema.FWD_NO_WRITE, outputs=())
        assert rc == 0 and intact and np.array_equal(got["slab"], b["slab"])  # nothing to do: nothing launched


def test_select(P):
    c = W.head(W.mix_cached(), 300)
    b, ch, want = laid_out(("mix", 300), c, "indexed")
    assert (want["status"] == W.SKIPPED).sum() > 8
    none = dict(c, select=None)
    rc, got, intact = run(P, none, b, ch)
    assert rc == 0 and intact
    W.check(got, W.expect(none, b, ch), "no select")
    zero = dict(c, select=np.zeros(300, np.uint8))
    rc, got, intact = run(P, zero, b, ch)
    assert rc == 0 and intact and (got["status"] == W.SKIPPED).all() and np.array_equal(got["slab"], b["slab"])
    assert (got["port"] == W.NONE).all() and (got["adj_index"] == W.NONE).all() and got["hits"][W.SKIPPED] == 300


def test_each_output_alone(P):
    c = W.head(W.mix_cached(), 257)
    b, ch, want = laid_out(("mix", 257), c, "indexed")
    for name in OUTS:
        rc, got, intact = run(P, c, b, ch, outputs=(name,))
        assert rc == 0 and intact and set(got) == {name, "slab"}
        W.check(got, want, f"{name} alone")
    rc, got, intact = run(P, c, b, ch, outputs=())
    assert rc == 0 and intact
    W.check(got, want, "no output: the rewrite alone")


def test_counters_accumulate_over_two_streams(P):
    """Two different batches on two streams, four calls each, into one pair of counter arrays."""
    import torch
    ca, cb = W.head(W.mix_cached(), 4096), W.head(W.mix_cached(), 1000)
    ba, cha, wa = laid_out(("mix", 4096), ca, "indexed")
    bb, chb, wb = laid_out(("mix", 1000), cb, "s128_lens")
    f = forwarder(P, ca)
    (ka, _), (kb, _) = dev_batch(ba), dev_batch(bb)
    da, db = dev_chain(cha), dev_chain(chb)
    na, nb, sa, sb = dev(ca["nexthop"]), dev(cb["nexthop"]), dev(ca["select"]), dev(cb["select"])
    hits = torch.zeros(10, dtype=torch.uint64, device="cuda")
    byts = torch.zeros(10, dtype=torch.uint64, device="cuda")
    ss = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    res = []
    for _ in range(4):
        for s, kw, ch, nh, sel in ((ss[0], ka, da, na, sa), (ss[1], kb, db, nb, sb)):
            with torch.cuda.stream(s):
                res.append(f.run(kw, ch, nexthop=nh, select=sel, write=False, hits=hits, bytes=byts, stream=s))
    torch.cuda.synchronize()
    for k, r in enumerate(res):
        W.check({c: r[c].cpu().numpy() for c in W.NAMES}, (wa, wb)[k % 2], f"two streams, call {k}")
    assert np.array_equal(hits.cpu().numpy(), 4 * (wa["hits"] + wb["hits"]))
    assert np.array_equal(byts.cpu().numpy(), 4 * (wa["bytes"] + wb["bytes"]))
    assert int(hits.cpu().numpy().sum()) == 4 * (4096 + 1000)


def test_counters_with_a_capped_grid(P):
    """More tiles than a counting launch has blocks: a block takes several tiles."""
    reps = 90  # 90 x 4096 packets = 1440 tiles of 256
    c0 = W.mix_cached()
    b0, ch0, w0 = laid_out(("mix", 4096), W.head(c0, 4096), "s64_lens")
    c = dict(c0, nexthop=np.tile(c0["nexthop"], reps), select=np.tile(c0["select"], reps))
    b = C.batch(np.tile(b0["slab"], reps), lens=np.tile(b0["lens"], reps), stride=64, n=4096 * reps)
    ch = {k: np.tile(v, reps) for k, v in ch0.items()}
    rc, got, intact = run(P, c, b, ch)
    assert rc == 0 and intact
    assert np.array_equal(got["hits"], reps * w0["hits"]) and np.array_equal(got["bytes"], reps * w0["bytes"])
    assert np.array_equal(got["status"], np.tile(w0["status"], reps)) and np.array_equal(got["slab"], np.tile(w0["slab"], reps))


# ------------------------------------------------------------------ the fused route lookup
_LPM = {}


def lpms(P, c):
    key = id(c["routes"])
    if key not in _LPM:
        arr = X.to_array(c["routes"])
        _LPM[key] = (c["routes"], P.lpm(arr, W.LPM_DEFAULT), P.lpm(arr, W.LPM_DEFAULT, host=True))
    return _LPM[key][1:]


@pytest.mark.parametrize("name,kind", [("boundary", "probe"), ("short_after_long", "probe"), ("short_before_long", "probe"),
                                       ("siblings", "probe"), ("only_32", "probe"), ("only_128", "probe"),
                                       ("only_defaults", "probe"), ("random", "probe"), ("random", "vxlan")])
def test_fused_lpm_equals_lookup_then_run_and_the_model(P, name, kind):
    c = W.fused(name, kind)
    d, h = lpms(P, c)
    for layout in ("indexed", "s128_lens"):
        b, ch, want = laid_out(("fused", name, kind), c, layout)
        rc, fused, intact = run(P, c, b, ch, lpm=d)
        assert rc == 0 and intact
        W.check(fused, want, f"fused {name} {kind} {layout}")
        same(fused, host(c, b, ch, lpm=h), f"fused {name} {kind} {layout}")
        kw, _ = dev_batch(b)
        nh = d.lookup(kw, dev_chain(ch), which_ip=c["which"], outputs=("nexthop",))["nexthop"].cpu().numpy()
        rc, pair, intact = run(P, c, b, ch, nexthop=nh)
        assert rc == 0 and intact
        same(pair, fused, f"unfused pair {name} {kind} {layout}")
    if name == "random":
        assert {W.OK, W.NO_ADJ, W.DROP, W.PUNT, W.MTU} <= set(np.unique(want["status"]))
        vers = {v for v, _ in X.cached(name)[1][:400]}
        assert kind == "vxlan" or vers == {4, 6}


# ------------------------------------------------------------------ refusals
def test_refusals_come_before_any_launch(P):
    import torch
    c = W.head(W.mix_cached(), 65)
    b, ch, want = laid_out(("mix", 65), c, "s64_lens")
    err = lambda: P._L.pkt_ctx_last_error(P._ctx).decode()  # noqa: E731
    routes = [(4, 8, X.ip4("10.0.0.0"), 1)]
    dl, hl = P.lpm(X.to_array(routes), 0), P.lpm(X.to_array(routes), 0, host=True)
    kw, _ = dev_batch(b)
    pb = P._batch(kw["slab"], kw["n"], kw["stride"], kw["offsets"], kw["lens"])
    L = P._lib
    huge = L.PktBatch(pb.slab, pb.slab_len, None, pb.lens, 64, 0, 1 << 32)
    unaligned = L.PktBatch(pb.slab + 1, pb.slab_len - 1, None, pb.lens, 64, 0, 64)
    no_slab = L.PktBatch(None, pb.slab_len, None, pb.lens, 64, 0, 65)
    stride0 = L.PktBatch(pb.slab, pb.slab_len, None, pb.lens, 0, 0, 65)
    no_lens = L.PktBatch(pb.slab, pb.slab_len, pb.lens, None, 0, 0, 4)
    dch = dev_chain(ch)
    no_col = L.PktChain(dch["n_hdrs"].data_ptr(), None, dch["hdr_off"].data_ptr())
    odd = torch.zeros(96, dtype=torch.uint8, device="cuda")
    bad = [({1: None}, "null argument"), ({2: None}, "null argument"), ({2: ctypes.byref(no_col)}, "null chain column"),
           ({1: ctypes.byref(huge)}, "n >= 2^32"), ({1: ctypes.byref(unaligned)}, "slab not 16-byte aligned"),
           ({1: ctypes.byref(no_slab)}, "null slab"), ({1: ctypes.byref(stride0)}, "stride 0"),
           ({1: ctypes.byref(no_lens)}, "offsets without lens"), ({3: 16}, "which_ip"), ({3: 0xFE}, "which_ip"),
           ({4: 4}, "unknown flag bits"), ({4: 0x80000001}, "unknown flag bits"), ({5: dl._t}, "both lpm and nexthop"),
           ({6: None}, "neither lpm nor nexthop"), ({5: hl._t, 6: None}, "host handle"),
           ({11: odd.data_ptr() + 4}, "8-byte aligned"), ({12: odd.data_ptr() + 2}, "8-byte aligned")]
    for over, text in bad:
        rc, got, intact = run(P, c, b, ch, over=over)
        assert rc == -1 and intact, text
        assert err().startswith("pkt_fwd_batch: ") and text in err(), (text, err())
        assert all((got[k].view(np.uint8) == (0 if k in ("hits", "bytes") else FILL)).all() for k in OUTS), text
        assert np.array_equal(got["slab"], b["slab"]), text
    assert run(P, c, b, ch, over={3: 15})[0] == 0 and run(P, c, b, ch, over={0: None})[0] == -1
    # n == 0 succeeds, launches nothing and leaves the counters alone
    empty = L.PktBatch(pb.slab, pb.slab_len, None, pb.lens, 64, 0, 0)
    rc, got, intact = run(P, c, b, ch, over={1: ctypes.byref(empty)})
    assert rc == 0 and intact and all((got[k].view(np.uint8) == (0 if k in ("hits", "bytes") else FILL)).all() for k in OUTS)
    # create
    good = W.adj_array(c["adj"])
    act, zero = good.copy(), good.copy()
    act["action"][3] = 3
    zero["zero"][5] = 1
    for arr, text in ((act, "action"), (zero, "zero")):
        with pytest.raises(RuntimeError, match="pkt_fwd_create: .*" + text):
            P.forwarder(arr)
    h = ctypes.c_void_p()
    assert P._L.pkt_fwd_create(P._ctx, None, 3, ctypes.byref(h)) == -1 and err().startswith("pkt_fwd_create: ") and "null adj" in err()
    assert P._L.pkt_fwd_create(P._ctx, good.ctypes.data, (1 << 20) + 1, ctypes.byref(h)) == -1 and "PKT_FWD_MAX_ADJ" in err()
    assert not h.value and P._L.pkt_fwd_create(P._ctx, good.ctypes.data, 3, None) == -1 and err().startswith("pkt_fwd")
    with pytest.raises(ValueError):
        forwarder(P, c).run(kw, dch, lpm=hl)
    dl.close()
    hl.close()


# ------------------------------------------------------------------ the Python interface and the pipeline
def test_python_interface(P):
    import torch
    c, _ = W.named_cached()["statuses_v4"]
    b, ch, want = laid_out("statuses_v4", c, "indexed")
    f = P.forwarder([(d, s, port, mtu, act) for d, s, port, mtu, act in c["adj"]])
    kw, big = dev_batch(b)
    r = f.run(kw, dev_chain(ch), nexthop=dev(c["nexthop"]), select=dev(c["select"]), hits=True, bytes=True)
    torch.cuda.synchronize()
    assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in r.values()) and set(r) == set(OUTS)
    W.check(dict({k: v.cpu().numpy() for k, v in r.items()}, slab=kw["slab"].cpu().numpy()), want, "Forwarder.run")
    r = f.run((kw["slab"], kw["offsets"], kw["lens"]), dev_chain(ch), nexthop=dev(c["nexthop"]), outputs=("port",), write=False)
    assert set(r) == {"port"}
    f.close()
    f.close()
    assert guards_intact(big, kw["slab"])


def test_end_to_end_route_forward_dispatch_reorder_write(P):
    """257 packets: run(lpm=...) -> dispatcher(4).run(port) -> reorder -> pcap_write of bucket 0: exactly the OK packets
    with port 0 come out, in source order, already rewritten."""
    import torch
    base, probes, _, _ = X.cached("random")
    adj = [W.adjacency(k, port=k % 5, mtu=(0, 60)[k % 2], action=(0, 0, 0, 1, 2)[k % 5]) for k in range(40)]
    routes = [(v, p, a, i % 44) for i, (v, p, a, _) in enumerate(base)]
    arp = X.template("arp")
    items = []
    for k, pr in enumerate(probes[:257]):
        p, hd = X.packet_for(pr)
        q = bytearray(p)
        o = X.ip_slots(hd)[0][1]
        q[o + (8 if pr[0] == 4 else 7)] = k % 7  # ttl 0 and 1 among them
        items.append(arp if k % 10 == 7 else (W.fix_csum(q, o) if pr[0] == 4 else bytes(q), hd))
    c = W.case(items, adj=adj, routes=routes)
    b, ch = W.layout(c, "indexed")
    want = W.expect(c, b, ch)
    ok0 = np.flatnonzero((want["status"] == W.OK) & (want["port"] == 0))
    assert ok0.size >= 8 and (np.bincount(want["status"], minlength=10)[[W.OK, W.NO_IP, W.TTL, W.NO_ADJ, W.DROP, W.PUNT, W.MTU]] > 0).all()
    lpm = P.lpm(X.to_array(routes), W.LPM_DEFAULT)
    f = P.forwarder(W.adj_array(adj))
    kw, big = dev_batch(b)
    src = dict(offsets=kw["offsets"], lens=kw["lens"])
    res = P.parse(kw["slab"], columns=["chain"], **src)
    chain = {k: res[k] for k in ("n_hdrs", "hdr_type", "hdr_off")}
    r = f.run(kw, chain, lpm=lpm)
    W.check(dict({k: v.cpu().numpy() for k, v in r.items()}, slab=kw["slab"].cpu().numpy()), want, "run over the device parse")
    disp = P.dispatcher(4, None, max_n=b["n"])
    d = disp.run(r["port"])
    slot = (max(len(p) for p, _ in items) + 15) // 16 * 16
    ro = P.reorder(d["perm"], kw["slab"], columns=chain, start=d["start"], slot=slot, **src)
    seg = pktgpu.segments(d["start"], ro)[0]
    cap, nrec, _, _, _ = P.pcap_write(seg["slab"], lens=seg["lens"], stride=seg["stride"], n=seg["n"])
    torch.cuda.synchronize()
    raw = cap.cpu().numpy().tobytes()
    offs, lens = pktgpu.pcap_index(raw)
    out = [raw[int(o):int(o) + int(ln)] for o, ln in zip(offs, lens)]
    after = C.packets(dict(b, slab=want["slab"]))
    assert nrec == ok0.size and out == [after[i] for i in ok0]
    assert all(out[k] != C.packets(b)[i] for k, i in enumerate(ok0))  # rewritten: not the source bytes
    disp.close()
    f.close()
    lpm.close()
    assert guards_intact(big, kw["slab"])
