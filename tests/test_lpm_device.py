"""pkt_lpm_create and the device lookups (Parser.lpm / Lpm.lookup / Lpm.lookup_keys): the kernel of pktgpu_lpm.hip
against lpm_cases' yardstick (a dict of prefixes per length) and the host handle.  The compile and the walk are
covered on the CPU (test_lpm_host.py: the host handle runs the same code); here it is the address extraction, the
launch shape and the stores.  Every output lies between two guard regions filled with 0xA5 and starts as 0x77, so
that a byte the call must not write is seen."""
import numpy as np
import pytest

import pktgpu
from pktgpu import gen

import compare_cases as C
import l4_cases as L4
import lpm_cases as X

pytestmark = pytest.mark.gpu
GUARD = 4096
FILL = 0x77
SHAPES = [1, 63, 64, 65, 257, 4096]


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


_DEV, _HOST = {}, {}


def handles(P, name):
    """One device and one host handle per named table for the module: create is the only allocation."""
    if name not in _DEV:
        arr = X.to_array(X.cached(name)[0])
        _DEV[name] = P.lpm(arr, X.DEFAULT)
        _HOST[name] = P.lpm(arr, X.DEFAULT, host=True)
    return _DEV[name], _HOST[name]


def dev_batch(b):
    big, slab = guarded(b["slab"].size)
    slab.copy_(dev(b["slab"]))
    kw = dict(slab=slab, n=b["n"], stride=b["stride"], offsets=None if b["offsets"] is None else dev(b["offsets"]),
              lens=None if b["lens"] is None else dev(b["lens"]))
    return kw, big


def dev_chain(ch):
    return {k: dev(v) for k, v in ch.items()}


def outputs_between_guards(n, outputs):
    bufs = {k: guarded(n * np.dtype(X.DT[k]).itemsize, FILL) for k in outputs}
    return bufs, [bufs[k][1].data_ptr() if k in bufs and n else None for k in X.NAMES]


def collect(bufs, n):
    import torch
    torch.cuda.synchronize()
    got = {k: g[1].cpu().numpy().view(X.DT[k])[:n] for k, g in bufs.items()}
    return got, all(guards_intact(*g) for g in bufs.values())


def run_batch(P, h, kw, chain, outputs=X.NAMES, which=0, src=False, stream=None):
    """pkt_lpm_lookup_batch with every output between guards -> (rc, {name: numpy}, guards intact)."""
    import ctypes
    b = P._batch(kw["slab"], kw["n"], kw["stride"], kw["offsets"], kw["lens"])
    ch = P._chain(chain)
    bufs, ptrs = outputs_between_guards(b.n, outputs)
    rc = P._L.pkt_lpm_lookup_batch(h._t, ctypes.byref(b), ctypes.byref(ch), which, 1 if src else 0, *ptrs, P._stream(stream))
    got, intact = collect(bufs, b.n)
    return rc, got, intact


def run_keys(P, h, keys, status=None, outputs=X.NAMES, src=False, shift=0, stream=None):
    """pkt_lpm_lookup_keys with the keys `shift` bytes past a 16-byte boundary and every output between guards."""
    n = keys.shape[0]
    gk = guarded(keys.size, shift=shift)
    gk[1].copy_(dev(keys.reshape(-1)))
    st = None if status is None else dev(status)
    bufs, ptrs = outputs_between_guards(n, outputs)
    rc = P._L.pkt_lpm_lookup_keys(h._t, gk[1].data_ptr(), None if st is None else st.data_ptr(), n, 1 if src else 0, *ptrs,
                                  P._stream(stream))
    got, intact = collect(bufs, n)
    return rc, got, intact and guards_intact(*gk) and np.array_equal(gk[1].cpu().numpy(), keys.reshape(-1))


# ------------------------------------------------------------------ keys
@pytest.mark.parametrize("name", X.SMALL + ["random", "large"])
def test_keys_against_the_model_and_the_host_handle(P, name):
    routes, probes, model, want = X.cached(name)
    if name in ("random", "large"):
        X.assert_mix(want, name)
    d, h = handles(P, name)
    assert d.info() == h.info()
    keys = X.keys_of(probes)
    rc, got, intact = run_keys(P, d, keys)
    assert rc == 0 and intact
    X.check(got, want, name)
    X.check(got, h.lookup_keys(keys), name + " (host handle)")


@pytest.mark.parametrize("shift", [0, 2, 4, 8, 14])
def test_keys_at_every_alignment_the_kernel_tells_apart(P, shift):
    """Dword loads where the keys are 4-byte aligned, 2-byte loads otherwise; with a status column and bad versions."""
    routes, probes, model, _ = X.cached("random")
    probes = list(probes[:321])
    for k in range(7, 321, 29):
        probes[k] = ((0, 5, 7, 46)[k % 4], probes[k][1] & 0xFFFFFFFF)
    st = (np.arange(321) % 9 == 4).astype(np.uint8) * 3
    d, _ = handles(P, "random")
    for src in (False, True):
        pr = [(v, a ^ ((1 << X.W[v]) - 1)) if v in X.W else (v, a) for v, a in probes] if src else probes
        want = X.expect_probes(model, pr, st)
        rc, got, intact = run_keys(P, d, X.keys_of(probes), st, src=src, shift=shift)
        assert rc == 0 and intact
        X.check(got, want, f"shift {shift} src={src}")
    assert (want["status"] == X.SKIPPED).sum() > 40


# ------------------------------------------------------------------ batches
_BATCHES = {}


def batch_of(kind, layout, n):
    """(batch, chain, expected by the model) of the first n probes of the random table, built once."""
    key = (kind, layout, n)
    if key not in _BATCHES:
        routes, probes, model, _ = X.cached("random")
        items = (X.mixed_items if kind == "mixed" else X.probe_items)(probes[:n])
        b, ch = X.batch_case(items, layout, seed=n)
        _BATCHES[key] = (b, ch, X.expect_batch(model, b, ch), X.expect_batch(model, b, ch, src=True))
    return _BATCHES[key]


@pytest.mark.parametrize("n", SHAPES)
@pytest.mark.parametrize("layout", [96, "indexed"])
@pytest.mark.parametrize("kind", ["probe", "mixed"])
def test_batch_shapes(P, kind, layout, n):
    """Fixed-stride batches and capture-layout batches at odd alignments, at the sizes where the launch can go
    wrong; "mixed" puts IPv4, IPv6, ARP, cut and header-less packets side by side in one wave."""
    b, ch, want, want_src = batch_of(kind, layout, n)
    d, h = handles(P, "random")
    kw, big = dev_batch(b)
    dch = dev_chain(ch)
    rc, got, intact = run_batch(P, d, kw, dch)
    assert rc == 0 and intact and guards_intact(big, kw["slab"])
    X.check(got, want, f"{kind} {layout} {n}")
    if n >= 257 and kind == "mixed":
        assert set(np.unique(want["status"])) == {X.OK, X.NO_ROUTE, X.NO_IP, X.SPAN}
    X.check(got, h.lookup(b, ch), f"{kind} {layout} {n} (host handle)")
    rc, got, intact = run_batch(P, d, kw, dch, src=True)
    assert rc == 0 and intact
    X.check(got, want_src, f"{kind} {layout} {n} src")
    assert np.array_equal(kw["slab"].cpu().numpy(), b["slab"])


def test_boundary_and_leaf_push_tables_through_packets(P):
    for name in X.SMALL:
        routes, probes, model, _ = X.cached(name)
        d, _ = handles(P, name)
        b, ch = X.batch_case(X.probe_items(probes), "indexed")
        kw, big = dev_batch(b)
        rc, got, intact = run_batch(P, d, kw, dev_chain(ch))
        assert rc == 0 and intact
        X.check(got, X.expect_batch(model, b, ch), name)


def test_vxlan_which_ip(P):
    routes, probes, model, _ = X.cached("large")
    v4 = [a for v, a in probes if v == 4]
    items = [X.vxlan_for(v4[2 * k], v4[2 * k + 1]) for k in range(150)] + X.probe_items(probes[:43])
    b, ch = X.batch_case(items, "indexed")
    d, _ = handles(P, "large")
    kw, big = dev_batch(b)
    dch = dev_chain(ch)
    wants = {w: X.expect_batch(model, b, ch, w) for w in (0, 1, X.LAST)}
    assert not np.array_equal(wants[0]["route"], wants[1]["route"]) and (wants[1]["status"][150:] == X.NO_IP).all()
    for w, want in wants.items():
        rc, got, intact = run_batch(P, d, kw, dch, which=w)
        assert rc == 0 and intact
        X.check(got, want, f"vxlan which_ip={w}")
    rc, got, intact = run_batch(P, d, kw, dch, which=1, src=True)
    assert rc == 0 and intact
    X.check(got, X.expect_batch(model, b, ch, 1, True), "vxlan inner src")


def test_deep_chain_rows_past_the_fourth(P):
    """An IP entry in slot row 5 (rows 0..3 are loaded up front, the rest in a loop): Ether / 4 x Vlan / IPv4."""
    routes, probes, model, _ = X.cached("random")
    v4 = [pr for pr in probes if pr[0] == 4][:70]
    items = []
    for k, (ver, addr) in enumerate(v4):
        p = bytearray(L4.pkt("UDP", vlans=4, payload=b"deep"))
        hdrs = L4.hdrs_of(bytes(p))
        o = X.ip_slots(hdrs)[0][1]
        assert [t for t, _ in hdrs].index(X.T_IPV4) == 5
        p[o + 16:o + 20] = addr.to_bytes(4, "big")
        items.append((bytes(p), hdrs))
    b, ch = X.batch_case(items, "indexed")
    d, _ = handles(P, "random")
    kw, big = dev_batch(b)
    for w in (0, X.LAST):
        rc, got, intact = run_batch(P, d, kw, dev_chain(ch), which=w)
        assert rc == 0 and intact
        X.check(got, X.expect_batch(model, b, ch, w), f"deep chain which_ip={w}")


def test_each_output_alone_and_none(P):
    b, ch, want, _ = batch_of("mixed", "indexed", 257)
    d, _ = handles(P, "random")
    kw, big = dev_batch(b)
    dch = dev_chain(ch)
    routes, probes, model, want_k = X.cached("random")
    keys = X.keys_of(probes[:257])
    for name in X.NAMES:
        rc, got, intact = run_batch(P, d, kw, dch, outputs=(name,))
        assert rc == 0 and intact and set(got) == {name}
        X.check(got, want, f"batch, {name} alone")
        rc, got, intact = run_keys(P, d, keys, outputs=(name,))
        assert rc == 0 and intact and set(got) == {name}
        X.check(got, {k: v[:257] for k, v in want_k.items()}, f"keys, {name} alone")
    assert run_batch(P, d, kw, dch, outputs=())[0] == 0 and run_keys(P, d, keys, outputs=())[0] == 0


def test_empty_calls_and_empty_table(P):
    import torch
    b, ch, want, _ = batch_of("mixed", "indexed", 65)
    d, _ = handles(P, "random")
    kw, big = dev_batch(b)
    rc, got, intact = run_batch(P, d, dict(kw, n=0, offsets=kw["offsets"][:0], lens=kw["lens"][:0]), dev_chain(ch))
    assert rc == 0 and intact and all(v.size == 0 for v in got.values())
    empty = P.lpm([], X.DEFAULT)
    rc, got, intact = run_batch(P, empty, kw, dev_chain(ch))
    assert rc == 0 and intact
    X.check(got, X.expect_batch(X.Model([]), b, ch), "empty table")
    assert not (got["status"] == X.OK).any() and (got["status"] == X.NO_ROUTE).any()
    res = empty.lookup_keys(dev(X.keys_of(X.cached("random")[1][:10])))
    torch.cuda.synchronize()
    assert (res["status"].cpu().numpy() == X.NO_ROUTE).all() and (res["nexthop"].cpu().numpy() == X.DEFAULT).all()
    empty.close()


def test_refusals_come_before_any_launch(P):
    b, ch, want, _ = batch_of("probe", 96, 65)
    d, _ = handles(P, "random")
    kw, big = dev_batch(b)
    dch = dev_chain(ch)
    err = lambda: P._L.pkt_lpm_last_error(d._t).decode()  # noqa: E731
    for over, which, text in ((dict(slab=kw["slab"][1:]), 0, "slab not 16-byte aligned"), ({}, 16, "which_ip"), ({}, 0xFE, "which_ip")):
        rc, got, intact = run_batch(P, d, dict(kw, **over), dch, which=which)
        assert rc == -1 and intact and all((v.view(np.uint8) == FILL).all() for v in got.values()), text
        assert err().startswith("pkt_lpm_lookup_batch: ") and text in err(), err()
    keys = X.keys_of(X.cached("random")[1][:65])
    rc, got, intact = run_keys(P, d, keys, shift=1)
    assert rc == -1 and intact and all((v.view(np.uint8) == FILL).all() for v in got.values())
    assert err().startswith("pkt_lpm_lookup_keys: ") and "2-byte aligned" in err()
    with pytest.raises(RuntimeError, match="pkt_lpm_create: .*same"):
        P.lpm([("10.0.0.0/8", 1), ("10.0.0.0/8", 2)])
    with pytest.raises(RuntimeError, match="pkt_lpm_create: .*needs 525320 bytes"):
        P.lpm([("10.1.2.0/24", 1)], max_bytes=4096)


def test_python_interface(P):
    """Parser.lpm with string routes, Lpm.lookup with a batch dict -> device tensors; a host handle -> numpy arrays."""
    import torch
    routes, probes, model, _ = X.cached("siblings")
    d = P.lpm(X.to_strings(routes), X.DEFAULT)
    b, ch = X.batch_case(X.probe_items(probes), "indexed")
    kw, big = dev_batch(b)
    res = d.lookup(kw, dev_chain(ch))
    assert all(isinstance(res[k], torch.Tensor) and res[k].is_cuda for k in X.NAMES)
    X.check({k: v.cpu().numpy() for k, v in res.items()}, X.expect_batch(model, b, ch), "Lpm.lookup")
    res = d.lookup(kw, dev_chain(ch), src=True, outputs=("nexthop",))
    assert set(res) == {"nexthop"}
    X.check({"nexthop": res["nexthop"].cpu().numpy()}, X.expect_batch(model, b, ch, src=True), "Lpm.lookup nexthop")
    h = P.lpm(X.to_strings(routes), X.DEFAULT, host=True)
    assert all(isinstance(v, np.ndarray) for v in h.lookup(b, ch).values()) and h.info() == d.info()
    d.close()


def test_two_lookups_on_one_handle_on_two_streams(P):
    import torch
    d, _ = handles(P, "random")
    ba, cha, wa, _ = batch_of("mixed", "indexed", 4096)
    bb, chb, wb, _ = batch_of("probe", 96, 4096)
    (ka, _), (kb, _) = dev_batch(ba), dev_batch(bb)
    da, db = dev_chain(cha), dev_chain(chb)
    alone = [{k: v.cpu().numpy() for k, v in d.lookup(kw, ch).items()} for kw, ch in ((ka, da), (kb, db))]
    ss = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    res = []
    for _ in range(4):
        for s, kw, ch in ((ss[0], ka, da), (ss[1], kb, db)):
            with torch.cuda.stream(s):
                res.append(d.lookup(kw, ch, stream=s))
    torch.cuda.synchronize()
    for k, r in enumerate(res):
        X.check({c: t.cpu().numpy() for c, t in r.items()}, (wa, wb)[k % 2], f"two streams, call {k}")
        assert all(np.array_equal(r[c].cpu().numpy(), alone[k % 2][c]) for c in X.NAMES)


def test_stream_windows_equal_the_whole_capture(P):
    """PcapStream.batch() with the stream's chain columns, window by window, against one lookup over the same
    capture parsed whole (and the model)."""
    import torch
    from pktgpu.stream import PcapStream
    routes, probes, model, _ = X.cached("random")
    items = X.mixed_items(probes[:150])
    pkts = [p for p, _ in items]
    raw = gen.pcap_bytes(pkts)
    d, _ = handles(P, "random")
    # whole: the capture indexed on the host, parsed on the device
    offs, lens = pktgpu.pcap_index(raw)
    whole = C.batch(np.frombuffer(raw, np.uint8), offs, lens)
    kw, big = dev_batch(whole)
    res = P.parse(kw["slab"], columns=["chain"], offsets=kw["offsets"], lens=kw["lens"])
    chain = {c: res[c] for c in ("n_hdrs", "hdr_type", "hdr_off")}
    full = {k: v.cpu().numpy() for k, v in d.lookup(kw, chain).items()}
    want = X.expect_batch(model, whole, L4.chain_of(whole))
    X.check(full, want, "whole capture")
    assert {X.OK, X.NO_ROUTE, X.NO_IP} <= set(np.unique(want["status"]))
    cap = 32
    st = PcapStream(0, max_bytes=1 << 20, cap=cap, columns=["chain"])
    parts = {k: [] for k in X.NAMES}
    rng = np.random.default_rng(5)
    try:
        at = 0
        while at < len(raw):
            k = int(rng.integers(1, 900))
            st.push(raw[at:at + k])
            at += k
        while True:
            n, _ = st.poll()
            last = n <= cap
            if last:
                n, _ = st.finish()
            win = st.batch()
            k = win[1].numel()
            ch = {c: st.out[c] if k == cap else st.out[c][..., :k].contiguous() for c in ("n_hdrs", "hdr_type", "hdr_off")}
            r = d.lookup(win, ch)
            torch.cuda.synchronize()  # the window's readers are done before the stream moves it
            for c in X.NAMES:
                parts[c].append(r[c].cpu().numpy())
            if last:
                break
            st.release(cap)
    finally:
        st.close()
    for c in X.NAMES:
        assert np.array_equal(np.concatenate(parts[c]), full[c]), c


def test_end_to_end_route_then_dispatch(P):
    """parse -> lookup (dst) -> dispatcher(nbuckets, DIRECT).run(key=nexthop) -> reorder: every packet of segment b
    has model next hop b, and the packets whose next hop is the default (>= nbuckets) form the dropped tail."""
    import torch
    nb, default = 4, 9
    base, probes, _, _ = X.cached("random")
    routes = [(v, p, a, i % nb) for i, (v, p, a, _) in enumerate(base)]
    model = X.Model(routes, default)
    arp = X.template("arp")
    items = [arp if k % 10 == 7 else X.packet_for(pr) for k, pr in enumerate(probes[:600])]
    pkts = [p for p, _ in items]
    b = C.indexed(pkts, np.random.default_rng(3))
    n = b["n"]
    want = X.expect_batch(model, b, L4.chain_of(b))
    dropped = want["nexthop"] == default
    assert dropped.sum() >= n // 8 and all((want["nexthop"] == q).sum() > 0 for q in range(nb))
    assert (want["nexthop"][~dropped] < nb).all() and (want["status"][dropped] != X.OK).all()
    d = P.lpm(X.to_array(routes), default)
    kw, big = dev_batch(b)
    src = dict(offsets=kw["offsets"], lens=kw["lens"])
    res = P.parse(kw["slab"], columns=["chain"], **src)
    chain = {c: res[c] for c in ("n_hdrs", "hdr_type", "hdr_off")}
    r = d.lookup(kw, chain)
    X.check({k: v.cpu().numpy() for k, v in r.items()}, want, "lookup over the device parse")
    disp = P.dispatcher(nb, None, max_n=n)
    run = disp.run(r["nexthop"])
    slot = (max(len(p) for p in pkts) + 15) // 16 * 16
    ro = P.reorder(run["perm"], kw["slab"], columns=chain, start=run["start"], slot=slot, **src)
    segs = pktgpu.segments(run["start"], ro)
    torch.cuda.synchronize()
    perm, start = run["perm"].cpu().numpy().astype(np.int64), run["start"].cpu().numpy().astype(np.int64)
    assert len(segs) == nb and int(start[nb]) == int((~dropped).sum()) and int(start[nb + 1]) == n
    for q, s in enumerate(segs):
        pq = perm[start[q]:start[q + 1]]
        assert s["n"] == pq.size > 0 and (np.diff(pq) > 0).all() and (want["nexthop"][pq] == q).all(), q
        again = d.lookup(s, s["chain"], outputs=("nexthop", "route"))  # a segment is a batch of its own
        assert (again["nexthop"].cpu().numpy() == q).all() and np.array_equal(again["route"].cpu().numpy(), want["route"][pq])
        got = C.packets(C.batch(s["slab"].cpu().numpy(), lens=s["lens"].cpu().numpy(), stride=s["stride"], n=s["n"]))
        assert got == [pkts[i] for i in pq], q
    tail = perm[start[nb]:]
    assert (np.diff(tail) > 0).all() and dropped[tail].all() and tail.size == dropped.sum()
    disp.close()
    d.close()
    assert guards_intact(big, kw["slab"]) and np.array_equal(kw["slab"].cpu().numpy(), b["slab"])
