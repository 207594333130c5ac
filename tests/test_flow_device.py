"""pkt_flow_key_batch and the device flow table (Parser.flow_keys, FlowTable(parser, slots)): the kernels of
pktgpu_flow.hip against flow_cases' yardstick (a pure-Python key builder, a bitwise Toeplitz, a dict model of
the table) and the host twin.  Every slab lies between two guard regions filled with 0xA5 (a kernel that took
address or port bytes from past slab_len would show 0xA5 in the key) and so does every output array.  Slot
numbers are racy on the device: partitions and the records sorted by `first` are compared, never slot ids."""
import ctypes

import numpy as np
import pytest

from pktgpu import gen

import compare_cases as C
import edit_cases as E
import flow_cases as F
import l4_cases as L4

pytestmark = pytest.mark.gpu
GUARD = 4096
OUT_NAMES = ("keys", "hash", "rss", "dir", "plen", "status")
OUT_SIZE = (40, 8, 4, 1, 4, 1)


@pytest.fixture(scope="module")
def P():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible")
    import pktgpu
    return pktgpu.Parser(0)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def guarded(nbytes, shift=0):
    """A 0xA5-filled allocation with `nbytes` in its middle, `shift` bytes off a 4096 boundary -> (all, middle)."""
    import torch
    big = torch.full((GUARD + shift + (nbytes + 15) // 16 * 16 + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    return big, big[GUARD + shift:GUARD + shift + nbytes]


def guards_intact(big, mid):
    lo = mid.data_ptr() - big.data_ptr()
    return bool((big[:lo] == 0xA5).all()) and bool((big[lo + mid.numel():] == 0xA5).all())


def dev_batch(b):
    big, slab = guarded(b["slab"].size)
    slab.copy_(dev(b["slab"]))
    kw = dict(slab=slab, n=b["n"], stride=b["stride"], offsets=None if b["offsets"] is None else dev(b["offsets"]),
              lens=None if b["lens"] is None else dev(b["lens"]))
    return kw, big


def run_guarded(P, c, kw, outputs=(True,) * 6, key_shift=0, rss_key=F.RSS_KEY, **over):
    """pkt_flow_key_batch with every output between guards -> (rc, {name: numpy}, guards intact)."""
    import torch
    o = dict(c["opt"], **over)
    chain = {k: dev(v) for k, v in c["chain"].items()}
    args, _, keep = P._flow_args(chain=chain, which_ip=o["which_ip"], symmetric=o["symmetric"], ports=o["ports"], seed=F.SEED,
                                 rss_key=rss_key, outputs=(False,) * 6, **kw)
    n = kw["n"]
    bufs = [guarded(n * sz, key_shift if name == "keys" else 0) if w else None for name, sz, w in zip(OUT_NAMES, OUT_SIZE, outputs)]
    ptrs = [None if b is None or not n else b[1].data_ptr() for b in bufs]
    rc = P._L.pkt_flow_key_batch(P._ctx, *args[:6], *ptrs, P._stream(None))
    torch.cuda.synchronize()
    dts = (np.uint8, np.uint64, np.uint32, np.uint8, np.uint32, np.uint8)
    got = {}
    for name, dt, b in zip(OUT_NAMES, dts, bufs):
        got[name] = None if b is None else b[1].cpu().numpy().view(dt).reshape((n, 40) if name == "keys" else (n,))
    return rc, got, all(guards_intact(*b) for b in bufs if b is not None)


def host_twin(c, **over):
    import pktgpu
    b, o = c["batch"], dict(c["opt"], **over)
    return pktgpu.flow_keys(b["slab"], c["chain"], o["which_ip"], o["symmetric"], o["ports"], F.SEED, F.RSS_KEY,
                            stride=b["stride"], n=b["n"], offsets=b["offsets"], lens=b["lens"])


@pytest.mark.parametrize("name", F.CASE_NAMES)
def test_cases(P, name):
    c, want = F.all_cases()[name]
    kw, big = dev_batch(c["batch"])
    rc, got, intact = run_guarded(P, c, kw)
    assert rc == 0 and intact
    F.check(got, want, name)
    F.check(got, host_twin(c), name + " (host twin)")
    assert guards_intact(big, kw["slab"]) and np.array_equal(kw["slab"].cpu().numpy(), c["batch"]["slab"])


def test_flags_null_outputs_and_key_alignments(P):
    c, _ = F.all_cases()["protocols"]
    kw, big = dev_batch(c["batch"])
    for which in (0, 1, F.LAST):
        for sym in (False, True):
            for ports in (False, True):
                rc, got, intact = run_guarded(P, c, kw, which_ip=which, symmetric=sym, ports=ports)
                assert rc == 0 and intact
                F.check(got, F.expect(c, which_ip=which, symmetric=sym, ports=ports), f"{which} {sym} {ports}")
    for name in ("c2_stride64_65", "span_lens", "every_alignment"):
        c, want = F.all_cases()[name]
        kw, big = dev_batch(c["batch"])
        for drop in range(6):
            rc, got, intact = run_guarded(P, c, kw, outputs=tuple(k != drop for k in range(6)))
            assert rc == 0 and intact
            F.check(got, want, f"{name} without output {drop}")
        assert run_guarded(P, c, kw, outputs=(False,) * 6, rss_key=None)[0] == 0
        for shift in (8, 2, 6):  # keys 8- and 2-byte aligned: the narrower stores
            rc, got, intact = run_guarded(P, c, kw, key_shift=shift)
            assert rc == 0 and intact
            F.check(got, want, f"{name} keys + {shift}")
        assert run_guarded(P, c, kw, key_shift=1)[0] == -1


def test_refusals(P):
    import torch
    c, want = F.all_cases()["c2_stride64_1000"]
    kw, big = dev_batch(c["batch"])
    chain = {k: dev(v) for k, v in c["chain"].items()}
    args, out, keep = P._flow_args(chain=chain, symmetric=True, seed=F.SEED, rss_key=F.RSS_KEY, **kw)
    L, s, lib = P._L, P._stream(None), P._lib

    def call(r=()):
        a = list(args)
        for k, v in dict(r).items():
            a[k] = v
        return L.pkt_flow_key_batch(P._ctx, *a, s)
    for t in out:
        t.view(torch.uint8).fill_(0x77)
    huge = P._batch(kw["slab"], 1 << 32, 64, None, None)
    odd = P._batch(kw["slab"][1:], None, 64, None, None)
    no_lens = lib.PktBatch()
    four = dev(np.zeros(4, np.uint64))
    no_lens.slab, no_lens.slab_len, no_lens.offsets, no_lens.n = keep[0].slab, keep[0].slab_len, four.data_ptr(), 4
    no_col = lib.PktChain(keep[1].n_hdrs, None, keep[1].hdr_off)
    bad = [{0: None}, {1: None}, {1: ctypes.byref(no_col)}, {0: ctypes.byref(huge)}, {0: ctypes.byref(odd)},
           {0: ctypes.byref(no_lens)}, {2: 16}, {2: 0xFE}, {3: 4}, {3: 0x80000001}, {5: None}, {6: out[0].data_ptr() + 1}]
    for r in bad:
        assert call(r) == -1, sorted(r)
    torch.cuda.synchronize()
    assert all(bool((t.view(torch.uint8) == 0x77).all()) for t in out)  # every refusal came before any launch
    empty = P._batch(kw["slab"], 0, 64, None, None)
    assert call({0: ctypes.byref(empty)}) == 0
    torch.cuda.synchronize()
    assert all(bool((t.view(torch.uint8) == 0x77).all()) for t in out)
    with pytest.raises(RuntimeError):
        P.flow_keys(kw["slab"], chain, which_ip=16, stride=64)
    assert call({2: 15}) == 0 and call() == 0
    F.check({k: t.cpu().numpy() for k, t in zip(OUT_NAMES, out)}, want, "after the errors")
    got = P.flow_keys(kw["slab"], chain, symmetric=True, seed=F.SEED, stride=64)
    assert "rss" not in got
    F.check({k: t.cpu().numpy() for k, t in got.items()}, want, "without rss")


def test_rss_matches_the_microsoft_vectors(P):
    key, vec, pk = F.rss_packets()
    b = C.indexed(pk, np.random.default_rng(3))
    kw, big = dev_batch(b)
    ch = {k: dev(v) for k, v in L4.chain_of(b).items()}
    for ports, col in ((True, "with_ports"), (False, "addr_only")):
        got = P.flow_keys(chain=ch, ports=ports, rss_key=key, **kw)["rss"].cpu().numpy()
        assert got.tolist() == [int(v[col], 16) for v in vec], (ports, [hex(x) for x in got])


def test_keys_on_edits_out_chain(P):
    """A VXLAN encap by pkt_edit_batch: which_ip 0 is the pushed outer IPv4, LAST the inner one; the keys are
    the yardstick's over the edited bytes with a parse of them by the Python model."""
    rng = np.random.default_rng(92)
    n = 70
    inner = [bytes(gen.test_tcp_packet_with_payload(E.rnd_bytes(rng, int(rng.integers(0, 200)))).to_vec()) for _ in range(n)]
    outer = bytes(gen.create_vxlan_packet(E.M1, E.M2, False, 10, 3, 5, "192.168.0.199", "192.168.0.1", 0, 64, 0, 0x4000, [],
                                          gen.VXLAN_PORT, 9090, False, 2000, gen.test_tcp_packet_with_payload(b"")).to_vec())[:50]
    src, _ = dev_batch(C.indexed(inner, rng))
    parsed = P.parse(src["slab"], offsets=src["offsets"], lens=src["lens"], columns=["chain"])
    dst, ln, st, ch = P.edit(src["slab"], parsed, E.encap_ops(outer), offsets=src["offsets"], lens=src["lens"], slot=512)
    assert (st.cpu().numpy() == E.OK).all()
    d, lens = dst.cpu().numpy(), ln.cpu().numpy()
    for which in (0, 1, F.LAST):
        got = {k: v.cpu().numpy() for k, v in P.flow_keys(dst, ch, which_ip=which, symmetric=True, seed=F.SEED, rss_key=F.RSS_KEY,
                                                          stride=512, lens=ln).items()}
        for i in range(n):
            p = d[512 * i:512 * i + int(lens[i])].tobytes()
            w = F.one(p, F.hdrs_of(p), which, True)
            assert (got["status"][i], got["keys"][i].tobytes(), int(got["hash"][i]), int(got["rss"][i]), got["dir"][i]) == \
                (w["status"], w["key"], w["hash"], w["rss"], w["dir"]), (which, i)
        assert (got["status"] == F.OK).all() and (got["plen"] == lens).all()


# ------------------------------------------------------------------ the table
def to_dev(k):
    return {c: dev(v) for c, v in k.items()}


def run_both(table, model, k, weight="plen", base=0):
    """One update on the device table and the model: statuses equal, the partition by flow_id the model's."""
    fid, upd = table.update(to_dev(k), weight=weight, base=base)
    fid, upd = fid.cpu().numpy(), upd.cpu().numpy()
    flow, want = model.update(k["keys"], k["hash"], k.get("dir"), k[weight] if isinstance(weight, str) else weight, k.get("status"), base)
    assert np.array_equal(upd, want), np.flatnonzero(upd != want)[:8]
    assert F.same_partition(fid, flow)
    return fid, upd


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_table_against_the_model_and_the_host_twin(P, n):
    import pktgpu
    rng = np.random.default_rng(n)
    for n_flows in (1, max(1, n // 7), n):
        t, h, m = pktgpu.FlowTable(P, 8192), pktgpu.FlowTable(None, 8192), F.TableModel(8192)
        k, f = F.traffic(rng, n, n_flows)
        fid, upd = run_both(t, m, k)
        h.update(k)
        assert (upd == F.UPD_OK).all() and t.count() == len(set(f.tolist()))
        F.check_records(t.flows(), m.records(), f"{n} {n_flows}")
        F.check_records(t.flows(), h.flows(), f"{n} {n_flows} (host twin)")
        t.close()
        h.close()


def test_one_flow_4097_packets_counts_exactly(P):
    """Every packet in one flow, one direction: wave aggregation and atomics across blocks."""
    import pktgpu
    k, _ = F.traffic(np.random.default_rng(1), 4097, 1, both_dirs=False)
    t = pktgpu.FlowTable(P, 64)
    fid, upd = t.update(to_dev(k))
    r = t.flows()
    assert r["pkts"].tolist() == [[4097, 0]] and r["bytes"].tolist() == [[int(k["plen"].sum()), 0]] and r["first"][0] == 0
    assert len(set(fid.cpu().numpy().tolist())) == 1 and (upd.cpu().numpy() == F.UPD_OK).all()
    t.close()


def test_three_updates_null_columns_and_a_falling_base(P):
    import pktgpu
    rng = np.random.default_rng(8)
    t, m = pktgpu.FlowTable(P, 1024), F.TableModel(1024)
    k, _ = F.traffic(rng, 900, 200)
    k["status"][::13] = 2
    parts = [{c: v[a:b] for c, v in k.items()} for a, b in ((0, 300), (300, 301), (301, 900))]
    for p, base in zip(parts, (0, 1000, 5000)):
        run_both(t, m, p, base=base)
    F.check_records(t.flows(), m.records())
    with pytest.raises(RuntimeError):
        t.update(to_dev(parts[0]), base=5598)
    run_both(t, m, parts[0], weight=None, base=1 << 40)
    run_both(t, m, {c: v for c, v in parts[2].items() if c in ("keys", "hash")}, weight=None, base=1 << 41)
    # neither flow_id nor upd_status: the table's own scratch words hold the entries between the launches
    d = to_dev(parts[2])
    args, out, keep = t._update_args(d, base=1 << 42, outputs=(False, False))
    assert P._L.pkt_flow_table_update(t._t, *args, P._stream(None)) == 0
    m.update(parts[2]["keys"], parts[2]["hash"], parts[2]["dir"], parts[2]["plen"], parts[2]["status"], 1 << 42)
    F.check_records(t.flows(), m.records(), "no outputs")
    t.close()


def test_slots_64_filled_and_overfilled(P):
    import pktgpu
    rng = np.random.default_rng(64)
    t, m = pktgpu.FlowTable(P, 64), F.TableModel(64)
    k, f = F.traffic(rng, 640, 64)
    fid, upd = run_both(t, m, k)
    assert (upd == F.UPD_OK).all() and t.count() == 64
    F.check_records(t.flows(), m.records())
    t.clear()
    k, f = F.traffic(rng, 650, 65)
    fid, upd = (x.cpu().numpy() for x in t.update(to_dev(k)))
    lost = set(f[upd == F.UPD_FULL].tolist())
    assert len(lost) == 1 and (upd[f == lost.pop()] == F.UPD_FULL).all()  # one flow's packets, whichever it is
    F.check_full(t, k, upd, fid, 64)
    t.close()


def test_tag_bits_make_collisions(P):
    """As in test_flow_host: the model shows a COLLISION and three OK flows at tag_bits 2 (all it can hold), a
    COLLISION and at least four OK flows at tag_bits 3; the device table matches it."""
    import pktgpu
    rng = np.random.default_rng(2)
    for bits, min_ok in ((2, 3), (3, 4)):
        k, f = F.traffic(rng, 400, 24)
        m = F.TableModel(256, bits)
        flow, want = m.update(k["keys"], k["hash"], k["dir"], k["plen"], k["status"], 0)
        assert (want == F.UPD_COLLISION).any() and len(set(flow[flow >= 0].tolist())) >= min_ok
        t = pktgpu.FlowTable(P, 256)
        t.set_tag_bits(bits)
        fid, upd = (x.cpu().numpy() for x in t.update(to_dev(k)))
        assert np.array_equal(upd, want) and F.same_partition(fid, flow)
        F.check_records(t.flows(), m.records(), f"tag_bits {bits}")
        t.close()


def test_export_cap_clear_and_refusals(P):
    import pktgpu
    rng = np.random.default_rng(5)
    t, m = pktgpu.FlowTable(P, 2048), F.TableModel(2048)   # two tiles of the export's scan
    k, _ = F.traffic(rng, 3000, 700)
    fid, upd = run_both(t, m, k)
    full, cnt = t.export()
    assert cnt == 700 and len(full) == 700
    part, cnt = t.export(cap=333)
    assert cnt == 700 and part.tobytes() == full[:333].tobytes()
    none, cnt = t.export(cap=0)
    assert cnt == 700 and len(none) == 0
    slots = np.unique(fid)                                  # ascending slot order
    for j in (0, 350, 699):
        assert full["key"][j].tobytes() == k["keys"][int(np.flatnonzero(fid == slots[j])[0])].tobytes()
    t.clear()
    assert t.count() == 0 and len(t.flows()["first"]) == 0
    run_both(t, F.TableModel(2048), k)
    L, h = P._L, ctypes.c_void_p()
    for slots in (0, 32, 96, 1 << 29):
        assert L.pkt_flow_table_create(P._ctx, slots, ctypes.byref(h)) == -1
    args, out, keep = t._update_args(to_dev(k), base=3000)
    s = P._stream(None)
    assert L.pkt_flow_table_update(t._t, None, *args[1:], s) == -1 and L.pkt_flow_table_update(t._t, args[0], None, *args[2:], s) == -1
    assert L.pkt_flow_table_update(t._t, args[0] + 4, *args[1:], s) == -1
    assert L.pkt_flow_table_update(t._t, *args[:5], 1 << 32, 1 << 50, None, None, s) == -1
    assert t.count() == 700
    t.close()


def test_stream_windows_feed_one_table(P):
    """push -> poll -> flow_keys(st.batch(), the stream's columns) -> update(base = released records) ->
    release, in windows of `cap` records: the table ends as the model fed the whole capture at once."""
    import torch
    import pktgpu
    from pktgpu.stream import PcapStream
    rng = np.random.default_rng(12)
    pool = F.protocol_packets(rng) + F.symmetric_packets()
    pk = [pool[int(j)] for j in rng.integers(0, len(pool), 700)]
    b = C.indexed(pk, rng)
    whole = F.expect(F.case(b, symmetric=True))
    m = F.TableModel(1024)
    m.update(whole["keys"], whole["hash"], whole["dir"], whole["plen"], whole["status"], 0)
    cap = 256
    st = PcapStream(0, max_bytes=1 << 20, cap=cap, columns=["chain"])
    t = pktgpu.FlowTable(P, 1024)
    try:
        st.push(gen.pcap_bytes(pk))
        seen = 0
        while True:
            n, _ = st.poll()
            last = n <= cap
            if last:
                n, _ = st.finish()
            slab, offs, lens = st.batch()
            k = offs.numel()
            assert k == min(n, cap)
            chain = st.out if k == cap else {c: st.out[c][..., :k].contiguous() for c in ("n_hdrs", "hdr_type", "hdr_off")}
            keys = P.flow_keys(slab, chain, symmetric=True, seed=F.SEED, offsets=offs, lens=lens)
            base = st.released()[0]
            assert base == seen
            F.check({c: v.cpu().numpy() for c, v in keys.items()}, {c: v[seen:seen + k] for c, v in whole.items()}, f"window at {seen}")
            t.update(keys, base=base)
            seen += k
            if last:
                break
            torch.cuda.synchronize()  # the window's readers are done before the stream moves it
            st.release(cap)
        assert seen == 700
        F.check_records(t.flows(), m.records(), "stream")
    finally:
        t.close()
        st.close()


def test_65536_packets_4096_flows_both_directions(P):
    """2^16 Ether/IPv4/UDP packets of 2^12 connections in random order and direction: parse, symmetric keys
    (equal to the host twin's; the first 256 to the yardstick's), one update; the partition by flow_id is the
    partition by key and the records are the dict model's."""
    import pktgpu
    n, nf = 1 << 16, 1 << 12
    rng = np.random.default_rng(16)
    ends = rng.integers(0, 256, (nf, 2, 6), dtype=np.uint8)        # per flow: two (address, port) ends
    ends[:, 0, 0], ends[:, 1, 0] = 10, 11
    ends[:, 0, 1:3] = np.arange(nf, dtype=np.uint16).view(np.uint8).reshape(nf, 2)  # distinct flows
    f, flip = rng.integers(0, nf, n), rng.integers(0, 2, n)
    f[:nf] = rng.permutation(nf)
    a = np.tile(gen.gen_c2(1, seed=3).reshape(1, 64), (n, 1))
    s, d = ends[f, flip], ends[f, 1 - flip]
    a[:, 26:30], a[:, 30:34], a[:, 34:36], a[:, 36:38] = s[:, :4], d[:, :4], s[:, 4:], d[:, 4:]
    a[:, 20:22] = (0x40, 0)
    kw, big = dev_batch(C.batch(a, stride=64))
    chain = P.parse(kw["slab"], stride=64, columns=["chain"])
    keys = P.flow_keys(kw["slab"], chain, symmetric=True, seed=F.SEED, rss_key=F.RSS_KEY, stride=64)
    hk = {c: v.cpu().numpy() for c, v in keys.items()}
    hchain = {c: chain[c].cpu().numpy() for c in ("n_hdrs", "hdr_type", "hdr_off")}
    F.check(hk, pktgpu.flow_keys(a, hchain, symmetric=True, seed=F.SEED, rss_key=F.RSS_KEY, stride=64), "host twin")
    for i in range(256):
        w = F.one(a[i].tobytes(), F.chain_rows(hchain, i), F.LAST, True)
        assert (hk["keys"][i].tobytes(), int(hk["hash"][i]), int(hk["rss"][i]), hk["dir"][i]) == (w["key"], w["hash"], w["rss"], w["dir"]), i
    assert 0 < hk["dir"].sum() < n
    t, m = pktgpu.FlowTable(P, 1 << 14), F.TableModel(1 << 14)
    fid, upd = (x.cpu().numpy() for x in t.update(keys, base=7))
    flow, want = m.update(hk["keys"], hk["hash"], hk["dir"], hk["plen"], hk["status"], 7)
    assert (upd == F.UPD_OK).all() and np.array_equal(upd, want) and F.same_partition(fid, flow)
    assert len(np.unique(fid)) == nf == t.count()
    _, inv = np.unique(hk["keys"], axis=0, return_inverse=True)
    assert F.same_partition(fid, inv.reshape(-1))                   # the partition by flow_id is the partition by key
    F.check_records(t.flows(), m.records(), "2^16")
    t.close()
