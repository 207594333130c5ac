"""pkt_frag_batch / _async / _result (Parser.fragment): the kernels of pktgpu_frag.hip against frag_cases' yardstick
(an independent Python model) and the host twin pkt_frag_host.  The decision and the fragment header are covered on
the CPU (test_frag_host.py: the host twin runs the same inline code); here it is the loads, the scan, the emitted
table and the copy.  dst and every output array lie between two guard regions filled with 0xA5, the outputs start as
0x77, and dst at and past the total must still be 0x77 after the call."""
import ctypes

import numpy as np
import pytest

import pktgpu
from pktgpu import schema

import frag_cases as G

pytestmark = pytest.mark.gpu
GUARD = 4096
FILL = 0x77
INVALID = -1
N_MIX = 3 * 256 + 131  # three tiles of the decision kernel and a ragged one


@pytest.fixture(scope="module")
def P():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible")
    return pktgpu.Parser(0)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def guarded(nbytes, fill=None):
    """A 0xA5-filled allocation with `nbytes` in its middle (filled with `fill`) -> (all, middle)."""
    import torch
    big = torch.full((GUARD + (nbytes + 15) // 16 * 16 + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    mid = big[GUARD:GUARD + nbytes]
    if fill is not None:
        mid.fill_(fill)
    return big, mid


def guards_intact(big, mid):
    lo = mid.data_ptr() - big.data_ptr()
    return bool((big[:lo] == 0xA5).all()) and bool((big[lo + mid.numel():] == 0xA5).all())


SHAPES = dict(status=np.uint8, nfrag=np.uint32, first=np.uint32, out_off=np.uint64, out_len=np.uint32, src_index=np.uint32,
              frag_index=np.uint16, oc_n_hdrs=np.uint8, oc_hdr_type=np.uint8, oc_hdr_off=np.uint16, hits=np.uint64)


def run(P, b, ch, mtu, select=None, which=0, flags=0, cap=None, dst_len=None, skip=(), mode="sync", over=None):
    """pkt_frag_batch over a device copy of the batch -> (rc, got, guards intact).  cap / dst_len default to the
    model-free sizing pass (PKT_FRAG_NO_WRITE).  hits start as 0x77.. and come back less that."""
    import torch
    L = P._L
    slab = dev(b["slab"])
    offs = None if b["offsets"] is None else dev(b["offsets"])
    lens = None if b["lens"] is None else dev(b["lens"])
    pb = P._batch(slab, b["n"], b["stride"], offs, lens)
    dch = {k: dev(v) for k, v in ch.items()}
    pc = P._chain(dch)
    n = b["n"]
    per = not np.isscalar(mtu)
    mt = dev(np.asarray(mtu, np.uint16)) if per else None
    sel = None if select is None else dev(np.asarray(select, np.uint8))
    tp = lambda t: t.data_ptr() if t is not None and t.numel() else None  # noqa: E731
    tot, cnt = ctypes.c_uint64(0), ctypes.c_uint64(0)
    head = [P._ctx, ctypes.byref(pb), ctypes.byref(pc), which]
    if cap is None or dst_len is None:
        rc = L.pkt_frag_batch(*head, flags | G.NO_WRITE, tp(mt), 0 if per else int(mtu), tp(sel), None, None, None, None, 0, 0,
                              None, None, None, None, None, None, ctypes.byref(tot), ctypes.byref(cnt), P._stream(None))
        assert rc == 0
        cap = max(1, cnt.value) if cap is None else cap
        dst_len = tot.value if dst_len is None else dst_len
    counts = dict(status=n, nfrag=n, first=n, out_off=cap, out_len=cap, src_index=cap, frag_index=cap, oc_n_hdrs=cap,
                  oc_hdr_type=G.MAXH * cap, oc_hdr_off=G.MAXH * cap, hits=G.NSTATUS)
    if flags & G.NO_WRITE:
        skip = set(skip) | {"dst", "out_off", "out_len", "src_index", "frag_index", "oc_n_hdrs", "oc_hdr_type", "oc_hdr_off"}
    bufs = {k: guarded(counts[k] * np.dtype(dt).itemsize, FILL) for k, dt in SHAPES.items() if k not in skip}
    if "dst" not in skip:
        bufs["dst"] = guarded(dst_len + 64, FILL)  # 64 more bytes the call is not told of
    p = lambda k: bufs[k][1].data_ptr() if k in bufs and bufs[k][1].numel() else None  # noqa: E731
    oc = P._lib.PktChain(p("oc_n_hdrs"), p("oc_hdr_type"), p("oc_hdr_off"))
    args = head + [flags, tp(mt), 0 if per else int(mtu), tp(sel), p("status"), p("nfrag"), p("first"), p("dst"), dst_len, cap,
                   p("out_off"), p("out_len"), p("src_index"), p("frag_index"), ctypes.byref(oc), p("hits")]
    for k, v in dict(over or {}).items():
        args[k] = v
    if mode == "sync":
        rc = L.pkt_frag_batch(*args, ctypes.byref(tot), ctypes.byref(cnt), P._stream(None))
    else:
        rc = L.pkt_frag_batch_async(*args, P._stream(None))
        if rc == 0:
            if mode == "async_twice":  # the one-in-flight rule
                rc2 = L.pkt_frag_batch_async(*args, P._stream(None))
                assert rc2 == INVALID and P._L.pkt_ctx_last_error(P._ctx).decode().startswith("pkt_frag")
                assert "pkt_frag_result" in P._L.pkt_ctx_last_error(P._ctx).decode()
            rc = L.pkt_frag_result(P._ctx, ctypes.byref(tot), ctypes.byref(cnt))
    torch.cuda.synchronize()
    got = {k: g[1].cpu().numpy().view(SHAPES.get(k, np.uint8)) for k, g in bufs.items()}
    if "hits" in got:
        got["hits"] = got["hits"] - np.uint64(0x7777777777777777)
    got["n_out"], got["bytes_out"], got["cap"] = cnt.value, tot.value, cap
    intact = all(guards_intact(*g) for g in bufs.values())
    return rc, got, intact


def verify(got, want, label):
    G.check(got, want, got["cap"], label)
    assert (got["dst"][want["bytes_out"]:] == FILL).all(), (label, "dst written at or past the total")


def twin(b, ch, mtu, select=None, which=0, flags=0, cap=None, dst_len=None):
    rc, h = G.host_call(b, ch, mtu, select, which, flags, cap=cap, dst_len=dst_len)
    assert rc == 0
    return h


def same_as_twin(got, h, label):
    k, nb = h["n_out"], h["bytes_out"]
    assert (got["n_out"], got["bytes_out"]) == (k, nb), label
    assert np.array_equal(got["dst"][:nb], h["dst"][:nb]), (label, "dst")
    for name in SHAPES:
        if name in got and name in h and not name.startswith("oc_hdr"):
            assert np.array_equal(got[name], h[name]), (label, name)


def mix(kind):
    def build():
        items, mtu, sel = G.mix(N_MIX, big=kind == "indexed")
        b, ch = G.layout(items, kind)
        return b, ch, mtu, sel, G.expect(b, ch, mtu, sel)
    return G.cached(("dev_mix", kind), build)


# ------------------------------------------------------------------ the mix, both layouts
@pytest.mark.parametrize("kind", ["indexed", "stride"])
def test_mix_against_the_model_and_the_host_twin(P, kind):
    """60..1600-byte packets, a few of 9000 and (indexed) two of 65535, mtus of 28 / 68 / 576 / 1500 per packet, source
    packets at every alignment 0..15, ip_off 14, 18 and 64, more than three tiles of the decision kernel."""
    b, ch, mtu, sel, want = mix(kind)
    counts = np.bincount(want["status"], minlength=G.NSTATUS)
    assert all(counts[s] >= 3 for s in (G.FITS, G.SPLIT, G.SKIPPED, G.NO_IP, G.IPV6, G.DF)), counts
    if kind == "indexed":
        assert {int(o) % 16 for o in b["offsets"][:16]} == set(range(16)) and int(b["offsets"][-1]) + int(b["lens"][-1]) == b["slab"].size
        assert sorted(b["lens"])[-2:] == [65535, 65535]
    rc, got, intact = run(P, b, ch, mtu, sel)
    assert rc == 0 and intact
    verify(got, want, kind)
    same_as_twin(got, twin(b, ch, mtu, sel), kind)
    assert int(got["hits"].sum()) == b["n"]


def test_4098_tiles_the_scan_in_two_rounds_and_the_counting_grid_capped(P):
    """4096 * 256 + 256 + 3 packets: the one-block scan of the tile sums takes 4096 tiles a round, so its second round
    holds two tiles, the last one ragged, and first[] / out_off check every tile's prefix across the two rounds; with
    hits the decision launch is capped at 1280 blocks, so a block takes up to four tiles.  60-byte Ether / IPv4 / UDP
    packets at stride 64, mtu 0 (FITS) and 28 (SPLIT into 4) in turn, every 61st packet selected (about four a tile, at
    varying places).  Against the host twin alone: the Python model is too slow at this size, and test_frag_host.py
    holds the twin to it."""
    n = 4096 * 256 + 256 + 3
    b, ch = G.tiled([G.v4(26, seed=k) for k in range(4)], n)
    mtu = np.where(np.arange(n) % 2 == 0, 0, 28).astype(np.uint16)
    sel = (np.arange(n) % 61 == 0).astype(np.uint8)
    rc, got, intact = run(P, b, ch, mtu, sel)
    assert rc == 0 and intact
    h = twin(b, ch, mtu, sel)
    counts = np.bincount(h["status"], minlength=G.NSTATUS)
    assert counts[G.FITS] > 8000 and counts[G.SPLIT] > 8000 and counts[G.SKIPPED] == n - counts[G.FITS] - counts[G.SPLIT]
    assert set(h["nfrag"][h["status"] == G.SPLIT]) == {4} and h["n_out"] == counts[G.FITS] + 4 * counts[G.SPLIT]
    same_as_twin(got, h, "4098 tiles")
    assert np.array_equal(got["hits"], counts) and (got["dst"][h["bytes_out"]:] == FILL).all()


def test_two_runs_give_identical_bytes_and_arrays(P):
    b, ch, mtu, sel, want = mix("stride")
    r1, g1, i1 = run(P, b, ch, mtu, sel)
    r2, g2, i2 = run(P, b, ch, mtu, sel)
    assert r1 == r2 == 0 and i1 and i2
    for k in g1:
        assert np.array_equal(g1[k], g2[k]), k


@pytest.mark.parametrize("which", [0, G.LAST])
def test_inner_and_outer_headers_of_vxlan(P, which):
    items = [G.vxlan(1000 + 3 * i, seed=i) for i in range(70)] + [G.v4(900, vlan=True, pad=2)]
    b, ch = G.layout(items)
    want = G.expect(b, ch, 576, None, which)
    rc, got, intact = run(P, b, ch, 576, which=which)
    assert rc == 0 and intact
    verify(got, want, f"vxlan {which}")


# ------------------------------------------------------------------ one case each
def test_every_packet_split_and_none(P):
    items = [G.v4(600 + 7 * i, vlan=i % 2 == 1, seed=i, pad=i % 3) for i in range(300)]
    b, ch = G.layout(items)
    for m, st in ((576, G.SPLIT), (0, G.FITS), (3000, G.FITS)):
        want = G.expect(b, ch, m)
        assert (want["status"] == st).all()
        rc, got, intact = run(P, b, ch, m)
        assert rc == 0 and intact
        verify(got, want, f"mtu {m}")
    want = G.expect(b, ch, 3000, flags=G.ONLY_SPLIT)
    rc, got, intact = run(P, b, ch, 3000, flags=G.ONLY_SPLIT)
    assert rc == 0 and intact and got["n_out"] == 0
    verify(got, want, "only_split, none split")


def test_a_single_packet_of_8190_fragments(P):
    """65535 bytes that start at their IPv4 header (a parse with PKT_ENTRY_IPV4), mtu 28: ceil(65515 / 8) fragments,
    more rows than one round of a wave."""
    p = G.ip4_hdr(65535) + G.pattern(65515, 3)
    b, ch = G.layout([(p, [(G.T_IPV4, 0)])])
    want = G.expect(b, ch, 28)
    assert want["n_out"] == 8190 and want["nfrag"].tolist() == [8190]
    rc, got, intact = run(P, b, ch, 28)
    assert rc == 0 and intact
    verify(got, want, "8190")
    assert got["frag_index"][-1] == 8189 and int(got["out_len"][-1]) == 20 + 3


def test_n_out_landing_on_out_cap_and_one_below_the_need(P):
    b, ch, mtu, sel, want = mix("stride")
    rc, got, intact = run(P, b, ch, mtu, sel, cap=want["n_out"], dst_len=want["bytes_out"])
    assert rc == 0 and intact
    verify(got, want, "exact")
    for cap, room in ((want["n_out"] - 1, want["bytes_out"]), (want["n_out"], want["bytes_out"] - 16)):
        rc, got, intact = run(P, b, ch, mtu, sel, cap=cap, dst_len=room)
        assert rc == INVALID and intact
        assert P._L.pkt_ctx_last_error(P._ctx).decode().startswith("pkt_frag")
        assert (got["n_out"], got["bytes_out"]) == (want["n_out"], want["bytes_out"])
        for k in ("status", "nfrag", "hits"):
            assert np.array_equal(got[k], want[k]), k
    rc, got, intact = run(P, b, ch, mtu, sel, cap=want["n_out"] + 300, dst_len=want["bytes_out"] + 8192)
    assert rc == 0 and intact
    verify(got, want, "empty tail")


def test_no_write_and_null_outputs(P):
    b, ch, mtu, sel, want = mix("stride")
    rc, got, intact = run(P, b, ch, mtu, sel, flags=G.NO_WRITE)
    assert rc == 0 and intact
    G.check(got, want, 0, "no_write")
    for skip in (["status", "nfrag", "first", "hits"], ["src_index", "frag_index"], ["oc_n_hdrs", "oc_hdr_type", "oc_hdr_off"],
                 ["src_index", "oc_hdr_off", "first"]):
        rc, got, intact = run(P, b, ch, mtu, sel, skip=skip)
        assert rc == 0 and intact, skip
        verify(got, want, str(skip))


def test_async_result_and_one_in_flight(P):
    b, ch, mtu, sel, want = mix("stride")
    for mode in ("async", "async_twice"):
        rc, got, intact = run(P, b, ch, mtu, sel, mode=mode)
        assert rc == 0 and intact
        verify(got, want, mode)
    tot, cnt = ctypes.c_uint64(5), ctypes.c_uint64(5)
    assert P._L.pkt_frag_result(P._ctx, ctypes.byref(tot), ctypes.byref(cnt)) == INVALID
    assert P._L.pkt_ctx_last_error(P._ctx).decode().startswith("pkt_frag_result")
    rc, got, intact = run(P, b, ch, mtu, sel, cap=want["n_out"] - 1, dst_len=want["bytes_out"], mode="async")
    assert rc == INVALID and intact and (got["n_out"], got["bytes_out"]) == (want["n_out"], want["bytes_out"])


def test_n_0(P):
    b, ch = G.layout([G.v4(100)])
    b = dict(b, n=0, offsets=b["offsets"][:1], lens=b["lens"][:1])
    rc, got, intact = run(P, b, ch, 576, cap=70, dst_len=64, skip=["status", "nfrag", "first"])
    assert rc == 0 and intact and (got["n_out"], got["bytes_out"]) == (0, 0)
    assert (got["out_off"] == 0).all() and (got["out_len"] == 0).all() and (got["src_index"] == G.NONE).all()
    assert (got["frag_index"] == 0).all() and (got["oc_n_hdrs"] == 0).all() and (got["dst"] == FILL).all()
    assert (got["hits"] == 0).all()


# ------------------------------------------------------------------ the next calls take the output
def test_fwd_flow_key_and_pcap_write_over_the_output(P):
    import torch
    items, mtu, sel = G.mix(400, seed=21, big=False)
    b, ch = G.layout(items)
    mt = dev(mtu)
    r = P.fragment(dict(slab=dev(b["slab"]), offsets=dev(b["offsets"]), lens=dev(b["lens"])), {k: dev(v) for k, v in ch.items()},
                   mtu=mt, select=dev(sel), hits=True)
    h = pktgpu.Parser.fragment(None, b, ch, mtu=mtu, select=sel, hits=True, host=True)
    k = h.n_out
    assert r.n_out == k and r.bytes_out == h.bytes_out and np.array_equal(r.hits.cpu().numpy(), h.hits)
    for name in ("status", "nfrag", "first", "offsets", "lens", "src_index", "frag_index"):
        assert np.array_equal(getattr(r, name).cpu().numpy(), getattr(h, name)), name
    assert np.array_equal(r.slab.cpu().numpy()[:h.bytes_out], h.slab[:h.bytes_out])
    assert np.array_equal(r.out_chain["n_hdrs"].cpu().numpy(), h.out_chain["n_hdrs"])
    # each output forwards at the mtu its source was cut to
    out_mtu = mtu[h.src_index[:k]]
    adj = [("02:00:00:00:00:01", "02:00:00:00:00:02", 9, int(m)) for m in G.MTUS]
    nh = np.searchsorted(np.asarray(G.MTUS), out_mtu).astype(np.uint32)
    fd = P.forwarder(adj).run(r.batch(), r.out_chain, nexthop=dev(nh))
    hb = dict(slab=h.slab.copy(), offsets=h.offsets, lens=h.lens)
    fh = pktgpu.Forwarder(None, adj).run(hb, h.out_chain, nexthop=nh)
    torch.cuda.synchronize()
    for name in ("status", "port"):
        assert np.array_equal(fd[name].cpu().numpy(), fh[name]), name
    ok4 = (h.status[h.src_index[:k]] == G.SPLIT)
    assert (fh["status"][:k][ok4] == pktgpu.FWD_OK).all() and (fh["status"][k:] == pktgpu.FWD_NO_IP).all()
    assert np.array_equal(r.slab.cpu().numpy()[:h.bytes_out], hb["slab"][:h.bytes_out])
    kd = P.flow_keys(r.slab, r.out_chain, which_ip=0, offsets=r.offsets, lens=r.lens)
    kh = pktgpu.flow_keys(hb["slab"], h.out_chain, which_ip=0, offsets=h.offsets, lens=h.lens)
    for name in ("keys", "hash", "status"):
        assert np.array_equal(kd[name].cpu().numpy(), kh[name]), name
    keys = kh["keys"].view(schema.FLOW_KEY_DTYPE).reshape(-1)[:k]
    assert (keys["sport"][ok4] == 0).all() and (keys["dport"][ok4] == 0).all()
    cap, nrec, ro, rl, rs = P.pcap_write(r.slab, offsets=r.offsets[:k], lens=r.lens[:k])
    hc, hn, ho, hl, hs = pktgpu.pcap_write(hb["slab"], offsets=h.offsets[:k], lens=h.lens[:k])
    assert nrec == hn == k and np.array_equal(cap.cpu().numpy(), hc)


# ------------------------------------------------------------------ refusals
A_BATCH, A_CHAIN, A_WHICH, A_FLAGS, A_MTU, A_MTU_ALL, A_SELECT, A_STATUS, A_NFRAG, A_FIRST, A_DST, A_DST_LEN, A_CAP, A_OFF, \
    A_LEN = range(1, 16)
A_HITS = 19


def test_refusal_texts(P):
    import torch
    b, ch = G.layout([G.v4(1000), G.v4(100)])
    odd = torch.zeros(64, dtype=torch.uint8, device="cuda")
    base = odd.data_ptr()
    cases = {"n >= 2^32": None, "which_ip": {A_WHICH: 16}, "flag": {A_FLAGS: 8}, "mtu_all": {A_MTU: None, A_MTU_ALL: 65536},
             "dst not 16": {A_DST: base + 8}, "hits not 8": {A_HITS: base + 4}, "out_off not 8": {A_OFF: base + 4},
             "mtu not 2": {A_MTU: base + 1}, "null dst": {A_DST: None}, "null dst, out_off": {A_OFF: None},
             "out_len": {A_LEN: None}, "out_cap": {A_CAP: 0}, "out_cap is 0 or": {A_CAP: 1 << 32}, "null argument": {A_CHAIN: None}}
    for text, over in cases.items():
        if over is None:
            continue
        rc, got, intact = run(P, b, ch, np.asarray([576, 576], np.uint16), cap=8, dst_len=4096, over=over)
        msg = P._L.pkt_ctx_last_error(P._ctx).decode()
        assert rc == INVALID and intact and msg.startswith("pkt_frag_batch: ") and text in msg, (text, msg)
        assert (got["status"] == FILL).all() and (got["dst"] == FILL).all() and (got["hits"] == 0).all(), text
    for form, text in (("n", "n >= 2^32"), ("lens", "offsets without lens"), ("slab", "slab not 16-byte aligned"), ("col", "null chain column")):
        slab = dev(b["slab"])
        pb = P._batch(slab, b["n"], None, dev(b["offsets"]), dev(b["lens"]))
        dch = {k: dev(v) for k, v in ch.items()}
        pc = P._chain(dch)
        if form == "n":
            pb.n = 1 << 32
        elif form == "lens":
            pb.lens = None
        elif form == "slab":
            pb.slab = slab.data_ptr() + 1
        else:
            pc.hdr_off = None
        tot, cnt = ctypes.c_uint64(7), ctypes.c_uint64(7)
        rc = P._L.pkt_frag_batch(P._ctx, ctypes.byref(pb), ctypes.byref(pc), 0, G.NO_WRITE, None, 576, None, None, None, None, None, 0,
                                 0, None, None, None, None, None, None, ctypes.byref(tot), ctypes.byref(cnt), P._stream(None))
        msg = P._L.pkt_ctx_last_error(P._ctx).decode()
        assert rc == INVALID and msg.startswith("pkt_frag_batch: ") and text in msg and (tot.value, cnt.value) == (0, 0), (form, msg)
