"""pkt_tunnel_create and pkt_tunnel_encap_batch / pkt_tunnel_decap_batch with their _async / _result forms
(Parser.tunnels): the kernels of pktgpu_tunnel.hip against tunnel_cases' yardstick (an independent Python model) and the
host twins, and the properties that tie the outputs to the rest of the library (parse, l4_checksum, Forwarder, fragment,
reassemble).  The decisions and the header words are covered on the CPU (test_tunnel_host.py: the twins run the same
inline code); here it is the loads, the lookup on the device, the scan, the chunk walk with its three sources and the
payload's sum.  dst and every output array lie between two guard regions filled with 0xA5, the outputs start as 0x77,
and dst at and past the total must still be 0x77 after the call."""
import ctypes

import numpy as np
import pytest

import pktgpu
from pktgpu import schema

import tunnel_cases as T

pytestmark = pytest.mark.gpu
GUARD = 4096
FILL = 0x77
INVALID = -1
ENTS = T.table()
N_MIX = 2 * 256 + 131  # two tiles of the decision kernel and a ragged one


@pytest.fixture(scope="module")
def P():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible")
    return pktgpu.Parser(0)


@pytest.fixture(scope="module")
def TUN(P):
    return P.tunnels(T.records(ENTS))


@pytest.fixture(scope="module")
def HT():
    return T.HostTable(ENTS)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def h(t):
    return None if t is None else t.cpu().numpy()


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


def dev_batch(P, b, ch):
    slab = dev(b["slab"])
    offs = None if b["offsets"] is None else dev(b["offsets"])
    lens = None if b["lens"] is None else dev(b["lens"])
    dch = {k: dev(v) for k, v in ch.items()}
    return P._batch(slab, b["n"], b["stride"], offs, lens), P._chain(dch), (slab, offs, lens, dch)


def run(P, TUN, op, b, ch, tunnel=0, entropy=None, ident=0, select=None, which=0, flags=0, cap=None, dst_len=None, skip=(),
        mode="sync", over=None):
    """pkt_tunnel_<op>_batch over a device copy of the batch -> (rc, got, guards intact).  cap / dst_len default to the
    model-free sizing pass (PKT_TUN_NO_WRITE).  hits start as 0x77.. and come back less that."""
    import torch
    L = P._L
    fn, fa, fr = (getattr(L, f"pkt_tunnel_{op}_{s}") for s in ("batch", "batch_async", "result"))
    pb, pc, keep = dev_batch(P, b, ch)
    n = b["n"]
    tp = lambda t: t.data_ptr() if t is not None and t.numel() else None  # noqa: E731
    tn = None if np.isscalar(tunnel) else dev(np.asarray(tunnel, np.uint32))
    en = None if entropy is None else dev(np.asarray(entropy, np.uint32))
    sel = None if select is None else dev(np.asarray(select, np.uint8))
    per = (tp(tn), 0 if tn is not None else int(tunnel), tp(en), ident, tp(sel))
    tot, cnt = ctypes.c_uint64(0), ctypes.c_uint64(0)
    head = [P._ctx, ctypes.byref(pb), ctypes.byref(pc), which, flags]
    if cap is None or dst_len is None:
        sizing = T.call_args(op, head[:4] + [flags | T.NO_WRITE], TUN._t, per, lambda k: None, 0, 0, None)
        rc = fn(*sizing, ctypes.byref(tot), ctypes.byref(cnt), P._stream(None))
        assert rc == 0, L.pkt_ctx_last_error(P._ctx)
        cap = max(1, cnt.value) if cap is None else cap
        dst_len = tot.value if dst_len is None else dst_len
    cn = T.counts(op, n, cap)
    if flags & T.NO_WRITE:
        skip = set(skip) | T.PER_OUTPUT
    bufs = {k: guarded(cn[k] * np.dtype(T.SHAPES[k]).itemsize, FILL) for k in cn if k not in skip}
    if "dst" not in skip:
        bufs["dst"] = guarded(dst_len + 64, FILL)  # 64 more bytes the call is not told of
    p = lambda k: bufs[k][1].data_ptr() if k in bufs and bufs[k][1].numel() else None  # noqa: E731
    oc = P._lib.PktChain(p("oc_n_hdrs"), p("oc_hdr_type"), p("oc_hdr_off"))
    args = T.call_args(op, head, TUN._t, per, p, dst_len, cap, oc)
    for k, v in dict(over or {}).items():
        args[k + 1] = v  # the positions are the host twin's: the ctx comes first here
    if mode == "sync":
        rc = fn(*args, ctypes.byref(tot), ctypes.byref(cnt), P._stream(None))
    else:
        rc = fa(*args, P._stream(None))
        if rc == 0:
            if mode == "async_twice":  # the one-in-flight rule
                rc2 = fa(*args, P._stream(None))
                msg = L.pkt_ctx_last_error(P._ctx).decode()
                assert rc2 == INVALID and msg.startswith(f"pkt_tunnel_{op}_batch") and f"pkt_tunnel_{op}_result" in msg, msg
            rc = fr(P._ctx, ctypes.byref(tot), ctypes.byref(cnt))
    torch.cuda.synchronize()
    got = {k: g[1].cpu().numpy().view(T.SHAPES.get(k, np.uint8)) for k, g in bufs.items()}
    if "hits" in got:
        got["hits"] = got["hits"] - np.uint64(0x7777777777777777)
    got["n_out"], got["bytes_out"], got["cap"] = cnt.value, tot.value, cap
    return rc, got, all(guards_intact(*g) for g in bufs.values())


def verify(got, want, label):
    T.check_all(got, want, got["cap"], label)
    assert (got["dst"][want["bytes_out"]:] == FILL).all(), (label, "dst written at or past the total")


def same_as_twin(got, hgot, label):
    k, nb = hgot["n_out"], hgot["bytes_out"]
    assert (got["n_out"], got["bytes_out"]) == (k, nb), label
    assert np.array_equal(got["dst"][:nb], hgot["dst"][:nb]), (label, "dst")
    for name in T.SHAPES:
        if name in got and name in hgot and not name.startswith("oc_hdr"):
            assert np.array_equal(got[name], hgot[name]), (label, name)


def emix(kind):
    def build():
        items, tun, ent, sel = T.encap_mix(N_MIX)
        b, ch = T.layout(items, kind)
        return b, ch, tun, ent, sel, T.expect("encap", b, ch, ENTS, tun, ent, 65000, sel, T.LAST if kind == "stride" else 0)
    return T.cached(("dev emix", kind), build)


def dmix(kind):
    def build():
        items, sel = T.decap_mix(N_MIX)
        b, ch = T.layout(items, kind)
        return b, ch, sel, T.expect("decap", b, ch, ENTS, select=sel)
    return T.cached(("dev dmix", kind), build)


# ------------------------------------------------------------------ the mixes, both layouts
@pytest.mark.parametrize("kind", ["indexed", "stride"])
def test_encap_mix_against_the_model_and_the_host_twin(P, TUN, HT, kind):
    """Every written byte and every output array: the 22 reference packets, 0..2 VLAN tags, MPLS, raw IP, IPv4 and IPv6
    inners, per-packet tunnels over 3 kinds x 2 outer versions with every flag, entropy, select, forged chains; indexed
    with packet i at alignment i % 16 and the last packet ending on the slab's last byte (which_ip 0), and fixed stride
    (which_ip LAST)."""
    b, ch, tun, ent, sel, want = emix(kind)
    which = T.LAST if kind == "stride" else 0
    rc, got, intact = run(P, TUN, "encap", b, ch, tun, ent, 65000, sel, which)
    assert rc == 0 and intact
    verify(got, want, kind)
    assert got["hits"].sum() == b["n"]
    rc, hgot = T.host_call("encap", HT, b, ch, tun, ent, 65000, sel, which)
    same_as_twin(got, hgot, kind)


@pytest.mark.parametrize("kind", ["indexed", "stride"])
def test_decap_mix_against_the_model_and_the_host_twin(P, TUN, HT, kind):
    b, ch, sel, want = dmix(kind)
    assert np.bincount(want["status"], minlength=11).all()
    rc, got, intact = run(P, TUN, "decap", b, ch, select=sel)
    assert rc == 0 and intact
    verify(got, want, kind)
    assert got["hits"].sum() == b["n"]
    rc, hgot = T.host_call("decap", HT, b, ch, select=sel)
    same_as_twin(got, hgot, kind)


@pytest.mark.parametrize("n", [0, 1, 64, 65, 256, 257])
def test_sizes_at_the_wave_and_tile_edges(P, TUN, n):
    """n = 0 writes the empty tail alone; `tunnel` as tunnel_all (a UDP_CSUM entry) and as an array."""
    items, tun, ent, _ = T.encap_mix(257)
    b, ch = T.layout(items[:max(n, 1)], "indexed")
    b = dict(b, n=n)  # n = 0: a batch of one packet that the call is told nothing of
    for tn in (6, tun[:max(n, 1)]):
        want = T.expect("encap", b, ch, ENTS, tn, ent, 7)
        rc, got, intact = run(P, TUN, "encap", b, ch, tn, ent[:max(n, 1)], 7, cap=max(1, want["n_out"]) + 3, dst_len=want["bytes_out"] + 32)
        assert rc == 0 and intact
        verify(got, want, n)
    eb, ech = T.layout(T.tunnelled(items[:max(n, 1)], 1, ent), "indexed")
    eb = dict(eb, n=min(n, eb["n"]))
    want = T.expect("decap", eb, ech, ENTS)
    rc, got, intact = run(P, TUN, "decap", eb, ech, cap=max(1, want["n_out"]) + 3, dst_len=want["bytes_out"] + 32)
    assert rc == 0 and intact
    verify(got, want, n)


def test_fixed_stride_c2(P, TUN):
    """The flagship's 64-byte packets (gen.gen_c2) into VXLAN with and without UDP_CSUM, GRE / IPv6 and back."""
    from pktgpu import gen
    n = 1024 + 17
    c2 = gen.gen_c2(n, seed=3)
    b = T.C.batch(c2.reshape(-1), stride=64, n=n)
    ch = T.C.chain_of(dict(b, lens=None, offsets=None))
    ent = (np.arange(n, dtype=np.uint64) * 2654435761 % (1 << 32)).astype(np.uint32)
    for t in (0, 6, 3):
        want = T.expect("encap", b, ch, ENTS, t, ent, 9)
        rc, got, intact = run(P, TUN, "encap", b, ch, t, ent, 9)
        assert rc == 0 and intact and got["n_out"] == n
        verify(got, want, t)
        eb, ech = T.layout(T.out_items(got), "stride", stride=144)
        rc, back, intact = run(P, TUN, "decap", eb, ech)
        assert rc == 0 and intact and back["n_out"] == n and (back["tunnel_out"] == t + 14).all()
        verify(back, T.expect("decap", eb, ech, ENTS), ("decap", t))


def test_outer_length_edges_and_row_edges(P, TUN):
    """Outer lengths of exactly 65535 (OK) and 65536 (TOO_BIG); rows landing on exactly 16 (OK) and 17 (DEPTH)."""
    items = [T.big(65535 - 36 - 14), T.big(65536 - 36 - 14), T.big(65535 - 16 - 14), T.big(65536 - 16 - 14),
             T.big(65535 - 24), T.big(65536 - 24), T.big(65535 - 28), T.big(65536 - 28),
             T.big(65535 - 20, v6=True), T.big(65536 - 20, v6=True),
             T.deep(12), T.deep(13), T.deep(15), T.deep(16), T.deep(13), T.deep(14), T.deep(14), T.deep(15)]
    tun = np.array([6, 6, 1, 1, 2, 2, 7, 7, 4, 4, 0, 0, 4, 4, 3, 3, 2, 2], np.uint32)
    b, ch = T.layout(items, "indexed")
    want = T.expect("encap", b, ch, ENTS, tun)
    assert list(want["status"]) == [T.E_OK, T.E_TOO_BIG] * 5 + [T.E_OK, T.E_DEPTH] * 4
    rc, got, intact = run(P, TUN, "encap", b, ch, tun)
    assert rc == 0 and intact
    verify(got, want, "edges")
    eb, ech = T.layout(T.out_items(got), "indexed")
    rc, back, intact = run(P, TUN, "decap", eb, ech)
    assert rc == 0 and intact
    verify(back, T.expect("decap", eb, ech, ENTS), "edges back")


def test_forged_chains_read_nothing_outside_the_slab(P, TUN):
    """Offsets past the packet and n_hdrs 255: a status, the model's outputs, and the slab is an exact-size tensor whose
    last packet ends on its last byte."""
    items = T.forged()
    b, ch = T.layout(items, "indexed")
    ch = dict(ch, n_hdrs=np.where(np.arange(len(items)) % 2, 255, ch["n_hdrs"]).astype(np.uint8))
    for t in (0, 2, 5, 6):
        rc, got, intact = run(P, TUN, "encap", b, ch, t)
        assert rc == 0 and intact
        verify(got, T.expect("encap", b, ch, ENTS, t), t)
    rc, got, intact = run(P, TUN, "decap", b, ch)
    assert rc == 0 and intact
    verify(got, T.expect("decap", b, ch, ENTS), "decap")


# ------------------------------------------------------------------ properties
def parsed_sources():
    """Sources whose chains are the parser's own: the reference packets and Ether / VLAN / IP / UDP ones."""
    items = T.ref22() + [T.pkt(T.udp(20 + 7 * k, k), v6=bool(k & 1), vlans=k % 3) for k in range(106)]
    return [(p, hd) for p, hd in items if hd == T.L4.hdrs_of(p) and hd and hd[0][0] == T.T_ETHER]


def test_parse_of_the_output_gives_out_chain_and_the_checksums_hold(P, TUN):
    """For Ether-entry sources a parse of the encap output gives exactly out_chain, its ipv4_csum_calc equals the stored
    outer checksum, and l4_checksum(which=0) says OK on every UDP_CSUM output and UNCHECKED on IPv4 outers without it
    (an IPv6 outer with the zero checksum of RFC 6935 is what l4_checksum calls BAD: RFC 8200's rule)."""
    import torch
    items = parsed_sources()
    n = len(items)
    assert n > 100
    b, ch = T.layout(items, "indexed")
    tun = (np.arange(n) % 14).astype(np.uint32)
    dch = {k: dev(v) for k, v in ch.items()}
    e = TUN.encap(dict(slab=dev(b["slab"]), offsets=dev(b["offsets"]), lens=dev(b["lens"])), dch, tunnel=dev(tun),
                  entropy=dev(np.arange(n, dtype=np.uint32) * 40503), ident=77)
    st = h(e.status)
    ok = np.flatnonzero(st == T.E_OK)
    assert len(ok) > 90 and e.n_out == len(ok)
    k = e.n_out
    res = P.parse(e.slab, offsets=e.offsets[:k], lens=e.lens[:k])
    torch.cuda.synchronize()
    nh = h(res["n_hdrs"]).astype(int)
    oc = {c: h(v) for c, v in e.out_chain.items()}
    assert np.array_equal(nh, oc["n_hdrs"][:k])
    m = np.arange(schema.MAX_HDRS)[:, None] < nh[None, :]
    assert np.array_equal(h(res["hdr_type"])[m], oc["hdr_type"][:, :k][m])
    assert np.array_equal(h(res["hdr_off"])[m], oc["hdr_off"][:, :k][m])
    slab, offs = h(e.slab), h(e.offsets)
    o4 = np.array([ENTS[int(tun[i])]["ipver"] == 4 for i in ok])
    ipo = np.array([oc["hdr_off"][[j for j in range(nh[q]) if oc["hdr_type"][j, q] in (T.T_IPV4, T.T_IPV6)][0], q] for q in range(k)])
    stored = np.array([int(slab[int(offs[q]) + int(ipo[q]) + 10]) << 8 | int(slab[int(offs[q]) + int(ipo[q]) + 11]) for q in range(k)])
    assert np.array_equal(h(res["ipv4_csum_calc"])[o4], stored[o4])
    l4 = P.l4_checksum(e.slab, e.out_chain, which=0, offsets=e.offsets[:k], lens=e.lens[:k], n=k)
    ls = h(l4["status"])
    vx = np.array([ENTS[int(tun[i])]["kind"] == T.VXLAN for i in ok])
    cs = np.array([bool(ENTS[int(tun[i])]["flags"] & T.F_CSUM) for i in ok])
    assert cs.sum() > 10 and (ls[vx & cs] == pktgpu.L4_OK).all()
    assert (vx & ~cs & o4).sum() > 5 and (ls[vx & ~cs & o4] == pktgpu.L4_UNCHECKED).all()


def test_decap_of_encap_returns_the_packets(P, TUN):
    """decap(encap(x)) is x exactly for VXLAN and x cut to its IP length for the L3 kinds, chain and all; the matched
    entry is the other end's; the hits of both calls add exactly n."""
    items, tun, ent, _ = T.encap_mix(N_MIX)
    tun = tun % 14
    b, ch = T.layout(items, "indexed")
    dch = {k: dev(v) for k, v in ch.items()}
    e = TUN.encap(dict(slab=dev(b["slab"]), offsets=dev(b["offsets"]), lens=dev(b["lens"])), dch, tunnel=dev(tun),
                  entropy=dev(ent), hits=True)
    assert int(h(e.hits).sum()) == N_MIX
    k = e.n_out
    eb = dict(slab=e.slab, offsets=e.offsets[:k].contiguous(), lens=e.lens[:k].contiguous())
    ech = dict(n_hdrs=e.out_chain["n_hdrs"][:k].contiguous(), hdr_type=e.out_chain["hdr_type"][:, :k].contiguous(),
               hdr_off=e.out_chain["hdr_off"][:, :k].contiguous())
    d = TUN.decap(eb, ech, hits=e.hits.new_zeros(11))
    assert int(h(d.hits).sum()) == k and (h(d.status) == T.D_OK).all() and d.n_out == k > 300
    src = h(e.src_index)[:k]
    slab, offs, lens = h(d.slab), h(d.offsets), h(d.lens)
    oty, oof, onh = h(d.out_chain["hdr_type"]), h(d.out_chain["hdr_off"]), h(d.out_chain["n_hdrs"])
    assert np.array_equal(h(d.tunnel_out), tun[src] + 14)
    for q, i in enumerate(src):
        p, hdrs = items[i]
        if ENTS[int(tun[i])]["kind"] != T.VXLAN:
            j = T.pick_ip(hdrs, 0)
            ip = hdrs[j][1]
            p = p[:ip + (T.be16(p, ip + 2) if hdrs[j][0] == T.T_IPV4 else 40 + T.be16(p, ip + 4))]
        assert slab[int(offs[q]):int(offs[q]) + int(lens[q])].tobytes() == p, (q, i)
        assert [(int(oty[j, q]), int(oof[j, q])) for j in range(int(onh[q]))] == hdrs[:T.MAXH], (q, i)


def test_encap_forward_fragment_reassemble_decap(P, TUN):
    """encap -> Forwarder.run(which_ip=0) -> fragment(mtu=576) -> reassemble -> decap returns the inner packets: the
    fragmenter splits the OUTER datagram, whose lengths encap has set."""
    import torch
    items = [T.pkt(T.udp(100 + 37 * (k % 40), k), v6=bool(k % 3 == 0), vlans=k % 2) for k in range(150)]
    n = len(items)
    b, ch = T.layout(items, "indexed")
    tun = np.where(np.arange(n) % 3 == 0, 0, np.where(np.arange(n) % 3 == 1, 7, 4)).astype(np.uint32)  # IPv4 outers without DF
    e = TUN.encap(dict(slab=dev(b["slab"]), offsets=dev(b["offsets"]), lens=dev(b["lens"])), {k: dev(v) for k, v in ch.items()},
                  tunnel=dev(tun), ident=100)
    assert e.n_out == n
    fwd = P.forwarder([("02:00:00:00:00:01", "02:00:00:00:00:02", 1)])
    r = fwd.run(e.batch(), e.out_chain, nexthop=torch.zeros(n, dtype=torch.uint32, device="cuda"), which_ip=0)
    assert (h(r["status"]) == pktgpu.FWD_OK).all()
    f = P.fragment(e.batch(), e.out_chain, mtu=576)
    assert f.n_out > n and (h(f.status)[:n] <= pktgpu.FRAG_SPLIT).all()
    k = f.n_out
    fb = dict(slab=f.slab, offsets=f.offsets[:k].contiguous(), lens=f.lens[:k].contiguous())
    fch = {c: (v[:k] if v.dim() == 1 else v[:, :k]).contiguous() for c, v in f.out_chain.items()}
    j = P.reassemble(fb, fch)
    assert j.n_out == n
    m = j.n_out
    res = P.parse(j.slab, offsets=j.offsets[:m].contiguous(), lens=j.lens[:m].contiguous())
    d = TUN.decap(dict(slab=j.slab, offsets=j.offsets[:m].contiguous(), lens=j.lens[:m].contiguous()),
                  {c: res[c] for c in ("n_hdrs", "hdr_type", "hdr_off")})
    assert (h(d.status) == T.D_OK).all() and d.n_out == n
    slab, offs, lens = h(d.slab), h(d.offsets), h(d.lens)
    # a VXLAN inner frame comes back whole; under GRE / IPIP the Ether header is the outer packet's too, which the
    # forwarder rewrote: the inner IP packet is what comes back
    tout, oty, oof = h(d.tunnel_out), h(d.out_chain["hdr_type"]), h(d.out_chain["hdr_off"])
    got = []
    for q in range(n):
        p = slab[int(offs[q]):int(offs[q]) + int(lens[q])].tobytes()
        ip = [int(oof[r, q]) for r in range(4) if oty[r, q] in (T.T_IPV4, T.T_IPV6)][0]
        got.append(p if tout[q] == 14 else p[ip:])
    want = [p if tun[i] == 0 else p[hd[1 + i % 2][1]:] for i, (p, hd) in enumerate(items)]
    assert sorted(got) == sorted(want) and set(tout.tolist()) == {14, 18, 21}
    fwd.close()


def test_exact_entry_before_any_remote(P, TUN):
    it = T.pkt(T.udp(40, 2))
    b, ch = T.layout([it] * 130, "indexed")
    tun = np.where(np.arange(130) % 2, 28, 26).astype(np.uint32)
    rc, e, intact = run(P, TUN, "encap", b, ch, tun)
    eb, ech = T.layout(T.out_items(e), "indexed")
    rc, d, intact = run(P, TUN, "decap", eb, ech)
    assert rc == 0 and intact and list(d["tunnel_out"]) == [13 if k % 2 else 12 for k in range(130)]


# ------------------------------------------------------------------ capacity
@pytest.mark.parametrize("op", ["encap", "decap"])
def test_plan_only_capacity_and_async(P, TUN, op):
    """plan_only totals equal a real run's; an out_cap or dst_bytes one too small returns the refusal with both totals and
    nothing is written; every NULL-output combination; _async / _result, and a second async call before _result."""
    if op == "encap":
        b, ch, tun, ent, sel, want = emix("indexed")
        kw = dict(tunnel=tun, entropy=ent, ident=65000, select=sel)
    else:
        b, ch, sel, want = dmix("indexed")
        kw = dict(select=sel)
    rc, plan, intact = run(P, TUN, op, b, ch, flags=T.NO_WRITE, **kw)
    assert rc == 0 and intact
    T.check_all(plan, want, 0, "plan")
    for cap, dl in ((want["n_out"] - 1, want["bytes_out"]), (want["n_out"], want["bytes_out"] - 1)):
        rc, got, intact = run(P, TUN, op, b, ch, cap=cap, dst_len=dl, **kw)
        msg = P._L.pkt_ctx_last_error(P._ctx).decode()
        assert rc == INVALID and msg.startswith(f"pkt_tunnel_{op}_batch") and intact
        assert (got["n_out"], got["bytes_out"]) == (want["n_out"], want["bytes_out"])
        assert (got["dst"] == FILL).all() and (got["out_len"].view(np.uint8) == FILL).all() and (got["oc_n_hdrs"] == FILL).all()
    for skip in (("status",), ("out_index", "hits"), ("src_index", "oc_hdr_type"), ("oc_n_hdrs", "oc_hdr_type", "oc_hdr_off"),
                 ("tunnel_out", "status")):
        rc, got, intact = run(P, TUN, op, b, ch, skip=skip, **kw)
        assert rc == 0 and intact
        verify(got, want, skip)
    for mode in ("async", "async_twice"):
        rc, got, intact = run(P, TUN, op, b, ch, mode=mode, **kw)
        assert rc == 0 and intact
        verify(got, want, mode)


# ------------------------------------------------------------------ refusals
def test_create_refusals_on_the_device(P):
    from test_tunnel_host import CREATE_REFUSALS
    L = P._L
    for change, text in CREATE_REFUSALS:
        ents = [T.entry(T.VXLAN, T.LOC4, T.REM4B, id=2000), T.entry(T.VXLAN, T.LOC4, T.REM4, id=5)]
        change(ents[1])
        rec = T.records(ents)
        hd = ctypes.c_void_p()
        rc = L.pkt_tunnel_create(P._ctx, rec.ctypes.data, 2, ctypes.byref(hd))
        if text is None:
            assert rc == 0 and L.pkt_tunnel_destroy(hd) == 0
        else:
            assert rc == INVALID and L.pkt_ctx_last_error(P._ctx).decode() == "pkt_tunnel_create: " + text
    rec = T.records(ENTS)
    hd = ctypes.c_void_p()
    for args, text in (((None, 3), "null entries"), ((rec.ctypes.data, 0), "count is 0 or above PKT_TUN_MAX_ENTRIES"),
                       ((rec.ctypes.data, 65537), "count is 0 or above PKT_TUN_MAX_ENTRIES")):
        assert L.pkt_tunnel_create(P._ctx, *args, ctypes.byref(hd)) == INVALID
        assert L.pkt_ctx_last_error(P._ctx).decode() == "pkt_tunnel_create: " + text


def test_call_refusals_on_the_device(P, TUN, HT):
    from test_tunnel_host import A_CAP, A_CHAIN, A_DST, A_ENTROPY, A_HITS, A_TUN, A_TUNNEL
    b, ch = T.layout([T.pkt(T.udp(30, k)) for k in range(8)], "indexed")

    def refused(op, text, **kw):
        kw.setdefault("cap", 64)
        kw.setdefault("dst_len", 4096)
        rc, got, intact = run(P, TUN, op, b, ch, **kw)
        msg = P._L.pkt_ctx_last_error(P._ctx).decode()
        assert rc == INVALID and msg == f"pkt_tunnel_{op}_batch: {text}" and intact, (msg, text)

    for op in ("encap", "decap"):
        refused(op, "unknown flag bits", flags=2)
        refused(op, "which_ip is neither below 16 nor PKT_FLOW_LAST", which=16)
        refused(op, "null argument", over={A_CHAIN: None})
        refused(op, "null tunnel table", over={A_TUN: None})
        refused(op, "the tunnel table is a host handle", over={A_TUN: HT.h})
        refused(op, "null dst, out_off or out_len without PKT_TUN_NO_WRITE", skip=("dst",))
    _, mid = guarded(256)
    refused("encap", "a uint32_t array is not 4-byte aligned", over={A_TUNNEL: mid.data_ptr() + 2})
    refused("encap", "a uint32_t array is not 4-byte aligned", over={A_ENTROPY: mid.data_ptr() + 1})
    refused("encap", "dst not 16-byte aligned", over={A_DST: mid.data_ptr() + 8})
    refused("encap", "out_cap is 0 or >= 2^32", over={A_CAP: 0})
    refused("encap", "hits not 8-byte aligned", over={A_HITS: mid.data_ptr() + 4})
    # a device handle is refused by the host twins
    rc, got = T.host_call("encap", HT, b, ch, cap=64, dst_len=4096, over={A_TUN: TUN._t})
    assert rc == INVALID and P._L.pkt_tunnel_last_error(TUN._t).decode() == "pkt_tunnel_encap_host: the tunnel table is a device handle"


# ------------------------------------------------------------------ far offsets
def test_far_offsets(P, TUN):
    """One encap and one decap with the source packets placed past 2^31 and past 2^32 bytes of one allocation
    (far_cases' indexed_shuffled plan: every wave mixes low, middle and far packets, every packet at or above 2^31 has a
    decoy where a truncated or sign-extended offset would land).  The outputs are the model's over the compact batch,
    and the allocation is untouched."""
    import torch

    import far_cases as FC
    plan = "indexed_shuffled"
    n = FC.N[plan]
    src = [T.pkt(T.udp(24 + 11 * (k % 50), k), v6=bool(k & 1), vlans=k % 3) for k in range(40)]
    word = int.from_bytes(bytes([FC.FILL]) * 8, "little", signed=True)
    a = None
    for op in ("encap", "decap"):
        items = FC.cycle(src if op == "encap" else T.tunnelled(src, np.arange(40) % 14, np.arange(40)), plan)
        b, ch = T.layout(items, "indexed")
        tun = (np.arange(n) % 14).astype(np.uint32)
        want = T.expect(op, b, ch, ENTS, tun, ident=3)
        pl = FC.place(plan, b)
        if a is None:
            try:
                a = torch.empty((pl.alloc_len + (1 << 20) + 15) // 16 * 16, dtype=torch.uint8, device="cuda")
            except Exception as ex:
                pytest.skip(f"allocating {pl.alloc_len} bytes failed ({ex})")
        assert pl.alloc_len <= a.numel()
        a.fill_(FC.FILL)
        pos, val, _, _ = pl.index()
        dpos = dev(pos)
        a[dpos] = dev(val)
        far = dict(slab=a[FC.FRONT:FC.FRONT + pl.slab_len], offsets=dev(pl.offsets), lens=dev(pl.lens))
        dch = {k: dev(v) for k, v in ch.items()}
        r = TUN.encap(far, dch, tunnel=dev(tun), ident=3, hits=True) if op == "encap" else TUN.decap(far, dch, hits=True)
        got = {k: h(getattr(r, k)) for k in ("status", "out_index", "hits") + (("tunnel_out",) if op == "decap" else ())}
        got.update(n_out=r.n_out, bytes_out=r.bytes_out, dst=h(r.slab), out_off=h(r.offsets), out_len=h(r.lens),
                   src_index=h(r.src_index), oc_n_hdrs=h(r.out_chain["n_hdrs"]), oc_hdr_type=h(r.out_chain["hdr_type"]).reshape(-1),
                   oc_hdr_off=h(r.out_chain["hdr_off"]).reshape(-1))
        T.check_all(got, want, r.offsets.numel(), (op, plan))
        assert want["n_out"] == n
        assert np.array_equal(h(a[dpos]), val), (op, "a source packet or a decoy was written")
        a[dpos] = FC.FILL
        v = a.view(torch.int64)
        for s in range(0, v.numel(), 1 << 27):
            assert bool((v[s:s + (1 << 27)] == word).all()), (op, "a byte outside the packets changed")
