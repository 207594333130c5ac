"""pkt_icmp_err_batch / _async / _result (Parser.icmp_errors): the kernels of pktgpu_icmp.hip against icmp_cases'
yardstick (an independent Python model) and the host twin pkt_icmp_err_host.  The decision and the header builders
are covered on the CPU (test_icmp_err_host.py: the host twin runs the same inline code); here it is the loads, the
scan, the chunk walk with its three sources and the quote's sum.  dst and every output array lie between two guard
regions filled with 0xA5, the outputs start as 0x77, and dst at and past the total must still be 0x77 after the call."""
import ctypes
import socket

import numpy as np
import pytest

import pktgpu
from pktgpu import schema

import icmp_cases as I

pytestmark = pytest.mark.gpu
GUARD = 4096
FILL = 0x77
INVALID = -1
N_MIX = 3 * 256 + 131  # three tiles of the decision kernel and a ragged one
CF = I.cfg(ident=65500, ttl=77, tos=0x20)


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


def dev_batch(P, b, ch):
    slab = dev(b["slab"])
    offs = None if b["offsets"] is None else dev(b["offsets"])
    lens = None if b["lens"] is None else dev(b["lens"])
    dch = {k: dev(v) for k, v in ch.items()}
    return P._batch(slab, b["n"], b["stride"], offs, lens), P._chain(dch), (slab, offs, lens, dch)


def run(P, b, ch, code, cf=CF, mtu=0, cmap=None, select=None, which=0, flags=0, cap=None, dst_len=None, skip=(), mode="sync",
        over=None):
    """pkt_icmp_err_batch over a device copy of the batch -> (rc, got, guards intact).  cap / dst_len default to the
    model-free sizing pass (PKT_ICMPE_NO_WRITE).  hits start as 0x77.. and come back less that."""
    import torch
    L = P._L
    pb, pc, keep = dev_batch(P, b, ch)
    n = b["n"]
    cd = None if np.isscalar(code) else dev(np.asarray(code, np.uint8))
    mt = None if np.isscalar(mtu) else dev(np.asarray(mtu, np.uint16))
    mp = None if cmap is None else np.ascontiguousarray(cmap, np.uint8)
    sel = None if select is None else dev(np.asarray(select, np.uint8))
    cc = I.lib_cfg(cf)
    tp = lambda t: t.data_ptr() if t is not None and t.numel() else None  # noqa: E731
    tot, cnt = ctypes.c_uint64(0), ctypes.c_uint64(0)
    head = [P._ctx, ctypes.byref(pb), ctypes.byref(pc), which, flags, ctypes.byref(cc), tp(cd), 0 if cd is not None else int(code),
            None if mp is None else mp.ctypes.data, tp(mt), 0 if mt is not None else int(mtu), tp(sel)]
    if cap is None or dst_len is None:
        sizing = list(head)
        sizing[4] = flags | I.NO_WRITE
        rc = L.pkt_icmp_err_batch(*sizing, None, None, None, 0, 0, None, None, None, None, None, ctypes.byref(tot),
                                  ctypes.byref(cnt), P._stream(None))
        assert rc == 0
        cap = max(1, cnt.value) if cap is None else cap
        dst_len = tot.value if dst_len is None else dst_len
    counts = dict(status=n, out_index=n, out_off=cap, out_len=cap, src_index=cap, oc_n_hdrs=cap, oc_hdr_type=I.MAXH * cap,
                  oc_hdr_off=I.MAXH * cap, hits=I.NSTATUS)
    if flags & I.NO_WRITE:
        skip = set(skip) | I.PER_OUTPUT
    bufs = {k: guarded(counts[k] * np.dtype(dt).itemsize, FILL) for k, dt in I.SHAPES.items() if k not in skip}
    if "dst" not in skip:
        bufs["dst"] = guarded(dst_len + 64, FILL)  # 64 more bytes the call is not told of
    p = lambda k: bufs[k][1].data_ptr() if k in bufs and bufs[k][1].numel() else None  # noqa: E731
    oc = P._lib.PktChain(p("oc_n_hdrs"), p("oc_hdr_type"), p("oc_hdr_off"))
    args = head + [p("status"), p("out_index"), p("dst"), dst_len, cap, p("out_off"), p("out_len"), p("src_index"),
                   ctypes.byref(oc), p("hits")]
    for k, v in dict(over or {}).items():
        args[k + 1] = v  # icmp_cases' positions are pkt_icmp_err_host's: the ctx comes first here
    if mode == "sync":
        rc = L.pkt_icmp_err_batch(*args, ctypes.byref(tot), ctypes.byref(cnt), P._stream(None))
    else:
        rc = L.pkt_icmp_err_batch_async(*args, P._stream(None))
        if rc == 0:
            if mode == "async_twice":  # the one-in-flight rule
                rc2 = L.pkt_icmp_err_batch_async(*args, P._stream(None))
                msg = P._L.pkt_ctx_last_error(P._ctx).decode()
                assert rc2 == INVALID and msg.startswith("pkt_icmp_err") and "pkt_icmp_err_result" in msg
            rc = L.pkt_icmp_err_result(P._ctx, ctypes.byref(tot), ctypes.byref(cnt))
    torch.cuda.synchronize()
    got = {k: g[1].cpu().numpy().view(I.SHAPES.get(k, np.uint8)) for k, g in bufs.items()}
    if "hits" in got:
        got["hits"] = got["hits"] - np.uint64(0x7777777777777777)
    got["n_out"], got["bytes_out"], got["cap"] = cnt.value, tot.value, cap
    intact = all(guards_intact(*g) for g in bufs.values())
    return rc, got, intact


def verify(got, want, label):
    I.check(got, want, got["cap"], label)
    assert (got["dst"][want["bytes_out"]:] == FILL).all(), (label, "dst written at or past the total")


def same_as_twin(got, b, ch, code, cf, mtu, cmap, select, which, label):
    rc, h = I.host_call(b, ch, code, cf, mtu, cmap, select, which)
    assert rc == 0
    k, nb = h["n_out"], h["bytes_out"]
    assert (got["n_out"], got["bytes_out"]) == (k, nb), label
    assert np.array_equal(got["dst"][:nb], h["dst"][:nb]), (label, "dst")
    for name in I.SHAPES:
        if name in got and name in h and not name.startswith("oc_hdr"):
            assert np.array_equal(got[name], h[name]), (label, name)


def outputs(got):
    return [got["dst"][int(o):int(o) + int(ln)].tobytes() for o, ln in zip(got["out_off"][:got["n_out"]], got["out_len"])]


def mix(kind, which, nosrc=False):
    def build():
        items, code, mtu, sel = I.mix(N_MIX)
        b, ch = I.layout(items, kind)
        cf = I.cfg(src6=None) if nosrc else I.cfg(ident=65000)
        return b, ch, code, mtu, sel, cf, I.expect(b, ch, code, cf, mtu, I.MAP, sel, which)
    return I.cached(("mix", kind, which, nosrc), build)


# ------------------------------------------------------------------ the mix, both layouts
@pytest.mark.parametrize("kind,which,nosrc", [("indexed", 0, False), ("stride", I.LAST, False), ("indexed", I.LAST, True)])
def test_mix_against_the_model_and_the_host_twin(P, kind, which, nosrc):
    """60..1600-byte packets and a few of 9000, IPv4 and IPv6, 0 / 1 / 2 VLAN tags, VXLAN with which_ip 0 and LAST,
    per-packet codes through ICMP_MAP_FWD (plus one forged row), per-packet mtus, a select mask; source packets at
    every alignment 0..15, more than three tiles of the decision kernel.  The third run has no IPv6 source address:
    NO_SRC is a status of a whole IP version, so no single cfg reaches all twelve."""
    b, ch, code, mtu, sel, cf, want = mix(kind, which, nosrc)
    I.mix_conditions(mix(kind if not nosrc else "indexed", which if not nosrc else 0)[-1], mix("indexed", I.LAST, True)[-1])
    if kind == "indexed":
        assert {int(o) % 16 for o in b["offsets"][:16]} == set(range(16)) and int(b["offsets"][-1]) + int(b["lens"][-1]) == b["slab"].size
    rc, got, intact = run(P, b, ch, code, cf, mtu, I.MAP, sel, which)
    assert rc == 0 and intact
    verify(got, want, kind)
    same_as_twin(got, b, ch, code, cf, mtu, I.MAP, sel, which, kind)
    assert int(got["hits"].sum()) == b["n"]


def test_1282_tiles_a_counting_block_takes_two(P):
    """1280 * 256 + 257 packets: with hits the decision launch is capped at 1280 blocks, so two of them take a second
    tile, the last one ragged.  52-byte Ether / IPv4 / UDP packets at stride 64, one reason for all of them, every 61st
    selected.  Against the host twin alone: the Python model is too slow at this size, and test_icmp_err_host.py holds
    the twin to it."""
    n = 1280 * 256 + 257
    b, ch = I.G.tiled([I.pkt(I.udp(18, seed=k)) for k in range(4)], n)
    sel = (np.arange(n) % 61 == 0).astype(np.uint8)
    rc, got, intact = run(P, b, ch, I.R_TIME_EXCEEDED, CF, 0, None, sel)
    assert rc == 0 and intact
    same_as_twin(got, b, ch, I.R_TIME_EXCEEDED, CF, 0, None, sel, 0, "1282 tiles")
    assert got["n_out"] == -(-n // 61) and got["hits"][I.SENT] == got["n_out"] and got["hits"][I.SKIPPED] == n - got["n_out"]
    assert (got["dst"][got["bytes_out"]:] == FILL).all()


def test_two_runs_give_identical_bytes_and_arrays(P):
    b, ch, code, mtu, sel, cf, want = mix("stride", I.LAST)
    r1, g1, i1 = run(P, b, ch, code, cf, mtu, I.MAP, sel, I.LAST)
    r2, g2, i2 = run(P, b, ch, code, cf, mtu, I.MAP, sel, I.LAST)
    assert r1 == r2 == 0 and i1 and i2
    for k in g1:
        assert np.array_equal(g1[k], g2[k]), k


# ------------------------------------------------------------------ the quote's edges, several in one wave
@pytest.mark.parametrize("v6", [False, True])
def test_quote_edges(P, v6):
    H, mx = (40, 1280) if v6 else (20, 576)
    room = mx - H - 8
    items = [I.pkt(I.udp(room - H + d, d + 5), v6=v6, vlans=d % 3) for d in (-1, 0, 1)]  # Q one less, exact, clipped
    items += [I.pkt(I.udp(50, 9), v6=v6, pad=13),             # L below len - ip_off: the padding is not quoted
              I.pkt(I.udp(300, 10), v6=v6, trunc=100),        # L above it: quoted as far as the record goes
              I.pkt(I.udp(128 - 14 - H - 8 - H, 1), v6=v6),   # out_len a multiple of 16
              I.pkt(I.udp(129 - 14 - H - 8 - H, 2), v6=v6)]   # ... and one over
    items += [I.pkt(I.udp(8 + k, k), v6=v6, vlans=k % 3) for k in range(40)]  # every length mod 16, all in one wave
    b, ch = I.layout(items)
    want = I.expect(b, ch, 2, CF, 1000)
    assert (want["status"] == I.SENT).all()
    rc, got, intact = run(P, b, ch, 2, CF, 1000)
    assert rc == 0 and intact
    verify(got, want, "edges")
    q = [len(o) - 14 - 4 * vl - H - 8 for vl, o in zip((2, 0, 1, 0, 0), outputs(got))]
    assert q == [room - 1, room, room, H + 50, H + 200] and got["out_len"][5] == 128 and got["out_len"][6] == 129


def test_v6_at_q_1232_and_the_largest_datagram_among_small_ones(P):
    """max6's default gives Q = 1232; max4 = 65535 with one 65535-byte packet among 64-byte ones: the wave walks its
    4097 chunks between its neighbours' five, and the quote's LDS sum stays below 2^31."""
    items = [I.pkt(I.udp(2000, 1), v6=True)] + [I.pkt(I.udp(22, k)) for k in range(20)]
    big = bytearray(I.pkt(I.udp(65535 - 20, 3))[0])
    big[42:] = b"\xff" * (len(big) - 42)  # the largest sum a quote can have
    items.insert(9, (bytes(big), [(I.T_ETHER, 0), (I.T_IPV4, 14), (I.T_UDP, 34)]))
    b, ch = I.layout(items)
    cf = I.cfg(max4=65535)
    want = I.expect(b, ch, 1, cf)
    assert len(want["pkts"][0]) == 14 + 1280 and len(want["pkts"][9]) == 14 + 65535 and want["n_out"] == 22
    rc, got, intact = run(P, b, ch, 1, cf)
    assert rc == 0 and intact
    verify(got, want, "largest")


def test_parity_of_the_prefix_and_of_the_source(P):
    """Forged chains with an odd eth_off (Ether at 1, IP at 15) and an odd P (Ether at 0, IP at 15), at every source
    alignment: the checksums are right by the model, and pkt_l4_checksum_batch says OK."""
    items = []
    for k in range(34):
        p, _ = I.pkt(I.udp(40 + 7 * k, k), v6=k % 2 == 1)
        t = I.T_IPV6 if k % 2 else I.T_IPV4
        items.append((b"\x00" + p, [(I.T_ETHER, 1), (t, 15)]))
        items.append((p[:14] + b"\x99" + p[14:], [(I.T_ETHER, 0), (t, 15)]))
    b, ch = I.layout(items)
    want = I.expect(b, ch, 3, CF)
    assert (want["status"] == I.SENT).all()
    rc, got, intact = run(P, b, ch, 3, CF)
    assert rc == 0 and intact
    verify(got, want, "parity")
    k = got["n_out"]
    oc = dict(n_hdrs=dev(got["oc_n_hdrs"]), hdr_type=dev(got["oc_hdr_type"].reshape(I.MAXH, -1)),
              hdr_off=dev(got["oc_hdr_off"].reshape(I.MAXH, -1)))
    r = P.l4_checksum(dev(got["dst"]), oc, which=pktgpu.L4_LAST, offsets=dev(got["out_off"]), lens=dev(got["out_len"]))
    assert (r["status"].cpu().numpy()[:k] == pktgpu.L4_OK).all()


def test_all_answered_and_none(P):
    items = [I.pkt(I.udp(30 + 5 * i, i), v6=i % 3 == 0, vlans=i % 2) for i in range(300)]
    b, ch = I.layout(items)
    want = I.expect(b, ch, 1, CF)
    rc, got, intact = run(P, b, ch, 1, CF)
    assert rc == 0 and intact and got["n_out"] == 300
    verify(got, want, "all")
    want = I.expect(b, ch, 0, CF)
    rc, got, intact = run(P, b, ch, 0, CF, cap=300, dst_len=4096)
    assert rc == 0 and intact and got["n_out"] == 0 and (got["dst"] == FILL).all()
    verify(got, want, "none")
    assert (got["status"] == I.SKIPPED).all() and (got["out_index"] == I.NONE).all()


# ------------------------------------------------------------------ capacities, NO_WRITE, NULL outputs, async, n == 0
def test_capacities_exact_short_and_with_an_empty_tail(P):
    b, ch, code, mtu, sel, cf, want = mix("stride", I.LAST)
    k, nb = want["n_out"], want["bytes_out"]
    rc, got, intact = run(P, b, ch, code, cf, mtu, I.MAP, sel, I.LAST, cap=k, dst_len=nb)
    assert rc == 0 and intact
    verify(got, want, "exact")
    for cap, room in ((k - 1, nb), (k, nb - 16)):
        rc, got, intact = run(P, b, ch, code, cf, mtu, I.MAP, sel, I.LAST, cap=cap, dst_len=room)
        assert rc == INVALID and intact
        assert P._L.pkt_ctx_last_error(P._ctx).decode().startswith("pkt_icmp_err")
        assert (got["n_out"], got["bytes_out"]) == (k, nb)
        for name in ("status", "hits"):
            assert np.array_equal(got[name], want[name]), name
    rc, got, intact = run(P, b, ch, code, cf, mtu, I.MAP, sel, I.LAST, cap=k + 300, dst_len=nb + 8192)
    assert rc == 0 and intact
    verify(got, want, "empty tail")


def test_no_write_and_null_outputs(P):
    b, ch, code, mtu, sel, cf, want = mix("stride", I.LAST)
    rc, got, intact = run(P, b, ch, code, cf, mtu, I.MAP, sel, I.LAST, flags=I.NO_WRITE)
    assert rc == 0 and intact
    I.check(got, want, 0, "no_write")
    for skip in (["status", "out_index", "hits"], ["src_index"], ["oc_n_hdrs", "oc_hdr_type", "oc_hdr_off"],
                 ["src_index", "oc_hdr_off", "out_index"]):
        rc, got, intact = run(P, b, ch, code, cf, mtu, I.MAP, sel, I.LAST, skip=skip)
        assert rc == 0 and intact, skip
        verify(got, want, str(skip))


def test_async_result_and_one_in_flight(P):
    b, ch, code, mtu, sel, cf, want = mix("stride", I.LAST)
    for mode in ("async", "async_twice"):
        rc, got, intact = run(P, b, ch, code, cf, mtu, I.MAP, sel, I.LAST, mode=mode)
        assert rc == 0 and intact
        verify(got, want, mode)
    tot, cnt = ctypes.c_uint64(5), ctypes.c_uint64(5)
    assert P._L.pkt_icmp_err_result(P._ctx, ctypes.byref(tot), ctypes.byref(cnt)) == INVALID
    assert P._L.pkt_ctx_last_error(P._ctx).decode().startswith("pkt_icmp_err_result")
    rc, got, intact = run(P, b, ch, code, cf, mtu, I.MAP, sel, I.LAST, cap=want["n_out"] - 1, dst_len=want["bytes_out"], mode="async")
    assert rc == INVALID and intact and (got["n_out"], got["bytes_out"]) == (want["n_out"], want["bytes_out"])


def test_n_0(P):
    b, ch = I.layout([I.pkt(I.udp(100))])
    b = dict(b, n=0, offsets=b["offsets"][:1], lens=b["lens"][:1])
    rc, got, intact = run(P, b, ch, 1, cap=70, dst_len=64, skip=["status", "out_index"])
    assert rc == 0 and intact and (got["n_out"], got["bytes_out"]) == (0, 0)
    assert (got["out_off"] == 0).all() and (got["out_len"] == 0).all() and (got["src_index"] == I.NONE).all()
    assert (got["oc_n_hdrs"] == 0).all() and (got["dst"] == FILL).all() and (got["hits"] == 0).all()


# ------------------------------------------------------------------ the other calls take the output (no model involved)
def parsed_batch(P, items):
    b, _ = I.layout(items)
    d = dict(slab=dev(b["slab"]), offsets=dev(b["offsets"]), lens=dev(b["lens"]))
    chain = P.parse(d["slab"], offsets=d["offsets"], lens=d["lens"], columns=["chain"])
    return b, d, chain


def test_l4_checksum_parse_flow_keys_and_pcap_write_take_the_output(P):
    import torch
    items = [it for it, k in zip(I.mix(400, seed=9)[0], range(400)) if k not in (7, 8) and k % 41 != 2]
    n = len(items)
    b, d, chain = parsed_batch(P, items)
    code = dev((np.arange(n) % 6 + 1).astype(np.uint8))
    e = P.icmp_errors(d, chain, reason=code, mtu=1300, src4=I.SRC4, src6=I.SRC6, which_ip=I.LAST, hits=True)
    k = e.n_out
    assert k > 150 and int(e.hits.cpu().numpy().astype(np.int64).sum()) == n
    r = P.l4_checksum(e.slab, e.out_chain, which=pktgpu.L4_LAST, offsets=e.offsets, lens=e.lens)
    assert (r["status"].cpu().numpy()[:k] == pktgpu.L4_OK).all()
    g = P.parse(e.slab, offsets=e.offsets[:k], lens=e.lens[:k], columns=["chain", "payload_off", "status"])
    torch.cuda.synchronize()
    nh = e.out_chain["n_hdrs"].cpu().numpy()[:k]
    assert (g["status"].cpu().numpy() == 0).all() and np.array_equal(g["n_hdrs"].cpu().numpy(), nh)
    gt, go = g["hdr_type"].cpu().numpy(), g["hdr_off"].cpu().numpy()
    et, eo = e.out_chain["hdr_type"].cpu().numpy()[:, :k], e.out_chain["hdr_off"].cpu().numpy()[:, :k]
    for j in range(int(nh.max())):
        m = nh > j
        assert np.array_equal(gt[j][m], et[j][m]) and np.array_equal(go[j][m], eo[j][m]), j
    icmp_off = eo[nh - 1, np.arange(k)]
    assert (et[nh - 1, np.arange(k)] == I.T_ICMP).all()
    assert np.array_equal(g["payload_off"].cpu().numpy(), (icmp_off + 4).astype(np.uint16))
    fk = P.flow_keys(e.slab, e.out_chain, which_ip=0, offsets=e.offsets, lens=e.lens)
    keys = fk["keys"].cpu().numpy().view(schema.FLOW_KEY_DTYPE).reshape(-1)[:k]
    v4 = keys["ipver"] == 4
    assert (keys["proto"][v4] == 1).all() and (keys["proto"][~v4] == 58).all() and v4.any() and (~v4).any()
    assert (keys["src"][v4][:, :4] == np.frombuffer(socket.inet_aton(I.SRC4), np.uint8)).all()
    assert (keys["src"][~v4] == np.frombuffer(socket.inet_pton(socket.AF_INET6, I.SRC6), np.uint8)).all()
    src = e.src_index.cpu().numpy()[:k]
    for q in np.flatnonzero(v4)[:50]:
        p = items[src[q]][0]
        assert bytes(keys["dst"][q][:4]) in p  # the original source address
    cap, nrec, ro, rl, rs = P.pcap_write(e.slab, offsets=e.offsets[:k], lens=e.lens[:k])
    assert nrec == k and cap.numel() == 24 + 16 * k + int(e.lens.cpu().numpy()[:k].astype(np.int64).sum())


def test_forward_answer_and_route_the_replies(P):
    """400 packets, some with ttl 1, some above their adjacency's mtu, some without a route: Forwarder.run ->
    icmp_errors(fwd_status=...) -> Forwarder.run over the replies, with an Lpm that routes the original sources."""
    import torch
    rng = np.random.default_rng(4)
    far = socket.inet_aton("203.0.113.9")
    items = []
    for i in range(400):
        v6 = i % 4 == 3
        ln = int(rng.integers(30, 1400))
        items.append(I.pkt(I.udp(ln, i), v6=v6, vlans=i % 2, ttl=1 if i % 5 == 0 else 64, dst=far if i % 7 == 1 and not v6 else None))
    b, d, chain = parsed_batch(P, items)
    adj_mtu = np.asarray([1500, 576, 0], np.uint16)
    adj = [("02:00:00:00:00:01", "02:00:00:00:00:02", 1, 1500), ("02:00:00:00:00:03", "02:00:00:00:00:04", 2, 576),
           ("02:00:00:00:00:05", "02:00:00:00:00:06", 3, 0)]
    lpm = P.lpm([("198.51.100.0/24", 1), ("2001:db8:2::/48", 0), ("10.0.0.0/8", 2), ("2001:db8:1::/48", 2)], default_nexthop=99)
    fwd = P.forwarder(adj)
    r = fwd.run(d, chain, lpm=lpm)
    torch.cuda.synchronize()
    st = r["status"].cpu().numpy()
    ai = r["adj_index"].cpu().numpy()
    for s in (schema.FWD_TTL, schema.FWD_MTU, schema.FWD_NO_ADJ, schema.FWD_OK):
        assert (st == s).sum() >= 10, (s, np.bincount(st))
    mt = np.where(ai < 3, adj_mtu[np.minimum(ai, 2)], 0).astype(np.uint16)
    e = P.icmp_errors(d, chain, fwd_status=r["status"], mtu=dev(mt), src4=I.SRC4, src6=I.SRC6)
    refused = np.isin(st, (schema.FWD_TTL, schema.FWD_MTU, schema.FWD_NO_ADJ))
    hb = dict(b, slab=d["slab"].cpu().numpy())
    ch = {k: v.cpu().numpy() for k, v in chain.items()}
    want = I.expect(hb, ch, st, I.cfg(), mt, schema.ICMP_MAP_FWD)
    assert e.n_out == want["n_out"] == int(refused.sum()) and np.array_equal(e.status.cpu().numpy(), want["status"])
    k = e.n_out
    assert [e.slab.cpu().numpy()[int(o):int(o) + int(ln)].tobytes() for o, ln in
            zip(e.offsets.cpu().numpy()[:k], e.lens.cpu().numpy())] == want["pkts"]
    r2 = fwd.run(e.batch(), e.out_chain, lpm=lpm)
    torch.cuda.synchronize()
    assert (r2["status"].cpu().numpy()[:k] == schema.FWD_OK).all() and (r2["port"].cpu().numpy()[:k] == 3).all()


# ------------------------------------------------------------------ refusals
def test_refusal_texts(P):
    import torch
    b, ch = I.layout([I.pkt(I.udp(1000)), I.pkt(I.udp(100))])
    odd = torch.zeros(64, dtype=torch.uint8, device="cuda")
    base = odd.data_ptr()
    bad = {k: I.lib_cfg(v) for k, v in (("neither", I.cfg(None, None)), ("max4 below 56", I.cfg(max4=55)), ("max6 below 96", I.cfg(max6=95)))}
    cases = {"which_ip": {I.A_WHICH: 16}, "flag": {I.A_FLAGS: 8}, "mtu_all": {I.A_MTU: None, I.A_MTU_ALL: 65536},
             "code_all above 255": {I.A_CODE: None, I.A_CODE_ALL: 256}, "null cfg": {I.A_CFG: None},
             "dst not 16": {I.A_DST: base + 8}, "hits not 8": {I.A_HITS: base + 4}, "out_off not 8": {I.A_OUT_OFF: base + 4},
             "mtu not 2": {I.A_MTU: base + 1}, "null dst": {I.A_DST: None}, "null dst, out_off": {I.A_OUT_OFF: None},
             "out_len": {I.A_OUT_LEN: None}, "out_cap": {I.A_CAP: 0}, "out_cap is 0 or": {I.A_CAP: 1 << 32},
             "null argument": {I.A_CHAIN: None}}
    cases.update({k: {I.A_CFG: ctypes.byref(c)} for k, c in bad.items()})
    for text, over in cases.items():
        rc, got, intact = run(P, b, ch, np.asarray([1, 2], np.uint8), CF, np.asarray([576, 576], np.uint16), cap=8, dst_len=4096, over=over)
        msg = P._L.pkt_ctx_last_error(P._ctx).decode()
        assert rc == INVALID and intact and msg.startswith("pkt_icmp_err_batch: ") and text in msg, (text, msg)
        assert (got["status"] == FILL).all() and (got["dst"] == FILL).all() and (got["hits"] == 0).all(), text
    cc = I.lib_cfg(CF)
    for form, text in (("n", "n >= 2^32"), ("lens", "offsets without lens"), ("slab", "slab not 16-byte aligned"), ("col", "null chain column")):
        pb, pc, keep = dev_batch(P, b, ch)
        if form == "n":
            pb.n = 1 << 32
        elif form == "lens":
            pb.lens = None
        elif form == "slab":
            pb.slab = keep[0].data_ptr() + 1
        else:
            pc.hdr_off = None
        tot, cnt = ctypes.c_uint64(7), ctypes.c_uint64(7)
        rc = P._L.pkt_icmp_err_batch(P._ctx, ctypes.byref(pb), ctypes.byref(pc), 0, I.NO_WRITE, ctypes.byref(cc), None, 1, None, None, 0,
                                     None, None, None, None, 0, 0, None, None, None, None, None, ctypes.byref(tot), ctypes.byref(cnt),
                                     P._stream(None))
        msg = P._L.pkt_ctx_last_error(P._ctx).decode()
        assert rc == INVALID and msg.startswith("pkt_icmp_err_batch: ") and text in msg and (tot.value, cnt.value) == (0, 0), (form, msg)
