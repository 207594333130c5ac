"""pkt_match_batch (Parser.match_program / Parser.match): the kernel of pktgpu_match.hip against match_cases'
yardstick (a pure-Python evaluator of the contract) and the host twin.  Every slab lies between two guard regions
filled with 0xA5 (a kernel that took field bytes from past slab_len would compare against 0xA5) and so does
every output array, the counters included."""
import ctypes
import itertools

import numpy as np
import pytest

from pktgpu import gen, schema

import compare_cases as C
import edit_cases as E
import l4_cases as L4
import match_cases as M

pytestmark = pytest.mark.gpu
GUARD = 4096
OUT_NAMES = ("rule", "action", "select", "matched", "hits", "bytes")
OUT_DT = (np.uint8, np.uint32, np.uint8, np.uint64, np.uint64, np.uint64)
INVALID = -1


@pytest.fixture(scope="module")
def P():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible")
    import pktgpu
    return pktgpu.Parser(0)


_PROGS = {}


def program(P, prog):
    """The compiled program of a match_cases program dict (kept for the module: create is the only allocation)."""
    if id(prog) not in _PROGS:
        _PROGS[id(prog)] = (P.match_program(M.to_ctypes(prog), prog["default"]), prog)
    return _PROGS[id(prog)][0]


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


def dev_chain(ch):
    return {k: dev(v) for k, v in ch.items()}


def run_guarded(P, mp, kw, chain, outputs=(True,) * 6, stream=None, counters=None):
    """pkt_match_batch with every output between guards -> (rc, {name: numpy}, guards intact).  counters: the
    (hits, bytes) guarded pairs of an earlier call, to be added to."""
    import torch
    n, nr = kw["n"], mp.nrules
    b = P._batch(kw["slab"], n, kw["stride"], kw["offsets"], kw["lens"])
    ch = P._chain(chain)
    bufs = []
    for k, (name, dt, w) in enumerate(zip(OUT_NAMES, OUT_DT, outputs)):
        if not w:
            bufs.append(None)
        elif k >= 4 and counters is not None:
            bufs.append(counters[k - 4])
        else:
            g = guarded((nr + 1 if k >= 4 else n) * np.dtype(dt).itemsize)
            if k >= 4:
                g[1].zero_()
            bufs.append(g)
    ptrs = [None if g is None or not g[1].numel() else g[1].data_ptr() for g in bufs]
    rc = P._L.pkt_match_batch(mp._m, ctypes.byref(b), ctypes.byref(ch), *ptrs, P._stream(stream))
    torch.cuda.synchronize()
    got = {name: None if g is None else g[1].cpu().numpy().view(dt) for name, dt, g in zip(OUT_NAMES, OUT_DT, bufs)}
    return rc, got, all(guards_intact(*g) for g in bufs if g is not None), bufs


def host_twin(b, ch, prog):
    import pktgpu
    return pktgpu.match(b["slab"], ch, M.to_ctypes(prog), prog["default"], stride=b["stride"], n=b["n"], offsets=b["offsets"],
                        lens=b["lens"], hits=True, bytes=True)


def check_on_device(P, b, ch, prog, want, label, twin=False, early=False):
    kw, big = dev_batch(b)
    chain = dev_chain(ch)
    mp = program(P, prog)
    rc, got, intact, _ = run_guarded(P, mp, kw, chain)
    assert rc == 0 and intact, label
    M.check(got, want, label)
    if twin:
        M.check(got, host_twin(b, ch, prog), label + " (host twin)")
    if early:  # matched == NULL: the wave may stop early; the same rule, action, select and counters
        rc, got, intact, _ = run_guarded(P, mp, kw, chain, outputs=(True, True, True, False, True, True))
        assert rc == 0 and intact, label
        M.check(got, want, label + " (no matched)")
    assert guards_intact(big, kw["slab"]) and np.array_equal(kw["slab"].cpu().numpy(), b["slab"]), label


@pytest.mark.parametrize("name", M.CASE_NAMES)
def test_cases(P, name):
    b, ch, prog, want = M.all_cases()[name]
    check_on_device(P, b, ch, prog, want, name, twin=True, early=True)
    if b["n"] == 0:
        return
    for kind in ("stride64", "stride128"):  # 64: the four-chunk window
        rb, rw = M.relaid_want(name, kind)
        check_on_device(P, rb, ch, prog, rw, f"{name} {kind}", early=kind == "stride64")


@pytest.mark.parametrize("name", ["mix_edges", "mix_deep", "mix_acl", "mix_terms256", "mix_refs30", "odd_chains", "ref22_edges",
                                  "random_03"])
def test_every_alignment(P, name):
    b, ch, prog, want = M.all_cases()[name]
    for shift in range(16):
        check_on_device(P, M.relaid(b, "indexed", shift), ch, prog, want, f"{name} + {shift}")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_wave_and_block_edges(P, n):
    """The first n packets of the random mix, the slab ending exactly with the last of them."""
    for name in ("random_acl", "random_07"):
        b, ch, prog, want = M.all_cases()[name]
        hb, hch, hw = M.head(b, ch, want, n)
        assert hb["slab"].size == int(hb["offsets"][-1]) + int(hb["lens"][-1])  # (offsets ascend)
        check_on_device(P, hb, hch, prog, hw, f"{name} first {n}", early=True)
        rb, rw = M.relaid_want(name, "stride64")
        sb = M.batch(rb["slab"][:64 * n], None, rb["lens"][:n], stride=64, n=n)
        sw = dict(M.head(M.batch(rb["slab"], [64 * i for i in range(rb["n"])], rb["lens"]), ch, rw, n, cut=False)[2])
        check_on_device(P, sb, hch, prog, sw, f"{name} stride 64 first {n}")


def tiled(b, ch, reps, extra):
    """The batch's packets reps times over and `extra` more: n = reps * b.n + extra, which the tests choose above
    1280 blocks of 256 packets and off a multiple of 256."""
    n0 = b["n"]
    n = reps * n0 + extra
    idx = np.arange(n) % n0
    if b["offsets"] is None:
        st = b["stride"]
        slab = np.tile(b["slab"][:st * n0], reps + 1)[:st * n]
        tb = M.batch(slab, None, b["lens"][idx], stride=st, n=n)
    else:
        size = (b["slab"].size + 15) // 16 * 16
        one = np.zeros(size, np.uint8)
        one[:b["slab"].size] = b["slab"]
        slab = np.tile(one, reps + 1)
        tb = M.batch(slab, b["offsets"][idx] + (np.arange(n) // n0).astype(np.uint64) * np.uint64(size), b["lens"][idx])
    tch = dict(n_hdrs=ch["n_hdrs"][idx].copy(), hdr_type=np.ascontiguousarray(ch["hdr_type"][:, idx]),
               hdr_off=np.ascontiguousarray(ch["hdr_off"][:, idx]))
    return tb, tch, idx


LARGE_PROGRAMS = {
    "one_term": M.nested([(3, [M.term("UDP", 0, "dst", M.EQ, 53)])], default=0),
    "five_rules_15_terms": M.nested([
        (1, [M.term("IPv4", 0, "src", M.EQ, M.ip4(M.SRC[0]), 0xFFFFFF00), M.term("IPv4", 0, "protocol", M.EQ, 6), M.has("TCP")]),
        (0, [M.term("UDP", 0, "dst", M.RANGE, 50, 100), M.term("IPv4", 0, "dst", M.EQ, M.ip4(M.DST[2]), 0xFFFFFF00), M.length(0, 80)]),
        (2, [M.has("Vlan", 1), M.term("Vlan", 1, "vid", M.EQ, 11), M.has("IPv6", 0, True)]),
        (4, [M.term("IPv6", 0, "next_hdr", M.EQ, 17), M.term("UDP", 0, "src", M.RANGE, 1000, 1100), M.has("Vlan", 0, True)]),
        (5, [M.has("TCP", 0, True), M.has("UDP", 0, True), M.length(60, 65535)])], default=6),
    "acl_80_terms": M.acl(),
}


@pytest.mark.parametrize("layout", ["stride64", "indexed"])
def test_large_batches_both_grids(P, layout):
    """400 137 packets (the random mix 200 times over and 137 more: above 1280 blocks of 256, no multiple of 256):
    a counting launch of a program of at most 16 compiled terms caps its grid and its blocks loop over tiles, one
    of more terms takes one tile a block.  All six outputs against the yardstick's per-packet results repeated
    (the counters recounted from them) and against the host twin over the whole batch; then without counters
    (one tile a block for every program), and with the counters alone."""
    b0, ch0, _, _ = M.all_cases()["random_acl"]
    if layout == "stride64":
        b0 = M.relaid(b0, "stride64")
    tb, tch, idx = tiled(b0, ch0, 200, 137)
    n = tb["n"]
    assert n == 400137 and n > 1280 * 256 and n % 256
    kw, big = dev_batch(tb)
    chain = dev_chain(tch)
    ev = M.Evaluator(b0, ch0)
    lens = np.array([ln for _, ln in M.extents(b0)], np.int64)[idx]
    for name, prog in LARGE_PROGRAMS.items():
        assert (len(prog["terms"]) <= 16) == (name != "acl_80_terms")
        w0 = ev.run(prog)
        nr = len(prog["rules"])
        want = {k: w0[k][idx] for k in ("rule", "action", "select", "matched")}
        slot = np.where(want["rule"] == M.NONE, nr, want["rule"]).astype(np.int64)
        want["hits"] = np.bincount(slot, minlength=nr + 1).astype(np.uint64)
        want["bytes"] = np.bincount(slot, weights=lens, minlength=nr + 1).astype(np.uint64)
        assert int(want["hits"].sum()) == n and (want["hits"] > 0).sum() >= 2, name
        mp = program(P, prog)
        for outs in ((True,) * 6, (True, True, True, True, False, False), (False, False, False, False, True, True),
                     (False, False, True, False, True, False)):
            rc, got, intact, _ = run_guarded(P, mp, kw, chain, outputs=outs)
            assert rc == 0 and intact, (name, outs)
            M.check(got, want, f"{name} {layout} {outs}")
        M.check(host_twin(tb, tch, prog), want, f"{name} {layout} (host twin)")
    assert guards_intact(big, kw["slab"])


def test_null_output_combinations(P):
    b, ch, prog, want = M.all_cases()["mix_acl"]
    kw, big = dev_batch(b)
    chain = dev_chain(ch)
    mp = program(P, prog)
    for outs in itertools.product((True, False), repeat=6):
        rc, got, intact, _ = run_guarded(P, mp, kw, chain, outputs=outs)
        assert rc == 0 and intact, outs
        M.check(got, want, str(outs))
    assert guards_intact(big, kw["slab"])


def many_udp(n=1000):
    rng = np.random.default_rng(7)
    pk = [L4.pkt("UDP", sport=1000 + int(rng.integers(0, 70)), payload=L4.rnd(rng, int(rng.integers(0, 9)))) for _ in range(n)]
    b = C.indexed(pk, rng)
    return b, L4.chain_of(b)


def test_counters(P):
    import torch
    b, ch = many_udp()
    ev = M.Evaluator(b, ch)
    kw, big = dev_batch(b)
    chain = dev_chain(ch)
    # all 1000 packets on one rule: one add per block and counter
    one = M.nested([(0, [M.has("ARP")]), (5, [M.has("UDP")])])
    rc, got, intact, _ = run_guarded(P, program(P, one), kw, chain)
    assert rc == 0 and intact and got["hits"].tolist() == [0, 1000, 0]
    assert got["bytes"].tolist() == [0, sum(ln for _, ln in M.extents(b)), 0]
    # spread over 64 rules (and "none"): the yardstick's histogram
    spread = M.nested([(r + 1, [M.term("UDP", 0, "src", M.EQ, 1000 + r)]) for r in range(64)])
    want = ev.run(spread)
    assert (want["hits"] > 0).all()
    rc, got, intact, _ = run_guarded(P, program(P, spread), kw, chain)
    assert rc == 0 and intact
    M.check(got, want, "spread")
    # two calls on two streams into the same counters: the exact sums
    mp = program(P, spread)
    hits, byt = guarded(65 * 8), guarded(65 * 8)
    hits[1].zero_()
    byt[1].zero_()
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    bb, cc = P._batch(kw["slab"], kw["n"], kw["stride"], kw["offsets"], kw["lens"]), P._chain(chain)
    for s in (s1, s2, s1, s2):
        assert P._L.pkt_match_batch(mp._m, ctypes.byref(bb), ctypes.byref(cc), None, None, None, None, hits[1].data_ptr(),
                                    byt[1].data_ptr(), P._stream(s)) == 0
    torch.cuda.synchronize()
    assert np.array_equal(hits[1].cpu().numpy().view(np.uint64), 4 * want["hits"])
    assert np.array_equal(byt[1].cpu().numpy().view(np.uint64), 4 * want["bytes"])
    assert guards_intact(*hits) and guards_intact(*byt)
    # Parser.match: hits=True allocates, a tensor passed in is accumulated into
    res = P.match(kw["slab"], chain, mp, offsets=kw["offsets"], lens=kw["lens"], hits=True, bytes=True)
    res2 = P.match(kw["slab"], chain, mp, offsets=kw["offsets"], lens=kw["lens"], outputs=("select",), hits=res["hits"])
    torch.cuda.synchronize()
    assert res2["hits"] is res["hits"] and set(res2) == {"select", "hits"}
    M.check({k: v.cpu().numpy() for k, v in res.items() if k != "hits"}, want, "Parser.match")
    assert np.array_equal(res["hits"].cpu().numpy(), 2 * want["hits"])


def test_refusals(P):
    import torch
    b, ch, prog, want = M.all_cases()["mix_acl"]
    kw, big = dev_batch(b)
    chain = dev_chain(ch)
    mp = program(P, prog)
    L, s, lib = P._L, P._stream(None), P._lib
    n = kw["n"]
    outs = [torch.full((n * sz,), 0x77, dtype=torch.uint8, device="cuda") for sz in (1, 4, 1, 8)]
    cnt = [torch.full((17 * 8,), 0x77, dtype=torch.uint8, device="cuda") for _ in range(2)]
    good, gch = P._batch(kw["slab"], n, None, kw["offsets"], kw["lens"]), P._chain(chain)
    base = [mp._m, ctypes.byref(good), ctypes.byref(gch)] + [t.data_ptr() for t in outs + cnt]

    def call(r=()):
        a = list(base)
        for k, v in dict(r).items():
            a[k] = v
        return L.pkt_match_batch(*a, s)
    huge = P._batch(kw["slab"], 1 << 32, 64, None, None)
    no_col = lib.PktChain(gch.n_hdrs, None, gch.hdr_off)
    forms = {"offsets without lens": lib.PktBatch(good.slab, good.slab_len, good.offsets, None, 0, 0, 4),
             "stride 0": lib.PktBatch(good.slab, good.slab_len, None, None, 0, 0, 4),
             "slab not 16-byte aligned": lib.PktBatch(good.slab + 1, good.slab_len - 1, None, None, 64, 0, 4),
             "null slab": lib.PktBatch(None, good.slab_len, None, None, 64, 0, 4)}
    bad = [{0: None}, {1: None}, {2: None}, {2: ctypes.byref(no_col)}, {1: ctypes.byref(huge)},
           {6: outs[3].data_ptr() + 4}, {7: cnt[0].data_ptr() + 4}, {8: cnt[1].data_ptr() + 1}]
    for r in bad:
        assert call(r) == INVALID, sorted(r)
    for text, fb in forms.items():  # the strict batch rules, with their texts
        assert call({1: ctypes.byref(fb)}) == INVALID, text
        assert L.pkt_ctx_last_error(P._ctx) == text.encode(), text
    empty = P._batch(kw["slab"], 0, 64, None, None)
    assert call({1: ctypes.byref(empty)}) == 0
    assert call({k: None for k in range(3, 9)}) == 0  # every output NULL: nothing launched
    torch.cuda.synchronize()
    assert all(bool((t == 0x77).all()) for t in outs + cnt)  # every refusal (and n == 0) came before any launch
    # create: every refusal of the host twin's list, with a text
    import test_match_host as H
    for label, terms, nt, rules, nr in H.bad_programs():
        h = ctypes.c_void_p()
        assert L.pkt_match_create(P._ctx, terms, nt, rules, nr, 0, ctypes.byref(h)) == INVALID and not h.value, label
        assert L.pkt_ctx_last_error(P._ctx).startswith(b"pkt_match"), label
    for label, terms, nt, rules, nr in H.good_edge_programs():
        h = ctypes.c_void_p()
        assert L.pkt_match_create(P._ctx, terms, nt, rules, nr, 0, ctypes.byref(h)) == 0 and h.value, label
        assert L.pkt_match_destroy(h) == 0
    h = ctypes.c_void_p()
    assert L.pkt_match_create(None, None, 0, None, 0, 0, ctypes.byref(h)) == INVALID
    assert L.pkt_match_create(P._ctx, None, 0, None, 0, 0, None) == INVALID
    assert L.pkt_match_destroy(None) == INVALID
    with pytest.raises(RuntimeError):
        P.match_program([(1, [("IPv4", 0, (0, 64), "==", 1)])])
    mp2 = P.match_program([(1, [("UDP", 0, "dst", "==", 53)])], default=0)
    assert (mp2.nrules, mp2.nterms) == (1, 1)
    mp2.close()
    mp2.close()


def test_edits_out_chain(P):
    """A VXLAN encap by pkt_edit_batch, then rules on the outer and inner headers over the edited bytes with edit's
    out_chain: the yardstick's over the edited bytes with a parse of them by the Python model."""
    rng = np.random.default_rng(93)
    n = 70
    inner = [bytes(gen.test_tcp_packet_with_payload(E.rnd_bytes(rng, int(rng.integers(0, 200)))).to_vec()) for _ in range(n)]
    src, _ = dev_batch(C.indexed(inner, rng))
    parsed = P.parse(src["slab"], offsets=src["offsets"], lens=src["lens"], columns=["chain"])
    dst, ln, st, ch = P.edit(src["slab"], parsed, E.encap_ops(), offsets=src["offsets"], lens=src["lens"], slot=512)
    assert (st.cpu().numpy() == E.OK).all()
    prog = M.nested([(1, [M.has("Vxlan"), M.term("TCP", 0, "dst", M.RANGE, 0, 65535), M.length(150, 65535)]),
                     (2, [M.term("IPv4", 1, "ttl", M.RANGE, 1, 255), M.term("Ether", 1, "etype", M.EQ, 0x0800)]),
                     (3, [M.has("UDP")])])
    got = P.match(dst, ch, program(P, prog), stride=512, n=n, lens=ln, hits=True, bytes=True)
    hb = M.batch(dst.cpu().numpy(), None, ln.cpu().numpy(), stride=512, n=n)
    want = M.Evaluator(hb, L4.chain_of(hb)).run(prog)
    assert len(set(want["rule"].tolist())) == 2
    M.check({k: v.cpu().numpy() for k, v in got.items()}, want, "out_chain")


def test_match_then_pcap_write(P):
    import pktgpu
    b, ch, prog, want = M.all_cases()["random_acl"]
    kw, _ = dev_batch(b)
    sel = P.match(kw["slab"], dev_chain(ch), program(P, prog), offsets=kw["offsets"], lens=kw["lens"], outputs=("select",))["select"]
    cap, n, offs, lens, src = P.pcap_write(kw["slab"], offsets=kw["offsets"], lens=kw["lens"], select=sel)
    keep = np.flatnonzero(want["select"])
    assert 0 < keep.size < b["n"] and n == keep.size and np.array_equal(src.cpu().numpy(), keep)
    buf = cap.cpu().numpy()
    ho, hl = pktgpu.pcap_index(buf)
    pk = C.packets(b)
    assert [buf[int(o):int(o) + int(x)].tobytes() for o, x in zip(ho, hl)] == [pk[i] for i in keep]


def test_stream_windows_carry_the_counters(P):
    """push (random sizes) -> poll -> match on st.batch() with the stream's columns -> release, in windows of `cap`
    records over ref22.pcap: the counters carried across the releases equal one host match over the whole file."""
    import torch
    from pktgpu.stream import PcapStream
    rng = np.random.default_rng(13)
    b, ch, prog, want = M.all_cases()["ref22_first_match_order"]
    raw = b["slab"].tobytes()
    mp = program(P, prog)
    cap = 8
    hits = torch.zeros(mp.nrules + 1, dtype=torch.uint64, device="cuda")
    byt = torch.zeros_like(hits)
    st = PcapStream(0, max_bytes=1 << 20, cap=cap, columns=["chain"])
    try:
        at = 0
        while at < len(raw):
            k = int(rng.integers(1, 700))
            st.push(raw[at:at + k])
            at += k
        seen, rules = 0, []
        while True:
            n, _ = st.poll()
            last = n <= cap
            if last:
                n, _ = st.finish()
            slab, offs, lens = st.batch()
            k = offs.numel()
            chain = st.out if k == cap else {c: st.out[c][..., :k].contiguous() for c in ("n_hdrs", "hdr_type", "hdr_off")}
            res = P.match(slab, chain, mp, offsets=offs, lens=lens, outputs=("rule",), hits=hits, bytes=byt)
            rules += res["rule"].cpu().tolist()
            seen += k
            if last:
                break
            torch.cuda.synchronize()  # the window's readers are done before the stream moves it
            st.release(cap)
        assert seen == 22 and rules == want["rule"].tolist()
        twin = host_twin(b, ch, prog)
        assert np.array_equal(hits.cpu().numpy(), twin["hits"]) and np.array_equal(byt.cpu().numpy(), twin["bytes"])
        assert np.array_equal(twin["hits"], want["hits"])
    finally:
        st.close()
