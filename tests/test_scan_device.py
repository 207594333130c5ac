"""pkt_scan_batch on the device (Parser.scanner): the kernel of pktgpu_scan.hip against scan_cases' yardstick (an
independent Python model that builds no trie).  The case list is the one test_scan_host.py runs, and it runs under
both placements: as it is (small sets: the whole automaton in LDS) and padded with 700 filler patterns that push
the deep levels to device memory.  Every slab and every output lies between two guard regions filled with 0xA5; the
outputs start as 0x77."""
import ctypes

import numpy as np
import pytest

import pktgpu
from pktgpu import gen, schema

import compare_cases as C
import match_cases as M
import scan_cases as S

pytestmark = pytest.mark.gpu
GUARD = 4096
FILL = 0x77
LDS, GLOBAL = schema.SCAN_PLACE_LDS, schema.SCAN_PLACE_GLOBAL


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


def dev_batch(b):
    """The batch on the device, its slab between guards -> (batch dict, the slab's guarded pair)."""
    big, mid = guarded(b["slab"].size)
    if b["slab"].size:
        mid.copy_(dev(b["slab"]))
    return dict(slab=mid, n=b["n"], stride=b["stride"], offsets=None if b["offsets"] is None else dev(b["offsets"]),
                lens=None if b["lens"] is None else dev(b["lens"])), (big, mid)


def run(P, sc, c, skip=(), stream=None, hits=None):
    """pkt_scan_batch over a device copy of the case's batch, every output guarded -> (outputs on the host, hits
    added, everything intact).  `hits`: a device counter array to add to (else a fresh one, unless skipped)."""
    import torch
    kw, slab = dev_batch(c["batch"])
    n = c["batch"]["n"]
    b = P._batch(kw["slab"], kw["n"], kw["stride"], kw["offsets"], kw["lens"])
    cols = None if c["chain"] is None else {k: dev(v) for k, v in c["chain"].items()}   # (kept alive to the end)
    ch = None if cols is None else P._chain(cols)
    sel = None if c["select"] is None else dev(c["select"])
    bufs = {k: guarded(n * np.dtype(dt).itemsize, FILL) for k, dt in S.OUTPUTS if k not in skip}
    if hits is None and "hits" not in skip:
        bufs["hits"] = guarded(8 * (len(c["pats"]) + 1), FILL)
    p = lambda k: bufs[k][1].data_ptr() if k in bufs and bufs[k][1].numel() else None  # noqa: E731
    hp = hits.data_ptr() if hits is not None else p("hits")
    rc = P._L.pkt_scan_batch(sc._t, ctypes.byref(b), None if ch is None else ctypes.byref(ch), schema.SCAN_REGION[c["region"]],
                             None if sel is None or not n else sel.data_ptr(), *[p(k) for k, _ in S.OUTPUTS], hp,
                             P._stream(stream))
    assert rc == 0, P._L.pkt_scan_last_error(sc._t)
    torch.cuda.synchronize()
    dt = dict(S.OUTPUTS, hits=np.uint64)
    got = {k: g[1].cpu().numpy().view(dt[k]) for k, g in bufs.items()}
    if "hits" in got:
        got["hits"] = got["hits"] - np.uint64(0x7777777777777777)
    intact = all(guards_intact(*g) for g in bufs.values()) and guards_intact(*slab) and \
        np.array_equal(slab[1].cpu().numpy(), c["batch"]["slab"])
    return got, intact


_FILLER = None


def padded(c):
    """The case with 700 more patterns of 12 bytes behind its own: the indexes stay, the set no longer fits LDS."""
    global _FILLER
    if _FILLER is None:
        rng = np.random.default_rng(77)
        _FILLER = [S.pat(rng.integers(0x80, 0xC0, 12, dtype=np.uint8).tobytes(), nocase=k % 2, group=40 + k % 8, action=1000 + k)
                   for k in range(700)]
    return dict(c, pats=c["pats"] + _FILLER)


_WANT = {}


def expected(name, place):
    if place == LDS or name == "limits":
        return S.all_cases()[name], S.expected(name)
    if name not in _WANT:
        c = padded(S.all_cases()[name])
        _WANT[name] = (c, S.expect(c))
    return _WANT[name]


@pytest.mark.parametrize("name,place", [(n, p) for n in S.NAMES for p in (LDS, GLOBAL) if (n, p) != ("limits", LDS)],
                         ids=lambda v: v if isinstance(v, str) else ("lds" if v == LDS else "global"))
def test_case_equals_model(P, name, place):
    c, want = expected(name, place)
    sc = pktgpu.Scanner(P, S.tables(c["pats"]), default=c["default"])
    assert sc.info["placement"] == place and sc.info["npatterns"] == len(c["pats"])   # the sets landed where meant
    got, intact = run(P, sc, c)
    S.check(got, want, name)
    assert intact
    assert int(got["hits"][:-1].sum()) == int(got["count"].sum(dtype=np.uint64))
    assert int(got["hits"][-1]) == int((got["status"] == S.MISS).sum())
    hinfo = pktgpu.Scanner(None, S.tables(c["pats"])).info
    assert {k: v for k, v in sc.info.items() if k != "placement"} == {k: v for k, v in hinfo.items() if k != "placement"}
    sc.close()


def test_limits_info(P):
    c = S.all_cases()["limits"]
    sc = pktgpu.Scanner(P, S.tables(c["pats"]))
    i = sc.info
    assert i["npatterns"] == 8192 and i["max_len"] == 16 and i["placement"] == GLOBAL
    assert 100000 < i["nstates"] <= 131074 and i["table_bytes"] < 8 << 20


def test_random_differential(P):
    c = S.random_differential()
    want = S.expect(c)
    share = float((want["status"] == S.HIT).mean())
    assert 0.25 <= share <= 0.75, share                      # not vacuous
    assert float((want["count"] >= 3).mean()) >= 0.01
    for cc, w in ((c, want), (padded(c), None)):
        sc = pktgpu.Scanner(P, S.tables(cc["pats"]), default=cc["default"])
        got, intact = run(P, sc, cc)
        if w is None:                                        # the fillers hold bytes no text has: the same answers
            assert sc.info["placement"] == GLOBAL
            got["hits"] = np.concatenate((got["hits"][:24], got["hits"][-1:]))
        S.check(got, want, "random")
        assert intact


def test_null_outputs_and_two_calls_accumulate(P):
    import torch
    c = S.all_cases()["family"]
    want = S.expected("family")
    sc = pktgpu.Scanner(P, S.tables(c["pats"]))
    hits = torch.full((len(c["pats"]) + 1,), 5, dtype=torch.uint64, device="cuda")
    every = tuple(k for k, _ in S.OUTPUTS)
    for _ in range(2):
        got, intact = run(P, sc, c, skip=every, hits=hits)   # hits alone
        assert intact and got == {}
    assert np.array_equal(hits.cpu().numpy(), 5 + 2 * want["hits"])
    for k in every:                                          # each output alone, no counters
        got, intact = run(P, sc, c, skip=tuple(x for x in every if x != k) + ("hits",))
        assert intact and list(got) == [k]
        S.check(got, want, k)
    got, intact = run(P, sc, c, skip=every + ("hits",))      # nothing asked for: succeeds, launches nothing
    assert intact and got == {}
    r = sc.run(dev_batch(c["batch"])[0], None, "packet", hits=True)   # the Python layer
    S.check({k: getattr(r, k).cpu().numpy() for k in every + ("hits",)}, want, "Scanner.run")
    assert bool(r.hit.any())


def test_two_streams_one_handle(P):
    import torch
    a, b = S.all_cases()["n257_indexed"], S.all_cases()["n65_lens"]
    assert a["pats"] == b["pats"]
    sc = pktgpu.Scanner(P, S.tables(a["pats"]))
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    outs = []
    for c, s in ((a, s1), (b, s2), (a, s2), (b, s1)):
        kw, _ = dev_batch(c["batch"])
        outs.append((kw, sc.run(kw, None, "packet", hits=True, stream=s)))
    torch.cuda.synchronize()
    for (kw, r), name in zip(outs, ("n257_indexed", "n65_lens", "n257_indexed", "n65_lens")):
        S.check({k: getattr(r, k).cpu().numpy() for k in [k for k, _ in S.OUTPUTS] + ["hits"]}, S.expected(name), name)


def test_device_parse_chains(P):
    """The chain columns of the device parse, PAYLOAD region: ref22.pcap and a C4 mix, indexed in place."""
    for name, (buf, offs, lens) in (("ref22", (lambda b: (b["slab"], b["offsets"], b["lens"]))(M.ref22_batch())),
                                    ("c4", gen.gen_c4(700, seed=9))):
        b = C.batch(buf, offs, lens)
        kw, _ = dev_batch(b)
        chain = P.parse(kw["slab"], offsets=kw["offsets"], lens=kw["lens"], columns=["chain", "payload_off"])
        hchain = {k: chain[k].cpu().numpy() for k in ("n_hdrs", "hdr_type", "hdr_off")}
        c = S.case([S.pat("\x00\x00", group=1), S.pat("a"), S.pat("\x08\x00", group=2), S.pat("E", nocase=True, group=3),
                    S.pat("abcd", group=4)], b, "payload", hchain)
        sc = pktgpu.Scanner(P, S.tables(c["pats"]))
        r = sc.run(kw, chain, "payload", hits=True)
        got = {k: getattr(r, k).cpu().numpy() for k in [k for k, _ in S.OUTPUTS] + ["hits"]}
        S.check(got, S.expect(c), name)
        # with the 256 one-byte patterns every byte of the region is one occurrence: r0 is the parse's payload_off
        every = pktgpu.Scanner(P, [bytes([v]) for v in range(256)])
        count = every.run(kw, chain, "payload", want=("count",)).count.cpu().numpy().astype(np.int64)
        ext = np.array([ln for _, ln in C.extents(b)], np.int64)
        scanned = got["status"] <= S.HIT
        assert scanned.sum() >= 0.9 * b["n"]
        assert np.array_equal((ext - count)[scanned], chain["payload_off"].cpu().numpy().astype(np.int64)[scanned]), name


def test_pcap_stream_window_and_result_slabs(P):
    """PcapStream.batch()'s window with the stream's device columns as the chain, and a ReasmResult as the batch."""
    from pktgpu.stream import PcapStream
    rng = np.random.default_rng(3)
    pk = M.random_mix(rng, 300)
    b = C.indexed(pk, rng)
    c = S.case([S.pat("\x00\x00"), S.pat("ab", nocase=True, group=1)], b, "payload", C.chain_of(b))
    want = S.expect(c)
    sc = pktgpu.Scanner(P, S.tables(c["pats"]))
    st = PcapStream(0, max_bytes=1 << 22, cap=len(pk), columns=["chain"])
    try:
        st.push(gen.pcap_bytes(pk))
        n, _ = st.finish()
        assert n == len(pk)
        r = sc.run(st.batch(), st.out, "payload")
        S.check({k: getattr(r, k).cpu().numpy() for k, _ in S.OUTPUTS}, want, "stream window")
    finally:
        st.close()
    kw, _ = dev_batch(b)
    chain = {k: dev(v) for k, v in c["chain"].items()}
    rs = P.reassemble(kw, chain)
    n_out = int(rs.n_out)                                    # the mix's few lone fragments stay PENDING; the rest pass whole
    src = rs.src_index.cpu().numpy()[:n_out]
    assert 250 <= n_out <= len(pk) and not (rs.status.cpu().numpy() == pktgpu.REASM_JOINED).any()
    r = sc.run(rs, None, "packet", want=("count", "status"))
    w = S.expect(dict(c, region="packet", chain=None))
    assert np.array_equal(r.count.cpu().numpy()[:n_out], w["count"][src])


def test_refusals(P):
    L = P._L
    c = S.all_cases()["edges_payload"]
    sc = pktgpu.Scanner(P, S.tables(c["pats"]))
    kw, _ = dev_batch(c["batch"])
    b = P._batch(kw["slab"], kw["n"], kw["stride"], kw["offsets"], kw["lens"])
    n = b.n
    cols = {k: dev(v) for k, v in c["chain"].items()}
    ch = P._chain(cols)
    _, st = guarded(n, FILL)
    _, out = guarded(8 * (n + 1), FILL)

    def rc(batch=b, chain=ch, region=1, matched=None, hits=None):
        r = L.pkt_scan_batch(sc._t, ctypes.byref(batch), None if chain is None else ctypes.byref(chain), region, None,
                             st.data_ptr(), None, None, None, None, None, matched, hits, None)
        return r, L.pkt_scan_last_error(sc._t).decode() if r else ""

    assert rc(chain=None) == (-1, "pkt_scan_batch: null chain with PKT_SCAN_PAYLOAD")
    for k in range(3):
        p = [cols[x].data_ptr() for x in ("n_hdrs", "hdr_type", "hdr_off")]
        p[k] = None
        assert rc(chain=P._lib.PktChain(*p)) == (-1, "pkt_scan_batch: null chain column")
    assert rc(region=2) == (-1, "pkt_scan_batch: unknown region")
    assert rc(matched=out.data_ptr() + 4) == (-1, "pkt_scan_batch: matched / hits not 8-byte aligned")
    assert rc(hits=out.data_ptr() + 1) == (-1, "pkt_scan_batch: matched / hits not 8-byte aligned")
    huge = P._lib.PktBatch()
    huge.slab, huge.slab_len, huge.stride, huge.n = b.slab, b.slab_len, 64, 1 << 32
    assert rc(batch=huge) == (-1, "pkt_scan_batch: n >= 2^32")
    for bad, msg in ((dict(offsets=b.offsets, lens=None, stride=0), "offsets without lens"),
                     (dict(offsets=None, lens=None, stride=0), "stride 0"),
                     (dict(offsets=b.offsets, lens=b.lens, stride=0, slab=None), "null slab"),
                     (dict(offsets=b.offsets, lens=b.lens, stride=0, slab=b.slab + 4), "slab not 16-byte aligned")):
        x = P._lib.PktBatch()
        x.slab, x.slab_len, x.n = bad.get("slab", b.slab), b.slab_len - 16, n
        x.offsets, x.lens, x.stride = bad["offsets"], bad["lens"], bad["stride"]
        assert rc(batch=x) == (-1, "pkt_scan_batch: " + msg)
    import torch
    torch.cuda.synchronize()
    assert bool((st == FILL).all())                                     # a refusal launches nothing
    empty = P._lib.PktBatch()
    assert rc(batch=empty) == (0, "")                                   # n == 0 succeeds
    assert rc() == (0, "")
    torch.cuda.synchronize()
    assert np.array_equal(st.cpu().numpy(), S.expected("edges_payload")["status"])
    # create: the text is the ctx's
    t = np.zeros(1, schema.SCAN_PATTERN_DTYPE)
    h = ctypes.c_void_p()
    blob = np.zeros(8, np.uint8)
    assert L.pkt_scan_create(P._ctx, blob.ctypes.data, 8, t.ctypes.data, 1, 0, ctypes.byref(h)) == -1
    assert L.pkt_ctx_last_error(P._ctx).decode() == "pkt_scan_create: pattern 0: len is not in 1..PKT_SCAN_MAX_LEN"
    t["len"], t["group"] = 8, 64
    assert L.pkt_scan_create(P._ctx, blob.ctypes.data, 8, t.ctypes.data, 1, 0, ctypes.byref(h)) == -1
    assert "group above 63" in L.pkt_ctx_last_error(P._ctx).decode()
    with pytest.raises(RuntimeError, match="pkt_scan_create"):
        P.scanner([b"x" * 65])
