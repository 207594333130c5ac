"""pkt_dispatch_batch and pkt_reorder_batch (Parser.dispatcher / Parser.reorder / pktgpu.segments): the kernels
of pktgpu_dispatch.hip against dispatch_cases' yardstick (numpy from the header's text) and the host twins.  Every
input and output lies between two guard regions filled with 0xA5; the outputs themselves start as 0x77, so that
a byte the call must not write is seen."""
import ctypes

import numpy as np
import pytest

from pktgpu import schema

import compare_cases as C
import dispatch_cases as D
import flow_cases as F
import match_cases as M

pytestmark = pytest.mark.gpu
GUARD = 4096
INVALID = -1
T = 2048  # the count kernel's tile: kTile of pktgpu_dispatch.hip (256 threads x 8 rounds)
SCAN_PASS = 1024  # the elements of the [bucket][tile] counts a scan block covers per pass of its loop (kScanPass)
SCAN_BLOCKS = 256  # and the most blocks the scan launches (kScanMaxBlocks)
NAMES = ("bucket", "perm", "rank", "start")
DT = dict(bucket=np.uint16, perm=np.uint32, rank=np.uint32, start=np.uint64)


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


def guarded(nbytes, fill=None, shift=0):
    """A 0xA5-filled allocation with `nbytes` in its middle (filled with `fill`) -> (all, middle)."""
    import torch
    big = torch.full((GUARD + shift + (nbytes + 15) // 16 * 16 + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    mid = big[GUARD + shift:GUARD + shift + nbytes]
    if fill is not None:
        mid.fill_(fill)
    return big, mid


def guarded_copy(a):
    a = np.ascontiguousarray(a)
    big, mid = guarded(a.nbytes)
    if a.nbytes:
        mid.copy_(dev(a.view(np.uint8).reshape(-1)))
    return big, mid


def guards_intact(big, mid):
    lo = mid.data_ptr() - big.data_ptr()
    return bool((big[:lo] == 0xA5).all()) and bool((big[lo + mid.numel():] == 0xA5).all())


_DISP = {}


def dispatcher(P, nb, table=None, max_n=4 * T):
    """One handle per definition for the module: create is the only allocation."""
    k = (nb, None if table is None else np.asarray(table, np.uint16).tobytes(), max_n)
    if k not in _DISP:
        _DISP[k] = P.dispatcher(nb, table, max_n)
    return _DISP[k]


def run_dispatch(P, d, key, select=None, outputs=NAMES, n=None, stream=None, start_shift=0, null_key=False):
    """pkt_dispatch_batch with every array between guards -> (rc, {name: numpy}, guards intact, untouched)."""
    import torch
    key = np.ascontiguousarray(key, np.uint32)
    n = key.size if n is None else n
    gk = guarded_copy(key)
    gs = None if select is None else guarded_copy(np.ascontiguousarray(select, np.uint8))
    bufs = {}
    for name in outputs:
        cnt = d.nbuckets + 2 if name == "start" else key.size
        bufs[name] = guarded(cnt * np.dtype(DT[name]).itemsize + (8 if name == "start" else 0), D.FILL)
    ptr = lambda g: g[1].data_ptr() if g is not None and g[1].numel() else None  # noqa: E731
    st = ptr(bufs.get("start"))
    rc = P._L.pkt_dispatch_batch(d._d, None if null_key else ptr(gk), ptr(gs), n, ptr(bufs.get("bucket")), ptr(bufs.get("perm")),
                                 ptr(bufs.get("rank")), st + start_shift if st else None, P._stream(stream))
    torch.cuda.synchronize()
    raw = {name: g[1].cpu().numpy() for name, g in bufs.items()}
    got = {}
    for name, r in raw.items():
        a = r[:r.size - 8] if name == "start" else r
        got[name] = a.view(DT[name])
    intact = all(guards_intact(*g) for g in list(bufs.values()) + [gk] + ([gs] if gs else []))
    intact = intact and np.array_equal(gk[1].cpu().numpy().view(np.uint32), key)
    if "start" in raw:  # the spare word after start stays as it was
        intact = intact and (raw["start"][-8:] == D.FILL).all()
    untouched = all((r == D.FILL).all() for r in raw.values())
    return rc, got, intact, untouched


def check_against_yardstick(P, d, key, table, select, label, twin=False, outputs=NAMES):
    import pktgpu
    want = D.expect_dispatch(key, d.nbuckets, table, select)
    rc, got, intact, _ = run_dispatch(P, d, key, select, outputs)
    assert rc == 0 and intact, label
    assert set(got) == set(outputs)
    D.check_dispatch(got, want, label)
    if twin:
        D.check_dispatch(got, pktgpu.dispatch(key, d.nbuckets, table, select), label + " (host twin)")
    return got


@pytest.mark.parametrize("c", D.dispatch_cases(), ids=lambda c: c["name"])
def test_cases(P, c):
    d = dispatcher(P, c["nb"], c["table"])
    check_against_yardstick(P, d, c["key"], c["table"], c["select"], c["name"], twin=True)


EDGE_N = [1, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 3 * T + 137]


@pytest.mark.parametrize("kind", ["uniform", "one", "dropped", "alternate"])
@pytest.mark.parametrize("nb", [1, 3, 256])
def test_edges(P, nb, kind):
    d = dispatcher(P, nb)
    for n in EDGE_N:
        key = D.edge_keys(kind, n, nb)
        bp = D.bprime(key, nb)
        if kind == "one":
            assert (bp == nb - 1).all()
        elif kind == "dropped":
            assert (bp == nb).all()
        elif kind == "alternate" and n > 1 and nb > 1:
            assert (bp[0::2] == 0).all() and (bp[1::2] == nb - 1).all()
        check_against_yardstick(P, d, key, None, None, f"{kind} nb {nb} n {n}")


def test_edges_with_a_table_and_select(P):
    rng = np.random.default_rng(8)
    tab = rng.integers(0, 256, 4096).astype(np.uint16)
    tab[::50] = D.DROP
    d = dispatcher(P, 256, tab)
    for n in (T - 1, T + 1, 3 * T + 137):
        key = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        sel = (rng.integers(0, 4, n) != 0).astype(np.uint8)
        check_against_yardstick(P, d, key, tab, sel, f"table n {n}", twin=True)


def test_scan_passes(P):
    """Keys only, 256 buckets, at an n that is no multiple of T and has more tiles than a scan block covers in one
    pass: the 257 x 1026 counts are more than SCAN_BLOCKS x SCAN_PASS, so every scan block loops (two passes),
    sums the chunks below its own, and bucket rows cross block boundaries."""
    import torch
    nb = 256
    n = 1025 * T + 137
    tiles = -(-n // T)
    assert n % T and tiles > SCAN_PASS and (nb + 1) * tiles > SCAN_BLOCKS * SCAN_PASS
    rng = np.random.default_rng(99)
    key = rng.integers(0, nb + 1, n).astype(np.uint32)
    want = D.expect_dispatch(key, nb)
    assert (np.diff(want["start"].astype(np.int64)) > 0).all()  # every bucket and the drop tail are populated
    d = P.dispatcher(nb, None, max_n=n)
    try:
        got = d.run(dev(key), outputs=("perm", "rank", "start"))
        torch.cuda.synchronize()
        D.check_dispatch({k: v.cpu().numpy() for k, v in got.items()}, want, "scan passes")
    finally:
        d.close()


def test_determinism_two_handles_two_streams(P):
    import torch
    rng = np.random.default_rng(4)
    n = 3 * T + 137
    key = dev(rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32))
    tab = (np.arange(128) % 7).astype(np.uint16)
    hs = [P.dispatcher(7, tab, max_n=n) for _ in range(2)]
    ss = [torch.cuda.Stream(), torch.cuda.Stream()]
    try:
        key.cpu()  # (the upload is done before the side streams read it)
        perms = []
        for rep in range(2):
            for h, s in zip(hs, ss):
                perms.append(h.run(key, outputs=("perm",), stream=s)["perm"])
        torch.cuda.synchronize()
        want = D.expect_dispatch(key.cpu().numpy(), 7, tab)["perm"]
        for p in perms:
            assert np.array_equal(p.cpu().numpy(), want)
    finally:
        for h in hs:
            h.close()


def test_every_null_output_combination(P):
    c = next(c for c in D.dispatch_cases() if c["name"] == "table_128_4_full")
    d = dispatcher(P, c["nb"], c["table"])
    key = np.concatenate([c["key"]] * 3)[:T + 300]
    for outs in D.OUTPUT_SETS:
        check_against_yardstick(P, d, key, c["table"], None, str(outs), outputs=outs)
    # n == 0: start zero-filled on the stream, nothing else
    rc, got, intact, _ = run_dispatch(P, d, np.zeros(0, np.uint32), outputs=("start",))
    assert rc == 0 and intact and got["start"].tolist() == [0] * (c["nb"] + 2)


def test_refusals_come_before_any_launch(P):
    d = dispatcher(P, 3, None, max_n=100)
    key = np.arange(101, dtype=np.uint32) % 4
    bad = [("max_n", dict(n=101)), ("2^32", dict(n=1 << 32)), ("start not 8-byte aligned", dict(n=100, start_shift=4)),
           ("null key", dict(n=100, null_key=True))]
    for text, kw in bad:
        rc, got, intact, untouched = run_dispatch(P, d, key, **kw)
        assert rc == INVALID and intact and untouched, text
        msg = P._L.pkt_ctx_last_error(P._ctx).decode()
        assert msg.startswith("pkt_dispatch") and text in msg, (text, msg)
    rc, got, intact, _ = run_dispatch(P, d, key[:100])
    assert rc == 0 and intact
    D.check_dispatch(got, D.expect_dispatch(key[:100], 3), "after the refusals")
    # create
    h = ctypes.c_void_p()
    t3 = np.zeros(3, np.uint16)
    t2 = np.array([0, 3], np.uint16)
    big = np.zeros(8192, np.uint16)
    for args in ((0, None, 0, 10), (257, None, 0, 10), (3, t3, 3, 10), (3, big, 8192, 10), (3, t2, 0, 10), (3, t2, 2, 10),
                 (3, None, 0, 0), (3, None, 0, 1 << 32)):
        tab = args[1].ctypes.data if args[1] is not None else None
        assert P._L.pkt_dispatch_create(P._ctx, args[0], tab, args[2], args[3], ctypes.byref(h)) == INVALID, args
        assert P._L.pkt_ctx_last_error(P._ctx).decode().startswith("pkt_dispatch") and not h.value, args
    with pytest.raises(RuntimeError, match="pkt_dispatch"):
        P.dispatcher(0)


# ------------------------------------------------------------------ reorder
def dev_batch(b):
    big, slab = guarded(b["slab"].size)
    slab.copy_(dev(b["slab"]))
    kw = dict(slab=slab, n=b["n"], stride=b["stride"], offsets=None if b["offsets"] is None else dev(b["offsets"]),
              lens=None if b["lens"] is None else dev(b["lens"]))
    return kw, big


def run_reorder(P, b, perm, cols, want_cols, seg, nseg, slot, **over):
    """pkt_reorder_batch with every array between guards, the outputs 0x77-filled -> (rc, dst, out_len, columns,
    guards intact and inputs unchanged, outputs untouched)."""
    import torch
    perm = np.ascontiguousarray(perm, np.uint32)
    m = over.get("m", perm.size)
    ma = min(m, 4096)
    kw, big = dev_batch(b)
    bs = P._batch(kw["slab"], kw["n"], kw["stride"], kw["offsets"], kw["lens"])
    gp = guarded_copy(perm)
    gseg = None if seg is None else guarded_copy(np.ascontiguousarray(seg, np.uint64))
    gd = guarded(ma * slot - over.get("dst_short", 0), D.FILL, shift=over.get("dst_shift", 0)) if slot else None
    gl = guarded(ma * 4, D.FILL) if slot or over.get("out_len_without_dst") else None
    ci, co, gin, gout = P._lib.PktOut(), P._lib.PktOut(), {}, {}
    for c in want_cols:
        a = np.ascontiguousarray(cols[c])
        gin[c] = guarded_copy(a)
        cnt = int(np.prod(schema.column_shape(c, ma)))
        gout[c] = guarded(cnt * a.dtype.itemsize, D.FILL)
        if c != over.get("out_only"):
            setattr(ci, c, gin[c][1].data_ptr())
        setattr(co, c, gout[c][1].data_ptr())
    ptr = lambda g: g[1].data_ptr() if g is not None and g[1].numel() else None  # noqa: E731
    rc = P._L.pkt_reorder_batch(P._ctx, ctypes.byref(bs), ctypes.byref(ci), None if over.get("perm_null") else ptr(gp), m,
                                ptr(gseg), nseg, ptr(gd), gd[1].numel() if gd else 0, slot or 0, ptr(gl), ctypes.byref(co),
                                P._stream(None))
    torch.cuda.synchronize()
    dst = gd[1].cpu().numpy() if gd else None
    out_len = gl[1].cpu().numpy().view(np.uint32) if gl else None
    oc = {c: g[1].cpu().numpy().view(np.ascontiguousarray(cols[c]).dtype) for c, g in gout.items()}
    every = [gp, (big, kw["slab"])] + [g for g in (gseg, gd, gl) if g] + list(gin.values()) + list(gout.values())
    intact = all(guards_intact(*g) for g in every) and np.array_equal(kw["slab"].cpu().numpy(), b["slab"])
    intact = intact and all(np.array_equal(gin[c][1].cpu().numpy(), np.ascontiguousarray(cols[c]).view(np.uint8).reshape(-1))
                            for c in gin)
    untouched = all((a.view(np.uint8) == D.FILL).all() for a in [dst, out_len] + list(oc.values()) if a is not None)
    return rc, dst, out_len, oc, intact, untouched


@pytest.mark.parametrize("c", D.reorder_cases(), ids=lambda c: c["name"])
def test_reorder_cases(P, c):
    b, cols = D.sources()[c["src"]]
    want = D.expect_reorder(b, c["perm"], {k: cols[k] for k in c["cols"]}, c["seg"], c["nseg"], c["slot"])
    rc, dst, out_len, oc, intact, _ = run_reorder(P, b, c["perm"], cols, c["cols"], c["seg"], c["nseg"], c["slot"])
    assert rc == 0 and intact, c["name"]
    D.check_reorder(dst, out_len, oc, want, c["name"])


@pytest.mark.parametrize("al", range(16))
def test_reorder_every_source_alignment(P, al):
    b0, cols = D.sources()["ref22"]
    b = D.aligned(b0, al)
    perm = np.random.default_rng(al).permutation(b["n"] + 2).astype(np.uint32)  # two empty positions
    seg = np.array([0, 5, 5, b["n"] - 1], np.uint64)  # an empty segment; the last three positions are not written
    for slot in (48, 1536):
        want = D.expect_reorder(b, perm, {}, seg, 3, slot)
        rc, dst, out_len, oc, intact, _ = run_reorder(P, b, perm, cols, (), seg, 3, slot)
        assert rc == 0 and intact
        D.check_reorder(dst, out_len, oc, want, f"align {al} slot {slot}")


def test_reorder_more_than_one_block(P):
    """600 positions (three blocks of the kernels, the last one partial) over the fixed-stride mix, repeats and
    empty positions included, in 9 segments."""
    b, cols = D.sources()["mix_stride"]
    rng = np.random.default_rng(12)
    m = 600
    perm = rng.integers(0, b["n"] + 10, m).astype(np.uint32)
    seg = np.sort(np.concatenate([[0, 0], rng.integers(0, m, 6), [m - 40, m - 40]])).astype(np.uint64)
    want = D.expect_reorder(b, perm, {k: cols[k] for k in D.COLSETS[4]}, seg, 9, 128)
    rc, dst, out_len, oc, intact, _ = run_reorder(P, b, perm, cols, D.COLSETS[4], seg, 9, 128)
    assert rc == 0 and intact
    D.check_reorder(dst, out_len, oc, want, "600 positions")


def test_reorder_refusals_come_before_any_launch(P):
    b, cols = D.sources()["ref22"]
    n = b["n"]
    perm = np.arange(n, dtype=np.uint32)
    seg = np.array([0, n], np.uint64)
    bad = [("slot", dict(slot=8)), ("slot", dict(slot=24)), ("dst not 16-byte aligned", dict(slot=1536, dst_shift=8)),
           ("dst_len", dict(slot=64, dst_short=1)), ("m >= 2^32", dict(m=1 << 32)),
           ("nseg", dict(nseg=258, seg=np.zeros(259, np.uint64))), ("seg_start", dict(nseg=1, seg=None)),
           ("null perm", dict(perm_null=True)), ("out_len without dst", dict(slot=None, out_len_without_dst=True)),
           ("out column", dict(out_only="hdr_off")), ("stride 0", dict(b=dict(slab=b["slab"], stride=0, n=n, offsets=None, lens=None))),
           ("slab not 16-byte aligned", dict(b=dict(b, slab=b["slab"][1:])))]
    for text, kw in bad:
        kw = dict(kw)
        bb = kw.pop("b", b)
        slot = kw.pop("slot", 64)
        sg, ns = kw.pop("seg", seg), kw.pop("nseg", 1)
        if text == "slab not 16-byte aligned":
            kw_b, big = dev_batch(bb)
            bs = P._batch(kw_b["slab"], n, None, kw_b["offsets"], kw_b["lens"])
            bs.slab += 1
            gd = guarded(64 * n, D.FILL)
            rc = P._L.pkt_reorder_batch(P._ctx, ctypes.byref(bs), None, dev(perm).data_ptr(), n, None, 0, gd[1].data_ptr(),
                                        64 * n, 64, None, None, P._stream(None))
            import torch
            torch.cuda.synchronize()
            untouched, intact = bool((gd[1] == D.FILL).all()), guards_intact(*gd)
        else:
            rc, dst, out_len, oc, intact, untouched = run_reorder(P, bb, perm, cols, ("n_hdrs", "hdr_off"), sg, ns, slot, **kw)
        assert rc == INVALID and intact and untouched, text
        assert text in P._L.pkt_ctx_last_error(P._ctx).decode(), (text, P._L.pkt_ctx_last_error(P._ctx))
    # m == 0 succeeds and launches nothing
    rc, dst, out_len, oc, intact, untouched = run_reorder(P, b, perm, cols, ("n_hdrs",), None, 0, 64, m=0)
    assert rc == 0 and intact and untouched


# ------------------------------------------------------------------ the queue loop
def test_end_to_end_queues(P):
    """parse -> flow_keys(rss) -> a 128-entry table over 4 queues -> reorder with the chain columns; each queue's
    segment is then a batch of its own for match, l4_checksum, flow_keys and pcap_write."""
    import pktgpu
    import torch
    rng = np.random.default_rng(31)
    pkts = M.random_mix(rng, 300)
    b = C.indexed(pkts, rng)
    n = b["n"]
    table = (np.arange(128) % 4).astype(np.uint16)
    # the premise, on the CPU with the host twins: at least two queues are non-empty
    hch = M.L4.chain_of(b)
    hk = pktgpu.flow_keys(b["slab"], hch, symmetric=True, rss_key=F.RSS_KEY, offsets=b["offsets"], lens=b["lens"])
    hd = pktgpu.dispatch(hk["rss"], 4, table)
    assert (np.diff(hd["start"][:5].astype(np.int64)) > 0).sum() >= 2 and int(hd["start"][4]) == n
    kw, big = dev_batch(b)
    src = dict(offsets=kw["offsets"], lens=kw["lens"])
    res = P.parse(kw["slab"], columns=["chain"], **src)
    chain = {c: res[c] for c in ("n_hdrs", "hdr_type", "hdr_off")}
    fk = P.flow_keys(kw["slab"], chain, symmetric=True, rss_key=F.RSS_KEY, **src)
    d = dispatcher(P, 4, table)
    r = d.run(fk["rss"])
    slot = (max(len(p) for p in pkts) + 15) // 16 * 16
    ro = P.reorder(r["perm"], kw["slab"], columns=chain, start=r["start"], slot=slot, **src)
    segs = pktgpu.segments(r["start"], ro)
    torch.cuda.synchronize()
    perm, start = r["perm"].cpu().numpy().astype(np.int64), r["start"].cpu().numpy().astype(np.int64)
    D.check_dispatch({k: v.cpu().numpy() for k, v in r.items()}, hd, "device rss dispatch against the host twins")
    prog = M.acl()
    mp = P.match_program(M.to_ctypes(prog), prog["default"])
    whole = {"match": P.match(kw["slab"], chain, mp, **src), "l4": P.l4_checksum(kw["slab"], chain, which=pktgpu.schema.L4_LAST, **src),
             "flow": fk}
    whole = {k: {c: t.cpu().numpy() for c, t in v.items()} for k, v in whole.items()}
    seen = {}
    assert len(segs) == 4 and sum(s["n"] for s in segs) == n
    for q, s in enumerate(segs):
        if not s["n"]:
            continue
        pq = perm[start[q]:start[q + 1]]
        assert (np.diff(pq) > 0).all() and s["n"] == pq.size
        part = {"match": P.match(prog=mp, **s), "l4": P.l4_checksum(which=pktgpu.schema.L4_LAST, **s),
                "flow": P.flow_keys(symmetric=True, rss_key=F.RSS_KEY, **s)}
        for call, out in part.items():
            for c, t in out.items():
                assert np.array_equal(t.cpu().numpy(), whole[call][c][pq]), (q, call, c)
        for i in pq[whole["flow"]["status"][pq] == 0]:
            assert seen.setdefault(whole["flow"]["keys"][i].tobytes(), q) == q  # a flow lives in one queue
        cap, cnt, offs, lens, idx = P.pcap_write(s["slab"], lens=s["lens"], stride=s["stride"], n=s["n"])
        got = C.packets(C.batch(cap.cpu().numpy(), offs.cpu().numpy(), lens.cpu().numpy()))
        assert cnt == pq.size and got == [pkts[i] for i in pq], q
    mp.close()
    assert guards_intact(big, kw["slab"]) and np.array_equal(kw["slab"].cpu().numpy(), b["slab"])


def test_stream_loop(P):
    """push -> poll -> the stream's parse columns -> match -> dispatch by rule (DIRECT) -> reorder -> release, in
    windows of cap = 8 over ref22.pcap: the per-bucket packet lists concatenated over the windows equal one host
    dispatch of the whole file."""
    import pktgpu
    import torch
    from pktgpu.stream import PcapStream
    rng = np.random.default_rng(13)
    b, ch, prog, want = M.all_cases()["ref22_first_match_order"]
    raw = b["slab"].tobytes()
    pk = C.packets(b)
    nb = len(prog["rules"])
    hd = pktgpu.dispatch(want["rule"].astype(np.uint32), nb)  # MATCH_NONE (0xFF) >= nb: dropped
    assert (np.diff(hd["start"].astype(np.int64)) > 0).sum() >= 2
    expect = [[pk[i] for i in hd["perm"][int(hd["start"][q]):int(hd["start"][q + 1])]] for q in range(nb)]
    mp = P.match_program(M.to_ctypes(prog), prog["default"])
    cap = 8
    d = dispatcher(P, nb, None, max_n=cap)
    st = PcapStream(0, max_bytes=1 << 20, cap=cap, columns=["chain"])
    queues = [[] for _ in range(nb)]
    try:
        at = 0
        while at < len(raw):
            k = int(rng.integers(1, 700))
            st.push(raw[at:at + k])
            at += k
        while True:
            n, _ = st.poll()
            last = n <= cap
            if last:
                n, _ = st.finish()
            slab, offs, lens = st.batch()
            k = offs.numel()
            chain = {c: st.out[c] if k == cap else st.out[c][..., :k].contiguous() for c in ("n_hdrs", "hdr_type", "hdr_off")}
            rule = P.match(slab, chain, mp, offsets=offs, lens=lens, outputs=("rule",))["rule"]
            r = d.run(rule.to(torch.int32).view(torch.uint32), outputs=("perm", "start"))
            ro = P.reorder(r["perm"], slab, offsets=offs, lens=lens, columns=chain, start=r["start"], slot=1536)
            for q, s in enumerate(pktgpu.segments(r["start"], ro)):
                if s["n"]:
                    queues[q] += C.packets(C.batch(s["slab"].cpu().numpy(), lens=s["lens"].cpu().numpy(), stride=s["stride"], n=s["n"]))
            if last:
                break
            torch.cuda.synchronize()  # the window's readers are done before the stream moves it
            st.release(cap)
        assert queues == expect
    finally:
        st.close()
        mp.close()
