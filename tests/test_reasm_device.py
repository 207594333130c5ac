"""pkt_reasm_batch / _async / _result (Parser.reassemble): the kernels of pktgpu_reasm.hip against reasm_cases'
yardstick (an independent Python model) and the host twin pkt_reasm_host, which groups by a sort and a walk where the
kernels use two hash tables and five words per datagram.  The case list is the one test_reasm_host.py runs.  dst and
every output array lie between two guard regions filled with 0xA5, the outputs start as 0x77, and dst at and past the
total must still be 0x77 after the call."""
import ctypes

import numpy as np
import pytest

import pktgpu

import frag_cases as G
import reasm_cases as R

pytestmark = pytest.mark.gpu
GUARD = 4096
FILL = 0x77
INVALID = -1
N_MIX = 3 * 256 + 131  # three tiles of the per-packet kernels and a ragged one


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


SHAPES = dict(status=np.uint8, out_index=np.uint32, out_off=np.uint64, out_len=np.uint32, src_index=np.uint32, nfrag=np.uint32,
              oc_n_hdrs=np.uint8, oc_hdr_type=np.uint8, oc_hdr_off=np.uint16, hits=np.uint64)
PER_OUTPUT = {"dst", "out_off", "out_len", "src_index", "nfrag", "oc_n_hdrs", "oc_hdr_type", "oc_hdr_off"}


def run(P, b, ch, select=None, which=0, flags=0, cap=None, dst_len=None, skip=(), mode="sync", over=None):
    """pkt_reasm_batch over a device copy of the batch -> (rc, got, guards intact).  cap / dst_len default to the
    model-free sizing pass (PKT_REASM_NO_WRITE).  hits start as 0x77.. and come back less that."""
    import torch
    L = P._L
    slab = dev(b["slab"])
    offs = None if b["offsets"] is None else dev(b["offsets"])
    lens = None if b["lens"] is None else dev(b["lens"])
    pb = P._batch(slab, b["n"], b["stride"], offs, lens)
    dch = {k: dev(v) for k, v in ch.items()}
    pc = P._chain(dch)
    n = b["n"]
    sel = None if select is None else dev(np.asarray(select, np.uint8))
    tp = lambda t: t.data_ptr() if t is not None and t.numel() else None  # noqa: E731
    tot, cnt = ctypes.c_uint64(0), ctypes.c_uint64(0)
    head = [P._ctx, ctypes.byref(pb), ctypes.byref(pc), which]
    if cap is None or dst_len is None:
        rc = L.pkt_reasm_batch(*head, flags | R.NO_WRITE, tp(sel), None, None, None, 0, 0, None, None, None, None, None, None,
                               ctypes.byref(tot), ctypes.byref(cnt), P._stream(None))
        assert rc == 0
        cap = max(1, cnt.value) if cap is None else cap
        dst_len = tot.value if dst_len is None else dst_len
    counts = dict(status=n, out_index=n, out_off=cap, out_len=cap, src_index=cap, nfrag=cap, oc_n_hdrs=cap,
                  oc_hdr_type=R.MAXH * cap, oc_hdr_off=R.MAXH * cap, hits=R.NSTATUS)
    if flags & R.NO_WRITE:
        skip = set(skip) | PER_OUTPUT
    bufs = {k: guarded(counts[k] * np.dtype(dt).itemsize, FILL) for k, dt in SHAPES.items() if k not in skip}
    if "dst" not in skip:
        bufs["dst"] = guarded(dst_len + 64, FILL)  # 64 more bytes the call is not told of
    p = lambda k: bufs[k][1].data_ptr() if k in bufs and bufs[k][1].numel() else None  # noqa: E731
    oc = P._lib.PktChain(p("oc_n_hdrs"), p("oc_hdr_type"), p("oc_hdr_off"))
    args = head + [flags, tp(sel), p("status"), p("out_index"), p("dst"), dst_len, cap, p("out_off"), p("out_len"),
                   p("src_index"), p("nfrag"), ctypes.byref(oc), p("hits")]
    for k, v in dict(over or {}).items():
        args[k] = v
    if mode == "sync":
        rc = L.pkt_reasm_batch(*args, ctypes.byref(tot), ctypes.byref(cnt), P._stream(None))
    else:
        rc = L.pkt_reasm_batch_async(*args, P._stream(None))
        if rc == 0:
            if mode == "async_twice":  # the one-in-flight rule
                rc2 = L.pkt_reasm_batch_async(*args, P._stream(None))
                msg = P._L.pkt_ctx_last_error(P._ctx).decode()
                assert rc2 == INVALID and msg.startswith("pkt_reasm") and "pkt_reasm_result" in msg
            rc = L.pkt_reasm_result(P._ctx, ctypes.byref(tot), ctypes.byref(cnt))
    torch.cuda.synchronize()
    got = {k: g[1].cpu().numpy().view(SHAPES.get(k, np.uint8)) for k, g in bufs.items()}
    if "hits" in got:
        got["hits"] = got["hits"] - np.uint64(0x7777777777777777)
    got["n_out"], got["bytes_out"], got["cap"] = cnt.value, tot.value, cap
    intact = all(guards_intact(*g) for g in bufs.values())
    return rc, got, intact


def verify(got, want, label):
    R.check(got, want, got["cap"], label)
    assert (got["dst"][want["bytes_out"]:] == FILL).all(), (label, "dst written at or past the total")


def twin(b, ch, select=None, which=0, flags=0):
    rc, h = R.host_call(b, ch, select, which, flags)
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
        items, sel = R.mix(N_MIX)
        b, ch = R.layout(items, kind)
        return b, ch, sel, R.expect(b, ch, sel)
    return R.cached(("dev_mix", kind), build)


# ------------------------------------------------------------------ the case list, both layouts
@pytest.mark.parametrize("kind", ["indexed", "stride"])
@pytest.mark.parametrize("name", R.CASES)
def test_cases(P, name, kind):
    c = R.get_case(name)
    b, ch = R.layout(c["items"], kind)
    want = R.expect(b, ch, c["select"], c["which"])
    rc, got, intact = run(P, b, ch, c["select"], c["which"])
    assert rc == 0 and intact
    verify(got, want, name)
    R.check_case(name, c, got, want)
    assert int(got["hits"].sum()) == b["n"]


# ------------------------------------------------------------------ the mix, both layouts
@pytest.mark.parametrize("kind", ["indexed", "stride"])
def test_mix_against_the_model_and_the_host_twin(P, kind):
    """Datagrams of 9..3000 payload bytes cut at 28 / 68 / 576 / 1280 and shuffled inside windows, broken ones and whole
    packets among them, source packets at every alignment 0..15, more than three tiles of the per-packet kernels."""
    b, ch, sel, want = mix(kind)
    counts = np.bincount(want["status"], minlength=R.NSTATUS)
    assert all(counts[s] >= 3 for s in (R.WHOLE, R.JOINED, R.PENDING, R.SKIPPED, R.NO_IP, R.BAD_HDR)), counts
    if kind == "indexed":
        assert {int(o) % 16 for o in b["offsets"][:16]} == set(range(16)) and int(b["offsets"][-1]) + int(b["lens"][-1]) == b["slab"].size
    rc, got, intact = run(P, b, ch, sel)
    assert rc == 0 and intact
    verify(got, want, kind)
    same_as_twin(got, twin(b, ch, sel), kind)
    assert int(got["hits"].sum()) == b["n"]


def test_1282_tiles_a_counting_block_takes_two(P):
    """1280 * 256 + 257 packets: with hits the counting launch is capped at 1280 blocks, so two of them take a second
    tile, the last one ragged.  Whole 60-byte packets (no fragments) at stride 64, every 61st selected.  Against the
    host twin alone: the Python model is too slow at this size, and test_reasm_host.py holds the twin to it."""
    n = 1280 * 256 + 257
    b, ch = G.tiled([G.v4(26, seed=k) for k in range(4)], n)
    sel = (np.arange(n) % 61 == 0).astype(np.uint8)
    rc, got, intact = run(P, b, ch, sel)
    assert rc == 0 and intact
    h = twin(b, ch, sel)
    counts = np.bincount(h["status"], minlength=R.NSTATUS)
    assert counts[R.WHOLE] == h["n_out"] == -(-n // 61) and counts[R.SKIPPED] == n - counts[R.WHOLE]
    same_as_twin(got, h, "1282 tiles")
    assert np.array_equal(got["hits"], counts) and (got["dst"][h["bytes_out"]:] == FILL).all()


def test_two_runs_give_identical_bytes_and_arrays(P):
    b, ch, sel, want = mix("indexed")
    r1, g1, i1 = run(P, b, ch, sel)
    r2, g2, i2 = run(P, b, ch, sel)
    assert r1 == r2 == 0 and i1 and i2
    for k in g1:
        assert np.array_equal(g1[k], g2[k]), k


# ------------------------------------------------------------------ one group across waves and blocks
def test_one_datagram_of_300_eight_byte_fragments(P):
    orig = R.dgram(G.pattern(2400, 5), 0x0A01)
    g = R.frags(orig, 28)
    assert len(g) == 300
    for order in ("in_order", "shuffled"):
        b, ch = R.layout(R.arrange([g], order))
        want = R.expect(b, ch)
        rc, got, intact = run(P, b, ch)
        assert rc == 0 and intact and got["nfrag"].tolist() == [300] and got["src_index"].tolist() == [int(np.flatnonzero(want["status"] == R.JOINED).max())]
        verify(got, want, order)
        assert got["dst"][:got["out_len"][0]].tobytes() == R.original(orig)


@pytest.mark.parametrize("spoil", [False, True])
def test_900_packets_sharing_one_key(P, spoil):
    pay = G.pattern(8 * 900, 3)
    g = R.arrange([[R.mkfrag(pay, 8 * k, 8, k + 1 < 900, 0x0B01) for k in range(900)]], "shuffled", seed=9)
    if spoil:
        g[450] = g[300]
    b, ch = R.layout(g)
    want = R.expect(b, ch)
    assert (want["status"] == (R.PENDING if spoil else R.JOINED)).all()
    rc, got, intact = run(P, b, ch)
    assert rc == 0 and intact and got["n_out"] == (0 if spoil else 1)
    verify(got, want, f"one key, spoilt {spoil}")


# ------------------------------------------------------------------ sizing, overflow, flags, NULL outputs
def test_n_out_landing_on_out_cap_and_one_below_the_need(P):
    b, ch, sel, want = mix("stride")
    rc, got, intact = run(P, b, ch, sel, cap=want["n_out"], dst_len=want["bytes_out"])
    assert rc == 0 and intact
    verify(got, want, "exact")
    for cap, room in ((want["n_out"] - 1, want["bytes_out"]), (want["n_out"], want["bytes_out"] - 16)):
        rc, got, intact = run(P, b, ch, sel, cap=cap, dst_len=room)
        assert rc == INVALID and intact
        assert P._L.pkt_ctx_last_error(P._ctx).decode().startswith("pkt_reasm")
        assert (got["n_out"], got["bytes_out"]) == (want["n_out"], want["bytes_out"])
        for k in ("status", "hits"):
            assert np.array_equal(got[k], want[k]), k
    rc, got, intact = run(P, b, ch, sel, cap=want["n_out"] + 300, dst_len=want["bytes_out"] + 8192)
    assert rc == 0 and intact
    verify(got, want, "empty tail")


def test_only_joined(P):
    b, ch, sel, _ = mix("indexed")
    want = R.expect(b, ch, sel, flags=R.ONLY_JOINED)
    rc, got, intact = run(P, b, ch, sel, flags=R.ONLY_JOINED)
    assert rc == 0 and intact and all(k > 1 for k in got["nfrag"][:got["n_out"]])
    verify(got, want, "only_joined")


NULLABLE = ["status", "out_index", "src_index", "nfrag", "oc_n_hdrs", "oc_hdr_type", "oc_hdr_off", "hits"]


def test_no_write_and_null_outputs(P):
    b, ch, sel, want = mix("stride")
    rc, got, intact = run(P, b, ch, sel, flags=R.NO_WRITE)
    assert rc == 0 and intact
    R.check(got, want, 0, "no_write")
    for mask in list(range(1, 256, 37)) + [255] + [1 << j for j in range(8)]:
        skip = [k for j, k in enumerate(NULLABLE) if mask >> j & 1]
        rc, got, intact = run(P, b, ch, sel, skip=skip)
        assert rc == 0 and intact, skip
        verify(got, want, str(skip))
    rc, got, intact = run(P, b, ch, sel, flags=R.NO_WRITE, skip=["status", "hits"])
    assert rc == 0 and intact and np.array_equal(got["out_index"], want["out_index"])


def test_async_result_and_one_in_flight(P):
    b, ch, sel, want = mix("stride")
    for mode in ("async", "async_twice"):
        rc, got, intact = run(P, b, ch, sel, mode=mode)
        assert rc == 0 and intact
        verify(got, want, mode)
    tot, cnt = ctypes.c_uint64(5), ctypes.c_uint64(5)
    assert P._L.pkt_reasm_result(P._ctx, ctypes.byref(tot), ctypes.byref(cnt)) == INVALID
    assert P._L.pkt_ctx_last_error(P._ctx).decode().startswith("pkt_reasm_result")
    rc, got, intact = run(P, b, ch, sel, cap=want["n_out"] - 1, dst_len=want["bytes_out"], mode="async")
    assert rc == INVALID and intact and (got["n_out"], got["bytes_out"]) == (want["n_out"], want["bytes_out"])


def test_n_0_and_n_1(P):
    b, ch = R.layout([R.dgram(G.pattern(100, 1), 1)])
    b0 = dict(b, n=0, offsets=b["offsets"][:1], lens=b["lens"][:1])
    rc, got, intact = run(P, b0, ch, cap=70, dst_len=64, skip=["status", "out_index"])
    assert rc == 0 and intact and (got["n_out"], got["bytes_out"]) == (0, 0)
    assert (got["out_off"] == 0).all() and (got["out_len"] == 0).all() and (got["src_index"] == R.NONE).all()
    assert (got["nfrag"] == 0).all() and (got["oc_n_hdrs"] == 0).all() and (got["dst"] == FILL).all()
    assert (got["hits"] == 0).all()
    for item in (R.dgram(G.pattern(100, 1), 1), R.mkfrag(G.pattern(100, 1), 0, 48, True, 1)):
        b, ch = R.layout([item])
        rc, got, intact = run(P, b, ch)
        assert rc == 0 and intact
        verify(got, R.expect(b, ch), "n = 1")


# ------------------------------------------------------------------ the next calls take the output
def test_parse_and_l4_checksum_over_the_output(P):
    """The fragments of a UDP datagram give PKT_L4_FRAGMENT; the joined datagram, parsed again, gives PKT_L4_OK."""
    import torch
    origs = [R.udp_dgram(1000 + 37 * k, 0x0C00 + k, seed=k) for k in range(5)]
    items = R.arrange([R.frags(o, 576) for o in origs], "interleaved") + [R.udp_dgram(64, 0x0CFF)]
    b, ch = R.layout(items)
    slab, offs, lens = dev(b["slab"]), dev(b["offsets"]), dev(b["lens"])
    parsed = P.parse(slab, offsets=offs, lens=lens)
    before = P.l4_checksum(slab, parsed, offsets=offs, lens=lens)
    torch.cuda.synchronize()
    assert before["status"].cpu().numpy().tolist() == [pktgpu.L4_FRAGMENT] * (len(items) - 1) + [pktgpu.L4_OK]
    r = P.reassemble(dict(slab=slab, offsets=offs, lens=lens), parsed, hits=True)
    h = pktgpu.Parser.reassemble(None, b, ch, hits=True, host=True)
    assert r.n_out == h.n_out == 6 and r.bytes_out == h.bytes_out and np.array_equal(r.hits.cpu().numpy(), h.hits)
    for name in ("status", "out_index", "offsets", "lens", "src_index", "nfrag"):
        assert np.array_equal(getattr(r, name).cpu().numpy(), getattr(h, name)), name
    assert np.array_equal(r.slab.cpu().numpy()[:h.bytes_out], h.slab[:h.bytes_out]) and not bool(r.pending.any())
    outs = [h.slab[int(o):int(o) + int(ln)].tobytes() for o, ln in zip(h.offsets, h.lens)]
    assert sorted(outs) == sorted(o[0] for o in origs + [R.udp_dgram(64, 0x0CFF)])
    again = P.parse(r.slab, offsets=r.offsets, lens=r.lens)
    after = P.l4_checksum(r.slab, again, offsets=r.offsets, lens=r.lens)
    torch.cuda.synchronize()
    assert after["status"].cpu().numpy().tolist() == [pktgpu.L4_OK] * 6
    assert (again["n_hdrs"].cpu().numpy() >= 3).all()  # Ether / IPv4 / UDP: the joined datagram's L4 header is walked now


# ------------------------------------------------------------------ refusals
A_BATCH, A_CHAIN, A_WHICH, A_FLAGS, A_SELECT, A_STATUS, A_INDEX, A_DST, A_DST_LEN, A_CAP, A_OFF, A_LEN = range(1, 13)
A_HITS = 16


def test_refusal_texts(P):
    import torch
    b, ch = R.layout(R.five(0x0201))
    odd = torch.zeros(64, dtype=torch.uint8, device="cuda")
    base = odd.data_ptr()
    cases = {"which_ip": {A_WHICH: 16}, "flag": {A_FLAGS: 8}, "dst not 16": {A_DST: base + 8}, "hits not 8": {A_HITS: base + 4},
             "out_off not 8": {A_OFF: base + 4}, "null dst": {A_DST: None}, "null dst, out_off": {A_OFF: None},
             "out_len": {A_LEN: None}, "out_cap": {A_CAP: 0}, "out_cap is 0 or": {A_CAP: 1 << 32}, "null argument": {A_CHAIN: None}}
    for text, over in cases.items():
        rc, got, intact = run(P, b, ch, cap=8, dst_len=4096, over=over)
        msg = P._L.pkt_ctx_last_error(P._ctx).decode()
        assert rc == INVALID and intact and msg.startswith("pkt_reasm_batch: ") and text in msg, (text, msg)
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
        rc = P._L.pkt_reasm_batch(P._ctx, ctypes.byref(pb), ctypes.byref(pc), 0, R.NO_WRITE, None, None, None, None, 0, 0, None,
                                  None, None, None, None, None, ctypes.byref(tot), ctypes.byref(cnt), P._stream(None))
        msg = P._L.pkt_ctx_last_error(P._ctx).decode()
        assert rc == INVALID and msg.startswith("pkt_reasm_batch: ") and text in msg and (tot.value, cnt.value) == (0, 0), (form, msg)
