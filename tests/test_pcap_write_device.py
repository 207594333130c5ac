"""pkt_pcap_write on the device (Parser.pcap_write): a batch in HBM written out as a
tests/pcap.rs:7-37 capture by pktgpu_pcapw.hip.  Every expected capture is built record by record
with struct.pack (pcap_write_cases.expect, or gen.pcap_bytes for the generator pipeline), never with
the code under test.  The destination is pre-filled with 0xA5 and 64 bytes longer than asked for, so
a byte left unwritten or a write at or past the total shows."""
import numpy as np
import pytest

import oracle
from pktgpu import gen, schema

import pcap_write_cases as C

pytestmark = pytest.mark.gpu


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


def dev_args(c):
    ts = tuple(t if isinstance(t, int) else dev(t) for t in c["ts"])
    return dict(slab=dev(c["slab"]), offsets=None if c["offsets"] is None else dev(c["offsets"]),
                lens=None if c["lens"] is None else dev(c["lens"]), stride=c["stride"], n=c["n"],
                select=None if c["select"] is None else dev(c["select"]), snaplen=c["snaplen"], ts=ts)


def run(P, c, want=None, room=(0,), label="", args=None):
    """Write case c at every capacity total + r, into an 0xA5-filled buffer 64 bytes longer."""
    import torch
    want, w_off, w_len, w_src = C.expect(c) if want is None else want
    total = len(want)
    args = dev_args(c) if args is None else args
    for r in room:
        buf = torch.full((total + r + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        cap, n, offs, lens, src = P.pcap_write(dst=buf[:total + r], **args)
        got = buf.cpu().numpy()
        assert n == len(w_src) and cap.numel() == total, (label, r, n, cap.numel(), total)
        bad = np.flatnonzero(got[:total] != np.frombuffer(want, np.uint8))
        assert bad.size == 0, (label, r, "first differing bytes", bad[:8])
        assert (got[total:] == 0xA5).all(), (label, r, "written at or past the total")
        assert cap.data_ptr() == buf.data_ptr()
        assert np.array_equal(offs.cpu().numpy(), w_off) and np.array_equal(lens.cpu().numpy(), w_len), (label, r)
        assert np.array_equal(src.cpu().numpy(), w_src), (label, r)
    return want, w_off, w_len, w_src


@pytest.mark.parametrize("name", list(C.host_cases()))
def test_host_cases_on_device(P, name):
    c = C.host_cases()[name]
    want = run(P, c, room=(0, 1, 4096), label=name)[0]
    if name == "golden":
        assert want == C.golden()[0]
    i_off, i_len = gen.pcap_index_py(want)
    assert np.array_equal(i_off, C.expect(c)[1]) and np.array_equal(i_len, C.expect(c)[2])


def test_capacity_errors_and_defaults(P):
    import torch
    c = C.edges()
    want = C.expect(c)[0]
    total, args = len(want), dev_args(c)
    buf = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match=str(total)):  # one byte short: the size needed is reported
        P.pcap_write(dst=buf[:total - 1], **args)
    assert (buf[total - 1:].cpu().numpy() == 0xA5).all()  # nothing outside [0, dst_len)
    with pytest.raises(RuntimeError, match=str(total)):
        P.pcap_write(dst=buf[:16], **args)
    assert (buf[16:].cpu().numpy() == 0xA5).all()
    # dst=None: the bound summed on the device; index=False: no record table asked for
    cap, n, offs, lens, src = P.pcap_write(index=False, **args)
    assert cap.cpu().numpy().tobytes() == want and n == c["n"] and offs is None and lens is None and src is None
    sel = C.select_case("every_third")
    cap, n, *_ = P.pcap_write(**dev_args(sel))
    assert cap.cpu().numpy().tobytes() == C.expect(sel)[0]
    # a bool mask is taken as it is
    a = dev_args(sel)
    a["select"] = a["select"].bool()
    assert P.pcap_write(**a)[0].cpu().numpy().tobytes() == C.expect(sel)[0]


def window_edge_lens():
    """Lengths that put a record header, a record's first data byte and a record's last data byte at
    file offset 4096 m - k for each k, with small random records between them."""
    rng = np.random.default_rng(17)
    lens, want_at = [], []
    pos = 24

    def add(ln):
        nonlocal pos
        lens.append(ln)
        pos += 16 + ln

    for k in (0, 1, 8, 15, 16, 17):
        for what in ("header", "first", "last"):
            for _ in range(int(rng.integers(8, 20))):
                add(int(rng.integers(0, 90)))
            t = ((pos + 200) // 4096 + 1) * 4096 - k
            if what == "header":
                add(t - pos - 16)       # a filler ending where the header must start
                want_at.append((what, k, len(lens)))
                add(int(rng.integers(1, 90)))
            elif what == "first":
                add(t - 16 - pos - 16)  # the header starts 16 before the first data byte
                want_at.append((what, k, len(lens)))
                add(int(rng.integers(1, 90)))
            else:
                want_at.append((what, k, len(lens)))
                add(t - pos - 16 + 1)   # the last data byte at t
    return lens, want_at


def random_batch(lens, seed):
    """An indexed batch of the given lengths at random (unordered, overlapping) places of a random slab."""
    rng = np.random.default_rng(seed)
    slab = rng.integers(0, 256, max(4096, max(lens) + 4096), dtype=np.uint8)
    offs = [int(rng.integers(0, slab.size - ln + 1)) for ln in lens]
    ts = (rng.integers(0, 2**32, len(lens), dtype=np.uint64).astype(np.uint32),
          rng.integers(0, 2**32, len(lens), dtype=np.uint64).astype(np.uint32))
    return C.case(slab, offs, lens, ts=ts)


def test_window_edges(P):
    lens, want_at = window_edge_lens()
    assert 200 < len(lens) < 1000
    c = random_batch(lens, 18)
    want, w_off, w_len, _ = run(P, c, room=(0, 4096), label="window edges")
    for what, k, j in want_at:  # the construction puts them where it says
        at = {"header": int(w_off[j]) - 16, "first": int(w_off[j]), "last": int(w_off[j]) + int(w_len[j]) - 1}[what]
        assert (at + k) % 4096 == 0 and w_len[j] >= 1, (what, k, j, at)


def test_every_total_mod_16(P):
    seen = set()
    for r in range(16):
        c = random_batch([5, 33, 70, 4090, r], 30 + r)
        want = run(P, c, room=(0, 1), label=f"tail {r}")[0]
        seen.add(len(want) % 16)
    assert seen == set(range(16))


@pytest.mark.parametrize("before,windows", [(100, 17), (4000, 18)])
def test_record_spanning_17_windows(P, before, windows):
    """One 65535-byte packet between small ones: its 65551-byte record has bytes in 17 windows, or in
    18 when it starts in a window's last 14 bytes (it then covers 17 window starts)."""
    c = random_batch([10, 3, before, 65535, 20, 0, 7], 40)
    want, w_off, w_len, _ = run(P, c, room=(0, 1, 4096), label="65535")
    lo, hi = int(w_off[3]) - 16, int(w_off[3]) + 65535
    assert (hi - 1) // 4096 - lo // 4096 + 1 == windows


def test_many_short_records(P):
    """70 000 packets of 0-3 bytes: a 16-byte chunk holds pieces of two records' headers and a
    record's data between them, a 4 KiB window some 230 records (and up to 256 of the empty ones)."""
    rng = np.random.default_rng(50)
    lens = rng.integers(0, 4, 70000)
    lens[20000:20600] = 0  # whole windows of 16-byte records
    run(P, random_batch([int(x) for x in lens], 51), label="short records")


def test_sparse_selection(P):
    n = 1 << 16
    sel = (np.arange(n) % 1000 == 0)
    sel[10000:50000] = False  # 40 000 consecutive unselected packets
    c = C.case(gen.gen_c2(n, seed=60), stride=64, select=sel, ts=(5, 6))
    want, _, _, w_src = run(P, c, room=(0, 4096), label="sparse")
    assert np.array_equal(w_src, np.flatnonzero(sel)) and len(want) == 24 + 80 * int(sel.sum())


def assert_oracle(res, ref, n, label):
    for k, ov in ref.items():
        gv = res[k].cpu().numpy()
        if k in ("hdr_type", "hdr_off"):
            valid = np.arange(schema.MAX_HDRS)[:, None] < ref["n_hdrs"].astype(np.int64)[None, :]
            assert not (valid & (gv[:, :n] != ov)).any(), (label, k)
        else:
            assert np.array_equal(gv[:n], ov), (label, k)


def test_c4_capture_reproduced(P):
    """An indexed batch over a C4 capture, all selected, with the capture's own times: the capture
    again, which then parses as the oracle parses the input."""
    n = 20000
    buf, offs, lens = gen.gen_c4(n, seed=81)
    c = C.case(buf, offs, lens, ts=(0, 0))
    a = dev_args(c)
    cap, m, o, l, src = P.pcap_write(**a)
    assert m == n and cap.cpu().numpy().tobytes() == buf.tobytes()
    assert np.array_equal(o.cpu().numpy(), offs) and np.array_equal(l.cpu().numpy(), lens)
    m2, res, o2, l2 = P.parse_pcap(cap.clone(), n)
    assert m2 == n and np.array_equal(o2.cpu().numpy(), offs)
    assert_oracle(res, oracle.parse_batch(buf, n, offsets=offs, lens=lens, nthreads=8), n, "c4")


def test_filter_pipeline(P):
    """Parse, keep the TCP packets (a predicate on a parsed column, built on the device), save, and
    parse what was saved: the oracle's columns of the selected source packets, by src_index."""
    import torch
    n = 30000
    c3 = gen.gen_c3(n, seed=82)
    slab = dev(c3.reshape(-1))
    res = P.parse(slab, stride=128, columns=["chain"])
    select = ((res["hdr_mask"].view(torch.int32) >> schema.HDR_ID["TCP"]) & 1).to(torch.uint8)
    cap, m, o, l, src = P.pcap_write(slab, stride=128, select=select, ts=(11, 12))
    ref_all = oracle.parse_batch(c3, n, stride=128, nthreads=8)
    keep = np.flatnonzero((ref_all["hdr_mask"] >> schema.HDR_ID["TCP"]) & 1)
    assert 0 < keep.size < n and m == keep.size and np.array_equal(src.cpu().numpy(), keep)
    assert cap.cpu().numpy().tobytes() == C.expect(C.case(c3, stride=128, select=select.cpu().numpy(), ts=(11, 12)))[0]
    m2, res2, o2, l2 = P.parse_pcap(cap.clone(), m)
    assert m2 == m and np.array_equal(o2.cpu().numpy(), o.cpu().numpy())
    sub = np.ascontiguousarray(c3[src.cpu().numpy().astype(np.int64)])
    assert_oracle(res2, oracle.parse_batch(sub, m, stride=128, nthreads=8), m, "filter")


def test_pktgen_pipeline(P):
    """pkt_gen_run's packets written straight out: gen.pcap_bytes of the same packets as the host
    model of test_pktgen.py builds them."""
    import torch
    from pktgpu import pktgen
    import pktgen_templates as T
    name, n, first = "udp", 10000, 77
    tpl = T.template_bytes(name)
    gf, values, host_vals, csum, build = T.make_case(name, n, first)
    G = pktgen.Generator(P, tpl, gf, csum=csum)
    stride = G.default_stride()
    slab = G.run(n, stride, values={j: torch.from_numpy(v).cuda() for j, v in values.items()}, first=first)
    lens = dev(np.full(n, len(tpl), np.uint32))
    cap, m, o, l, src = P.pcap_write(slab.reshape(-1), lens=lens, stride=stride, ts=(21, 22))
    model = T.oracle_batch(tpl, n, stride, [(f.hdr, f.occurrence, f.start, f.end) for f in gf], host_vals, csum)
    want = gen.pcap_bytes([model[i, :len(tpl)].tobytes() for i in range(n)], 21, 22)
    assert m == n and cap.cpu().numpy().tobytes() == want


def test_async_two_ctx(P):
    """Two writes queued on two ctxs and two streams, then both results; a second write on a ctx
    before its result is taken raises, and so does a result with nothing queued."""
    import torch
    import pktgpu
    P2 = pktgpu.Parser(0)
    try:
        cs = [C.edges(per_packet_ts=True), C.select_case("every_third")]
        wants = [C.expect(c) for c in cs]
        ps, ss, bufs = [P, P2], [torch.cuda.Stream(), torch.cuda.Stream()], []
        for j in (0, 1):
            a = dev_args(cs[j])
            bufs.append(torch.full((len(wants[j][0]) + 64,), 0xA5, dtype=torch.uint8, device="cuda"))
            ss[j].wait_stream(torch.cuda.current_stream())
            ps[j].pcap_write_async(dst=bufs[j][:len(wants[j][0]) + 7], stream=ss[j], **a)
        with pytest.raises(RuntimeError):
            P.pcap_write_async(dst=bufs[0], stream=ss[0], **dev_args(cs[0]))
        with pytest.raises(RuntimeError):
            P.pcap_write(dst=bufs[0], **dev_args(cs[0]))
        for j in (1, 0):
            cap, n, offs, lens, src = ps[j].pcap_write_result()
            want, w_off, w_len, w_src = wants[j]
            got = bufs[j].cpu().numpy()
            assert n == len(w_src) and cap.numel() == len(want)
            assert got[:len(want)].tobytes() == want and (got[len(want):] == 0xA5).all()
            assert np.array_equal(offs.cpu().numpy(), w_off) and np.array_equal(src.cpu().numpy(), w_src)
            assert np.array_equal(lens.cpu().numpy(), w_len)
        with pytest.raises(RuntimeError):
            P.pcap_write_result()
        # a queued write that does not fit reports the size at its result
        P.pcap_write_async(dst=bufs[0][:100], **dev_args(cs[0]))
        with pytest.raises(RuntimeError, match=str(len(wants[0][0]))):
            P.pcap_write_result()
        assert (bufs[0].cpu().numpy()[len(wants[0][0]):] == 0xA5).all()
    finally:
        P2.close()
