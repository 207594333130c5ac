"""pkt_compare_batch on the device (Parser.compare): Packet::compare (packet.rs:326-358) of two batches
in HBM by pktgpu_compare.hip.  Every expected value comes from compare_cases.expect (numpy, from the
definition) or is known by construction, never from pkt_compare_host or the device.  Every slab is a
slice of a larger 0xA5-filled allocation, so a kernel that did not clamp to slab_len would compare
0xA5 bytes and show it in the results, not in a fault."""
import os

import numpy as np
import pytest

from pktgpu import gen

import compare_cases as C
from compare_cases import check

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


def dev_batch(b):
    import torch
    big = torch.full(((b["slab"].size + 15) // 16 * 16 + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
    big[:b["slab"].size] = dev(b["slab"])
    d = dict(slab=big[:b["slab"].size], n=b["n"], stride=b["stride"])
    if b["offsets"] is not None:
        d["offsets"] = dev(b["offsets"])
    if b["lens"] is not None:
        d["lens"] = dev(b["lens"])
    return d


def dev_chain(ch):
    return None if ch is None else {k: dev(v) for k, v in ch.items()}


def host(got):
    return tuple(t.cpu().numpy() for t in got[:3]) + (got[3],)


def run(P, c):
    return host(P.compare(dev_batch(c["a"]), dev_batch(c["b"]), c["ignore"], dev_chain(c["chain"])))


@pytest.mark.parametrize("name", C.CASE_NAMES)
def test_cases(P, name):
    c, want = C.all_cases()[name]
    check(run(P, c), want, name)


def test_alignment(P):
    c, (res, mt, fd) = C.alignment()
    got = run(P, c)
    check(got, (res, mt, fd, None), "alignment")
    n = c["a"]["n"]
    assert got[3] == dict(n_equal=int((res == 0).sum()), n_len=0, n_bytes=int((res == 2).sum()),
                          first_bad=int(np.flatnonzero(res)[0]))
    assert n == 256 * (sum(C.ALIGN_LENS) + len(C.ALIGN_LENS))


def test_ignores_with_the_device_parse(P):
    """The ignore cases again with the chain columns of Parser.parse of `a`, not the Python model's."""
    for name in ("straddle", "ipv6_src", "absent_header", "sixteen"):
        c, want = C.all_cases()[name]
        a = dev_batch(c["a"])
        chain = P.parse(a["slab"], offsets=a["offsets"], lens=a["lens"], columns=["chain"])
        assert np.array_equal(chain["n_hdrs"].cpu().numpy(), c["chain"]["n_hdrs"])
        check(host(P.compare(a, dev_batch(c["b"]), c["ignore"], chain)), want, name)


def test_null_outputs_and_argument_errors(P):
    import ctypes
    c, want = C.all_cases()["tiling_1025"]
    a, b = dev_batch(c["a"]), dev_batch(c["b"])
    args, out, keep = P._compare_args(a, b, (), None, outputs=False)
    sm = P._lib.PktCmpSummary()
    assert P._L.pkt_compare_batch(P._ctx, *args, ctypes.byref(sm), P._stream(None)) == 0
    assert dict(n_equal=sm.n_equal, n_len=sm.n_len, n_bytes=sm.n_bytes, first_bad=sm.first_bad) == want[3]
    assert P._L.pkt_compare_batch(P._ctx, *args, None, P._stream(None)) == 0
    huge = P._batch(a["slab"], 1 << 32, 64, None, None)               # n >= 2^32: refused before any launch
    assert P._L.pkt_compare_batch(P._ctx, ctypes.byref(huge), ctypes.byref(huge), None, None, 0, None, None, None,
                                  None, P._stream(None)) != 0
    ch = dev_chain(C.chain_of(c["a"]))
    with pytest.raises(RuntimeError):
        P.compare(a, dict(b, n=1024))                                # a->n != b->n
    with pytest.raises(ValueError):
        P.compare(a, b, [("IPv4", 0, 64, 71)])                       # ignores without a chain
    with pytest.raises(RuntimeError):
        P.compare(a, b, [("IPv4", 0, 64, 63)], ch)                   # end < start
    with pytest.raises(RuntimeError):
        P.compare(a, b, [("IPv4", 0, 64, 71)] * 17, ch)              # more than 16
    check(host(P.compare(a, b)), want, "after the errors")


def test_summary_async_and_two_ctx(P):
    """Two compares queued on two ctxs and two streams, then both results; a second compare on a ctx
    before its result is taken raises, and so does a result with nothing queued."""
    import torch
    import pktgpu
    P2 = pktgpu.Parser(0)
    try:
        names = ["tiling_4099", "sixteen"]
        ps, ss = [P, P2], [torch.cuda.Stream(), torch.cuda.Stream()]
        for j in (0, 1):
            c = C.all_cases()[names[j]][0]
            ss[j].wait_stream(torch.cuda.current_stream())
            ps[j].compare_async(dev_batch(c["a"]), dev_batch(c["b"]), c["ignore"], dev_chain(c["chain"]), stream=ss[j])
        c0 = C.all_cases()[names[0]][0]
        with pytest.raises(RuntimeError):
            P.compare_async(dev_batch(c0["a"]), dev_batch(c0["b"]), stream=ss[0])
        with pytest.raises(RuntimeError):
            P.compare(dev_batch(c0["a"]), dev_batch(c0["b"]))
        for j in (1, 0):
            check(host(ps[j].compare_result()), C.all_cases()[names[j]][1], names[j])
        with pytest.raises(RuntimeError):
            P.compare_result()
        # n = 0 queued: an all-zero summary
        e = C.all_cases()["empty_batch"][0]
        P.compare_async(dev_batch(e["a"]), dev_batch(e["b"]))
        assert P.compare_result()[3] == dict(n_equal=0, n_len=0, n_bytes=0, first_bad=0)
        # the words are at rest again: the same compare twice gives the same summary
        for _ in range(2):
            check(run(P, c0), C.all_cases()[names[0]][1], "again")
    finally:
        P2.close()


def test_ref22_to_vec_round_trip(P):
    """tests/lib.rs:674-679, `slow::parse(bytes).compare(pkt)` for the 22 packets: the capture parsed,
    to_vec'd and compared with itself is all EQUAL."""
    pc = np.frombuffer(open(os.path.join(C.GOLD, "ref22.pcap"), "rb").read(), np.uint8)
    offs, lens = gen.pcap_index_py(pc.tobytes())
    b = dev_batch(C.batch(pc, offs, lens))
    parsed = P.parse(b["slab"], offsets=b["offsets"], lens=b["lens"])
    dst, out_len = P.to_vec(b["slab"], parsed, offsets=b["offsets"], lens=b["lens"])
    assert np.array_equal(out_len.cpu().numpy(), lens)
    res, mt, fd, sm = host(P.compare(dict(slab=dst, offsets=b["offsets"], lens=out_len), b))
    assert sm == dict(n_equal=22, n_len=0, n_bytes=0, first_bad=22)
    assert (res == 0).all() and np.array_equal(mt, lens) and np.array_equal(fd, lens)
    pk = [bytes(p.to_vec()) for p in gen.reference_22_packets()]
    built = dev_batch(C.indexed(pk, np.random.default_rng(1)))
    assert P.compare(built, b)[3]["n_equal"] == 22


def test_generate_write_index_compare(P):
    """pkt_gen_run -> pcap_write -> pcap_index -> compare (fixed stride against the indexed capture): all
    EQUAL.  After set_fields of ipv4.ttl (with the checksum refresh) on every third packet exactly those
    are BYTES with first_diff at the ttl byte; with ttl and header_checksum ignored all are EQUAL again."""
    import torch
    from pktgpu import pktgen
    import pktgen_templates as T
    name, n, first = "udp", 5000, 77
    tpl = T.template_bytes(name)
    gf, values, host_vals, csum, build = T.make_case(name, n, first)
    G = pktgen.Generator(P, tpl, gf, csum=csum)
    stride = G.default_stride()
    slab = G.run(n, stride, values={j: torch.from_numpy(v).cuda() for j, v in values.items()}, first=first).reshape(-1)
    lens = dev(np.full(n, len(tpl), np.uint32))
    cap, m, o, l, src = P.pcap_write(slab, lens=lens, stride=stride)
    offs, rlens, cnt = P.pcap_index(cap)
    assert m == n == cnt
    a, b = dict(slab=slab, stride=stride, lens=lens), dict(slab=cap, offsets=offs, lens=rlens)
    res, mt, fd, sm = host(P.compare(a, b))
    assert sm == dict(n_equal=n, n_len=0, n_bytes=0, first_bad=n) and (mt == len(tpl)).all() and (fd == len(tpl)).all()
    chain = P.parse(slab, stride=stride, lens=lens, columns=["chain"])
    ttl_spec, csum_spec = C.spec("IPv4", "ttl"), C.spec("IPv4", "header_checksum")
    ttl = P.extract_fields(slab, chain, [ttl_spec], stride=stride, lens=lens)[0][0].cpu().numpy()
    third = np.arange(n) % 3 == 0
    new = np.where(third, (ttl + 1) & 0xFF, ttl).astype(np.uint64)
    P.set_fields(slab, chain, [ttl_spec], [dev(new)], stride=stride, lens=lens, ipv4_checksum=0)
    res, mt, fd, sm = host(P.compare(a, b))
    assert np.array_equal(res, np.where(third, C.BYTES, C.EQUAL))
    assert (fd[third] == 14 + 8).all() and (fd[~third] == len(tpl)).all()
    assert sm == dict(n_equal=int((~third).sum()), n_len=0, n_bytes=int(third.sum()), first_bad=0)
    want = C.expect(C.case(C.batch(slab.cpu().numpy(), lens=lens.cpu().numpy(), stride=stride, n=n),
                           C.batch(cap.cpu().numpy(), offs.cpu().numpy(), rlens.cpu().numpy())))
    check((res, mt, fd, sm), want, "ttl changed")
    res, mt, fd, sm = host(P.compare(a, b, [ttl_spec, csum_spec], chain))
    assert sm == dict(n_equal=n, n_len=0, n_bytes=0, first_bad=n) and (mt == len(tpl)).all()
