"""pkt_edit_batch on the device (Parser.edit): Packet::push / insert / pop / remove (packet.rs:117-164) and
to_vec over a batch in HBM by pktgpu_edit.hip.  Every expected value comes from edit_cases.expect
(pyref.parse and plain Python list operations) or from the reference's own 22 packets, never from
pkt_edit_host or the device.  Every source slab is a slice of a larger 0xA5-filled allocation, so a
kernel that did not clamp to slab_len would copy 0xA5 bytes and show it in the results, not in a fault;
every destination is pre-filled with 0x5A and must keep it outside the packets written."""
import ctypes
import os

import numpy as np
import pytest

from pktgpu import gen, schema

import compare_cases as C
import edit_cases as E

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
    """The batch on the device, its slab a slice of a larger 0xA5-filled allocation."""
    import torch
    big = torch.full(((b["slab"].size + 15) // 16 * 16 + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
    big[:b["slab"].size] = dev(b["slab"])
    return dict(slab=big[:b["slab"].size], n=b["n"], stride=b["stride"],
                offsets=None if b["offsets"] is None else dev(b["offsets"]), lens=None if b["lens"] is None else dev(b["lens"]))


def args_of(c, parsed, b=None):
    import torch
    b = dev_batch(c["src"]) if b is None else b
    dst = torch.full((c["dst_len"],), E.FILL, dtype=torch.uint8, device="cuda")
    return dict(slab=b["slab"], parsed={k: dev(v) for k, v in parsed.items()} if isinstance(parsed["status"], np.ndarray) else parsed,
                ops=c["ops"], stride=b["stride"], n=b["n"], offsets=b["offsets"], lens=b["lens"],
                select=None if c["select"] is None else dev(c["select"]), dst=dst,
                dst_offsets=None if c["dst_offsets"] is None else dev(c["dst_offsets"]), slot=c["slot"])


def host(got):
    dst, ln, st, ch = got
    cpu = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
    return cpu(dst), cpu(ln), cpu(st), None if ch is None else {k: v.cpu().numpy() for k, v in ch.items()}


@pytest.mark.parametrize("name", E.CASE_NAMES)
def test_cases(P, name):
    c, parsed, want = E.get(name)
    E.check(c, host(P.edit(**args_of(c, parsed))), want, name)


def test_cases_with_the_device_parse(P):
    """Cases again with the chain columns of Parser.parse of the source, not the Python model's."""
    for name in ("c3_1025_strip0", "mixed_eight", "mixed_absent", "depth_insert", "select"):
        c, parsed, want = E.get(name)
        b = dev_batch(c["src"])
        res = P.parse(b["slab"], stride=b["stride"], n=b["n"], offsets=b["offsets"], lens=b["lens"], columns=["chain"])
        assert np.array_equal(res["n_hdrs"].cpu().numpy(), parsed["n_hdrs"]), name
        E.check(c, host(P.edit(**args_of(c, res, b))), want, name)


def ref22(P):
    pc = np.frombuffer(open(os.path.join(C.GOLD, "ref22.pcap"), "rb").read(), np.uint8)
    offs, lens = gen.pcap_index_py(pc.tobytes())
    b = dev_batch(C.batch(pc, offs, lens))
    parsed = P.parse(b["slab"], offsets=b["offsets"], lens=b["lens"])
    return [pc[int(o):int(o) + int(ln)].tobytes() for o, ln in zip(offs, lens)], b, parsed


def edit_packets(P, b, parsed, ops, slot=512):
    dst, ln, st, ch = host(P.edit(b["slab"], parsed, ops, offsets=b["offsets"], lens=b["lens"], slot=slot))
    return [dst[slot * i:slot * i + int(ln[i])].tobytes() for i in range(b["n"])], ln, st, ch


def test_reference_identities(P):
    """The reference's own fixtures, the 22 packets of tests/golden/ref22.pcap (tests/lib.rs:454-461,
    utils.rs:504-550): decap, IP-in-IP, encap by inserts and by pushes, and nops = 0 against to_vec."""
    pk, b, parsed = ref22(P)
    assert pk == [bytes(p.to_vec()) for p in gen.reference_22_packets()]
    out = edit_packets(P, b, parsed, [("remove", 0)] * 4)[0]
    assert out[8] == pk[0] and out[6] == pk[1]
    assert edit_packets(P, b, parsed, [("remove", 0)] * 2)[0][12] == edit_packets(P, b, parsed, [("remove", 0)])[0][0] == pk[0][14:]
    out, ln, st, ch = edit_packets(P, b, parsed, E.encap_ops(pk[8][:50]))
    assert out[0] == pk[8] and ln[0] == len(pk[8]) and (st == E.OK).all()
    o = pk[8][:50]
    pushes = [("pop",)] * 4 + [("push", "Ether", o[0:14]), ("push", "IPv4", o[14:34]), ("push", "UDP", o[34:42]),
                               ("push", "Vxlan", o[42:50])]
    assert edit_packets(P, b, parsed, pushes)[0][0] == o + pk[0][54:]
    # identity: pkt_to_vec_batch's bytes and the parse's chain columns
    import torch
    slot = 512
    offs = torch.arange(22, dtype=torch.int64, device="cuda").mul_(slot).view(torch.uint64)
    tv = torch.zeros(22 * slot, dtype=torch.uint8, device="cuda")
    tv, tv_len = P.to_vec(b["slab"], parsed, offsets=b["offsets"], lens=b["lens"], dst=tv, dst_offsets=offs)
    out, ln, st, ch = edit_packets(P, b, parsed, [], slot)
    tv, tv_len = tv.cpu().numpy(), tv_len.cpu().numpy()
    assert np.array_equal(ln, tv_len) and (st == E.OK).all()
    assert out == [tv[slot * i:slot * i + int(tv_len[i])].tobytes() for i in range(22)] == pk
    for k in ("status", "n_hdrs", "payload_off", "payload_len", "hdr_mask"):
        assert np.array_equal(ch[k], parsed[k].cpu().numpy()), k
    used = np.arange(schema.MAX_HDRS)[:, None] < ch["n_hdrs"][None, :]
    for k in ("hdr_type", "hdr_off"):
        assert np.array_equal(ch[k][used], parsed[k].cpu().numpy()[used]), k


def test_null_outputs_and_argument_errors(P):
    c, parsed, want = E.get("c3_1025_remove1")
    L, s = P._L, P._stream(None)
    for outputs in ((False, True, True), (True, False, True), (True, True, False), (False, False, False)):
        kw = args_of(c, parsed)
        args, out, keep = P._edit_args(**kw, outputs=outputs)
        assert L.pkt_edit_batch(P._ctx, *args, s) == 0
        E.check(c, host(out), want, str(outputs))
    kw = args_of(c, parsed)
    args, out, keep = P._edit_args(**kw)
    lib = P._lib
    ins = (lib.PktEditOp * 1)(lib.PktEditOp(3, E.hid("MPLS"), 0, 0, 0))

    def call(r=()):
        a = list(args)
        for k, v in dict(r).items():  # argument position (after ctx) -> value
            a[k] = v
        return L.pkt_edit_batch(P._ctx, *a, s)
    huge = P._batch(kw["slab"], 1 << 32, 128, None, None)
    nine = (lib.PktEditOp * 9)()
    no_status = lib.PktOut()
    no_status.n_hdrs, no_status.hdr_type = keep[1].n_hdrs, keep[1].hdr_type
    bad = [{2: nine, 3: 9},                                                            # nops > 8
           {2: (lib.PktEditOp * 1)(lib.PktEditOp(4, 0, 0, 0, 0))},                     # an unknown kind
           {2: (lib.PktEditOp * 1)(lib.PktEditOp(3, 22, 0, 0, 0)), 4: bytes(64), 5: 64},  # an INSERT of type 22
           {2: ins, 4: bytes(8), 5: 3}, {2: ins, 4: None, 5: 0},                       # bytes past hdr_data_len
           {2: ins, 4: bytes(400), 5: 321},                                            # hdr_data_len > 320
           {10: 0}, {0: ctypes.byref(huge)},                                           # slot 0, n >= 2^32
           {7: None}, {1: ctypes.byref(no_status)}, {2: None}, {0: None}, {1: None}]   # NULL required pointers
    for r in bad:
        assert call(r) == -1, sorted(r)
    import torch
    torch.cuda.synchronize()
    assert (out[0] == E.FILL).all()                                   # every error came before any launch
    with pytest.raises(RuntimeError):
        P.edit(kw["slab"], kw["parsed"], [("pop",)] * 9, stride=128)
    # n == 0 succeeds and does nothing
    e = P._batch(kw["slab"], 0, 128, None, None)
    a = list(args)
    a[0] = ctypes.byref(e)
    assert L.pkt_edit_batch(P._ctx, *a, s) == 0
    assert call() == 0
    E.check(c, host(out), want, "after the errors")


def test_encap_set_fields_compare(P):
    """Encap, then set_fields with the checksum refresh on the out chain, against packets built by
    gen.create_vxlan_packet with per-packet inner payload lengths: all EQUAL."""
    rng = np.random.default_rng(91)
    n = 200
    inner, built = [], []
    for i in range(n):
        p = gen.test_tcp_packet_with_payload(E.rnd_bytes(rng, int(rng.integers(0, 300))))
        inner.append(bytes(p.to_vec()))
        v = gen.create_vxlan_packet(E.M1, E.M2, False, 10, 3, 5, "192.168.0.199", "192.168.0.1", 0, 64, 0, 0x4000, [],
                                    gen.VXLAN_PORT, 9090, False, 2000, p)
        v["IPv4"].set_bits(80, 95, gen.ipv4_checksum(bytes(v["IPv4"].data)))   # refreshed, as set_fields_csum leaves it
        built.append(bytes(v.to_vec()))
    src = dev_batch(C.indexed(inner, rng))
    parsed = P.parse(src["slab"], offsets=src["offsets"], lens=src["lens"], columns=["chain"])
    dst, ln, st, ch = P.edit(src["slab"], parsed, E.encap_ops(built[0][:50]), offsets=src["offsets"], lens=src["lens"], slot=512)
    assert (st.cpu().numpy() == E.OK).all()
    import torch
    total = ln.to(torch.int64)
    vals = [(total - 14).view(torch.uint64), (total - 34).view(torch.uint64)]
    P.set_fields(dst, ch, [C.spec("IPv4", "total_len"), C.spec("UDP", "length")], vals, stride=512, lens=ln, ipv4_checksum=0)
    res, mt, fd, sm = P.compare(dict(slab=dst, stride=512, lens=ln), dev_batch(C.indexed(built, rng)))
    assert sm == dict(n_equal=n, n_len=0, n_bytes=0, first_bad=n), (sm, fd.cpu().numpy()[:8])


def test_edit_pcap_write_index_parse(P):
    """Edit (decap), pcap_write, pcap_index, parse: the chain of the re-parsed output is the model's."""
    c, parsed, (outs, w_len, w_st, w_ch) = E.get("mixed_absent")
    kw = args_of(c, parsed)
    dst, ln, st, ch = P.edit(**kw)
    cap, m, o, l, srci = P.pcap_write(dst, offsets=kw["dst_offsets"], lens=ln, select=(st == 0))
    offs, rlens, cnt = P.pcap_index(cap)
    ok = np.flatnonzero(w_st == E.OK)
    assert cnt == m == ok.size and np.array_equal(srci.cpu().numpy(), ok)
    re = P.parse(cap, offsets=offs, lens=rlens, columns=["chain"])
    re = {k: v.cpu().numpy() for k, v in re.items()}
    capn, offs = cap.cpu().numpy(), offs.cpu().numpy()
    for k, i in enumerate(ok):
        v = outs[i]
        assert capn[int(offs[k]):int(offs[k]) + len(v)].tobytes() == v
        status, hdrs, po, pl = E.pyref.parse(v)
        assert re["status"][k] == E.STATUS_ID[status] and re["n_hdrs"][k] == len(hdrs)
        assert [(schema.HDR_NAMES[re["hdr_type"][j, k]], int(re["hdr_off"][j, k])) for j in range(len(hdrs))] == hdrs
        assert (re["payload_off"][k], re["payload_len"][k]) == (po, pl)
