"""pkt_l4_checksum_batch on the device (Parser.l4_checksum): the TCP / UDP / ICMP checksum of every packet of
a batch in HBM by pktgpu_l4csum.hip.  Expected values come from l4_cases.expect (an independent pure-Python
RFC 1071 loop) and, beside it, from the host twin; the 2^16-packet shape is checked against the host twin
alone.  Every slab lies between two guard regions filled with 0xA5: a kernel that summed past slab_len
would sum 0xA5 bytes and show it in the results, and an UPDATE that stored outside a checksum field would
show in the guards or in the byte comparison with the expected slab."""
import ctypes

import numpy as np
import pytest

from pktgpu import gen, schema

import compare_cases as C
import edit_cases as E
import l4_cases as L4

pytestmark = pytest.mark.gpu
GUARD = 4096


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
    """The batch on the device, its slab a slice of a larger 0xA5-filled allocation: GUARD bytes before it
    and at least GUARD after it.  Returns (keyword arguments of l4_checksum, the whole allocation)."""
    import torch
    size = b["slab"].size
    big = torch.full((GUARD + (size + 15) // 16 * 16 + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    big[GUARD:GUARD + size] = dev(b["slab"])
    kw = dict(slab=big[GUARD:GUARD + size], n=b["n"], stride=b["stride"],
              offsets=None if b["offsets"] is None else dev(b["offsets"]), lens=None if b["lens"] is None else dev(b["lens"]))
    return kw, big


def guards_intact(big, size):
    return bool((big[:GUARD] == 0xA5).all()) and bool((big[GUARD + size:] == 0xA5).all())


def host(got):
    return {k: None if v is None else v.cpu().numpy() for k, v in got.items()}


def host_twin(c, update=False, keep=False, slab=None):
    import pktgpu
    b = c["batch"]
    return pktgpu.l4_checksum(b["slab"] if slab is None else slab, c["chain"], c["which"], update, keep,
                              stride=b["stride"], n=b["n"], offsets=b["offsets"], lens=b["lens"])


@pytest.mark.parametrize("name", L4.CASE_NAMES)
def test_cases(P, name):
    """Read-only, against the yardstick and the host twin; the slab is left as it was."""
    c, want, _, _ = L4.all_cases()[name]
    kw, big = dev_batch(c["batch"])
    got = host(P.l4_checksum(chain={k: dev(v) for k, v in c["chain"].items()}, which=c["which"], **kw))
    L4.check(got, want, name)
    L4.check(got, host_twin(c), name + " (host twin)")
    size = c["batch"]["slab"].size
    assert guards_intact(big, size) and np.array_equal(big[GUARD:GUARD + size].cpu().numpy(), c["batch"]["slab"])


@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("name", L4.CASE_NAMES)
def test_update(P, name, keep):
    """UPDATE on a cloned slab: byte-equal to the yardstick's and to the host twin's updated slab, guards
    untouched, the outputs describing the fields as they were read."""
    c, want, upd, kp = L4.all_cases()[name]
    kw, big = dev_batch(c["batch"])
    got = host(P.l4_checksum(chain={k: dev(v) for k, v in c["chain"].items()}, which=c["which"], update=True,
                             keep_zero_udp=keep, **kw))
    L4.check(got, want, name)
    size = c["batch"]["slab"].size
    after = big[GUARD:GUARD + size].cpu().numpy()
    exp = (kp if keep else upd)["slab"]
    assert np.array_equal(after, exp), np.flatnonzero(after != exp)[:8]
    twin = c["batch"]["slab"].copy()
    host_twin(c, True, keep, twin)
    assert np.array_equal(after, twin)
    assert guards_intact(big, size)


def test_null_outputs_and_refusals(P):
    L, s = P._L, P._stream(None)
    for name in ("mixed_1000", "c2_stride64_1000"):
        c, want, _, _ = L4.all_cases()[name]
        kw, big = dev_batch(c["batch"])
        chain = {k: dev(v) for k, v in c["chain"].items()}
        for outputs in ((False, True, True), (True, False, True), (True, True, False), (False, False, False)):
            args, out, keep = P._l4_args(chain=chain, which=c["which"], outputs=outputs, **kw)
            assert L.pkt_l4_checksum_batch(P._ctx, *args, s) == 0
            L4.check(host(dict(calc=out[0], stored=out[1], status=out[2])), want, f"{name} {outputs}")
    args, out, keep = P._l4_args(chain=chain, which=0, **kw)
    lib = P._lib

    def call(r=()):
        a = list(args)
        for k, v in dict(r).items():  # argument position (after ctx) -> value
            a[k] = v
        return L.pkt_l4_checksum_batch(P._ctx, *a, s)
    import torch
    for t in out:
        t.view(torch.uint8).fill_(0x77)
    huge = P._batch(kw["slab"], 1 << 32, 64, None, None)
    odd = P._batch(kw["slab"][1:], None, 64, None, None)
    no_lens = lib.PktBatch()
    four = dev(np.zeros(4, np.uint64))
    no_lens.slab, no_lens.slab_len, no_lens.offsets, no_lens.n = keep[0].slab, keep[0].slab_len, four.data_ptr(), 4
    no_col = lib.PktChain(keep[1].n_hdrs, None, keep[1].hdr_off)
    bad = [{0: None}, {1: None}, {1: ctypes.byref(no_col)}, {0: ctypes.byref(huge)}, {0: ctypes.byref(odd)},
           {0: ctypes.byref(no_lens)}, {2: 16}, {2: 0xFE}, {3: 4}, {3: 0x80000001}, {3: schema.L4_KEEP_ZERO_UDP}]
    for r in bad:
        assert call(r) == -1, sorted(r)
    torch.cuda.synchronize()
    assert all(bool((t.view(torch.uint8) == 0x77).all()) for t in out)  # every refusal came before any launch
    empty = P._batch(kw["slab"], 0, 64, None, None)
    assert call({0: ctypes.byref(empty)}) == 0                        # n == 0 succeeds and launches nothing
    torch.cuda.synchronize()
    assert all(bool((t.view(torch.uint8) == 0x77).all()) for t in out)
    with pytest.raises(RuntimeError):
        P.l4_checksum(kw["slab"], chain, which=16, stride=64)
    assert call({2: 15}) == 0 and call({2: 0xFF}) == 0 and call() == 0
    L4.check(host(dict(calc=out[0], stored=out[1], status=out[2])), L4.all_cases()["c2_stride64_1000"][1], "after the errors")


def verify_all_ok(P, slab, chain, which=0, **kw):
    st = P.l4_checksum(slab, chain, which=which, **kw)["status"].cpu().numpy()
    assert (st == L4.OK).all(), (np.flatnonzero(st != L4.OK)[:8], st[st != L4.OK][:8])


def yardstick_sample(slab, stride, length, k, which=L4.LAST):
    """The first k packets of a fixed-stride device slab through the yardstick: their statuses."""
    a = slab[:k * stride].cpu().numpy().reshape(k, stride)
    return [L4.one(a[i, :length].tobytes(), L4.hdrs_of(a[i, :length].tobytes()), which)[0] for i in range(k)]


def test_flow_generate_then_update_then_nat(P):
    """(1) pkt_gen_run of a TCP template with random ports and addresses -> parse -> UPDATE -> all OK.
    (2) NAT on the result: pkt_set_fields_csum on ipv4_src and tcp_src with the IPv4 refresh leaves the TCP
    checksum stale (BAD); UPDATE makes every packet OK again."""
    from pktgpu import pktgen
    n = 3000
    tpl = pktgen.test_tcp_template()
    G = pktgen.Generator(P, tpl, [pktgen.Field("TCP", "src", kind="random", base=1), pktgen.Field("TCP", "dst", kind="random", base=2),
                                  pktgen.Field("IPv4", "src", kind="random", base=3)], csum=[0])
    stride = G.default_stride()                                         # 160: six zero bytes pad every slot
    slab = G.run(n, stride)
    chain = P.parse(slab, stride=stride, columns=["chain"])
    first = P.l4_checksum(slab, chain, stride=stride)
    assert (first["stored"].cpu().numpy() == 0).all() and (first["status"].cpu().numpy() == L4.BAD).sum() > n - 3
    before = slab.clone()
    P.l4_checksum(slab, chain, update=True, stride=stride)
    verify_all_ok(P, slab, chain, stride=stride)
    assert yardstick_sample(slab, stride, len(tpl), 64) == [L4.OK] * 64
    changed = (slab != before).view(n, stride).any(dim=0).cpu().numpy()
    assert set(np.flatnonzero(changed)) <= {50, 51}                     # the TCP checksum field alone
    # (2)
    rng = np.random.default_rng(5)
    vals = [dev(rng.integers(0, 1 << 32, n, dtype=np.uint64)), dev(rng.integers(1, 1 << 16, n, dtype=np.uint64))]
    P.set_fields(slab, chain, [C.spec("IPv4", "src"), C.spec("TCP", "src")], vals, stride=stride, ipv4_checksum=0)
    stale = P.l4_checksum(slab, chain, stride=stride)["status"].cpu().numpy()
    assert (stale == L4.BAD).sum() > n - 3
    P.l4_checksum(slab, chain, update=True, stride=stride)
    verify_all_ok(P, slab, chain, stride=stride)
    assert yardstick_sample(slab, stride, len(tpl), 64) == [L4.OK] * 64
    ip = P.parse(slab, stride=stride, columns=["ipv4_header_checksum", "ipv4_csum_calc"])
    assert np.array_equal(ip["ipv4_header_checksum"].cpu().numpy(), ip["ipv4_csum_calc"].cpu().numpy())
    G.close()


def test_flow_vxlan_encap_outer_udp(P):
    """(3) pkt_edit_batch VXLAN encap with out_chain -> pkt_set_fields_csum for the two lengths -> UPDATE with
    which = 0: the outer UDP is OK; a verify with LAST shows the inner TCP still OK and untouched."""
    import torch
    rng = np.random.default_rng(92)
    n = 200
    inner, outer = [], None
    for i in range(n):
        p = gen.test_tcp_packet_with_payload(E.rnd_bytes(rng, int(rng.integers(0, 300))))
        inner.append(L4.finalize(bytes(p.to_vec())))
        if outer is None:
            outer = bytes(gen.create_vxlan_packet(E.M1, E.M2, False, 10, 3, 5, "192.168.0.199", "192.168.0.1", 0, 64, 0, 0x4000,
                                                  [], gen.VXLAN_PORT, 9090, False, 2000, p).to_vec())[:50]
    src, _ = dev_batch(C.indexed(inner, rng))
    parsed = P.parse(src["slab"], offsets=src["offsets"], lens=src["lens"], columns=["chain"])
    verify_all_ok(P, src["slab"], parsed, offsets=src["offsets"], lens=src["lens"])
    dst, ln, st, ch = P.edit(src["slab"], parsed, E.encap_ops(outer), offsets=src["offsets"], lens=src["lens"], slot=512)
    assert (st.cpu().numpy() == E.OK).all()
    total = ln.to(torch.int64)
    vals = [(total - 14).view(torch.uint64), (total - 34).view(torch.uint64)]
    P.set_fields(dst, ch, [C.spec("IPv4", "total_len"), C.spec("UDP", "length")], vals, stride=512, lens=ln, ipv4_checksum=0)
    assert (P.l4_checksum(dst, ch, which=0, stride=512, lens=ln)["status"].cpu().numpy() == L4.UNCHECKED).all()
    before = dst.clone()
    got = P.l4_checksum(dst, ch, which=0, update=True, stride=512, lens=ln)
    verify_all_ok(P, dst, ch, which=0, stride=512, lens=ln)
    verify_all_ok(P, dst, ch, which=L4.LAST, stride=512, lens=ln)
    verify_all_ok(P, dst, ch, which=1, stride=512, lens=ln)
    changed = (dst != before).view(n, 512).any(dim=0).cpu().numpy()
    assert set(np.flatnonzero(changed)) <= {40, 41}                     # the outer UDP checksum alone
    # against the yardstick, packet by packet, with a parse of the bytes by the Python model
    d, lens = dst.cpu().numpy(), ln.cpu().numpy()
    calc = got["calc"].cpu().numpy()
    for i in range(n):
        p = d[512 * i:512 * i + int(lens[i])].tobytes()
        hd = L4.hdrs_of(p)
        assert L4.one(p, hd, 0)[:2] == (L4.OK, int(calc[i])) and L4.one(p, hd, L4.LAST)[0] == L4.OK, i


def test_pcap_stream_window(P):
    """The window of a PcapStream.batch() with the stream's device columns as the chain: no copy and no
    second parse."""
    from pktgpu.stream import PcapStream
    c, want, _, _ = L4.all_cases()["mixed_1000"]
    pk = C.packets(c["batch"])
    st = PcapStream(0, max_bytes=1 << 22, cap=len(pk), columns=["chain"])
    try:
        st.push(gen.pcap_bytes(pk))
        n, _ = st.finish()
        assert n == len(pk)
        slab, offs, lens = st.batch()
        got = host(P.l4_checksum(slab, st.out, which=L4.LAST, offsets=offs, lens=lens))
        L4.check(got, want, "stream window")
    finally:
        st.close()


def test_mixed_c4_65536_against_the_host_twin(P):
    """2^16 packets of C4 traffic (the 22 reference templates in a capture, an indexed batch over it in
    place): enough to cross block and grid boundaries.  Read-only and UPDATE against the host twin."""
    import pktgpu
    n = 1 << 16
    buf, offs, lens = gen.gen_c4(n, seed=44)
    b = C.batch(buf, offs, lens)
    kw, big = dev_batch(b)
    chain = P.parse(kw["slab"], offsets=kw["offsets"], lens=kw["lens"], columns=["chain"])
    hchain = {k: chain[k].cpu().numpy() for k in ("n_hdrs", "hdr_type", "hdr_off")}
    for which in (0, L4.LAST):
        got = host(P.l4_checksum(kw["slab"], chain, which=which, offsets=kw["offsets"], lens=kw["lens"]))
        twin = pktgpu.l4_checksum(buf, hchain, which, offsets=offs, lens=lens)
        L4.check(got, twin, f"c4 which={which}")
        assert len(set(twin["status"].tolist())) >= 3
    P.l4_checksum(kw["slab"], chain, which=L4.LAST, update=True, offsets=kw["offsets"], lens=kw["lens"])
    twin_slab = buf.copy()
    pktgpu.l4_checksum(twin_slab, hchain, L4.LAST, True, offsets=offs, lens=lens)
    assert np.array_equal(big[GUARD:GUARD + buf.size].cpu().numpy(), twin_slab) and guards_intact(big, buf.size)
    again = P.l4_checksum(kw["slab"], chain, which=L4.LAST, offsets=kw["offsets"], lens=kw["lens"])["status"].cpu().numpy()
    assert (again[twin["status"] <= L4.UNCHECKED] == L4.OK).all()
