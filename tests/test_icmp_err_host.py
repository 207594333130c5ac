"""pkt_icmp_err_host, the CPU twin of pkt_icmp_err_batch, against icmp_cases' yardstick (an independent Python model
written from include/pktgpu.h's rules) and against packets written out field by field from RFC 792 / 1191 / 4443.  The
twin runs the same inline code as the kernels (pktgpu_icmp.hpp): the find step, the decision, both header builders
and the refusals are covered here without a device.  (The refusals' texts need a ctx: test_icmp_err_device.py.)"""
import ctypes
import socket
import struct

import numpy as np
import pytest

import pktgpu
from pktgpu import schema

import icmp_cases as I
from l4_cases import pin_yardstick, rfc1071_sum

INVALID = -1
CF = I.cfg(ident=0xFFF0, ttl=200, tos=0xC0)


def run(items, code, cf=CF, mtu=0, cmap=None, select=None, which=0, kind="indexed", **kw):
    b, ch = I.layout(items, kind)
    want = I.expect(b, ch, code, cf, mtu, cmap, select, which)
    rc, got = I.host_call(b, ch, code, cf, mtu, cmap, select, which, **kw)
    assert rc == 0 and got["guards"]
    I.check(got, want, got["cap"])
    return got, want


def outputs(got):
    return [got["dst"][int(o):int(o) + int(ln)].tobytes() for o, ln in zip(got["out_off"][:got["n_out"]], got["out_len"])]


def test_the_yardsticks_checksum_is_rfc_1071():
    pin_yardstick()


# ------------------------------------------------------------------ 1. the mix
def mix(kind, which, nosrc=False):
    def build():
        items, code, mtu, sel = I.mix(3 * 256 + 131)
        b, ch = I.layout(items, kind)
        cf = I.cfg(src6=None) if nosrc else I.cfg(ident=65000)
        return b, ch, code, mtu, sel, cf, I.expect(b, ch, code, cf, mtu, I.MAP, sel, which)
    return I.cached(("mix", kind, which, nosrc), build)


@pytest.mark.parametrize("kind,which,nosrc", [("indexed", 0, False), ("stride", I.LAST, False), ("indexed", I.LAST, True)])
def test_mix_against_the_model(kind, which, nosrc):
    b, ch, code, mtu, sel, cf, want = mix(kind, which, nosrc)
    rc, got = I.host_call(b, ch, code, cf, mtu, I.MAP, sel, which)
    assert rc == 0 and got["guards"]
    I.check(got, want, got["cap"], kind)
    assert int(got["hits"].sum()) == b["n"]


def test_the_mix_meets_its_conditions():
    I.mix_conditions(mix("indexed", 0)[-1], mix("indexed", I.LAST, True)[-1])
    I.mix_conditions(mix("stride", I.LAST)[-1], mix("indexed", I.LAST, True)[-1])


# ------------------------------------------------------------------ 2. known answers, field by field
def csum(data):
    return ~rfc1071_sum(data) & 0xFFFF


def test_known_answer_time_exceeded_v4():
    """RFC 792: type 11 code 0, 4 unused bytes, the IP header + payload of the original datagram."""
    src = I.pkt(I.udp(30, 1), ttl=1)
    got, _ = run([src], I.R_TIME_EXCEEDED)
    dgram = src[0][14:]
    icmp = struct.pack(">BBHI", 11, 0, 0, 0) + dgram
    icmp = icmp[:2] + struct.pack(">H", csum(icmp)) + icmp[4:]
    ip = struct.pack(">BBHHHBBH4s4s", 0x45, 0xC0, 20 + len(icmp), 0xFFF0, 0, 200, 1, 0, socket.inet_aton(I.SRC4), I.A4S)
    ip = ip[:10] + struct.pack(">H", csum(ip)) + ip[12:]
    assert outputs(got) == [I.MAC_S + I.MAC_D + b"\x08\x00" + ip + icmp]


def test_known_answer_too_big_v4_with_its_mtu():
    """RFC 1191: type 3 code 4, 2 unused bytes, the next-hop MTU in bytes 6..7; 576 bytes in all (RFC 1812)."""
    src = I.pkt(I.udp(1400, 2), vlans=1)
    got, _ = run([src], I.R_TOO_BIG, mtu=1280)
    dgram = src[0][18:18 + 576 - 28]
    icmp = struct.pack(">BBHHH", 3, 4, 0, 0, 1280) + dgram
    icmp = icmp[:2] + struct.pack(">H", csum(icmp)) + icmp[4:]
    ip = struct.pack(">BBHHHBBH4s4s", 0x45, 0xC0, 576, 0xFFF0, 0, 200, 1, 0, socket.inet_aton(I.SRC4), I.A4S)
    ip = ip[:10] + struct.pack(">H", csum(ip)) + ip[12:]
    assert outputs(got) == [I.MAC_S + I.MAC_D + b"\x81\x00\x00\x64\x08\x00" + ip + icmp]


def v6_answer(src_item, ip_off, ty, code, word, l2):
    dgram = src_item[0][ip_off:ip_off + 1280 - 48]
    icmp = struct.pack(">BBHI", ty, code, 0, word) + dgram
    a = socket.inet_pton(socket.AF_INET6, I.SRC6)
    pseudo = a + I.A6S + struct.pack(">IBBBB", len(icmp), 0, 0, 0, 58)
    icmp = icmp[:2] + struct.pack(">H", csum(pseudo + icmp) or 0xFFFF) + icmp[4:]
    return l2 + struct.pack(">IHBB", 6 << 28 | 0xC0 << 20, len(icmp), 58, 200) + a + I.A6S + icmp


def test_known_answer_time_exceeded_v6():
    """RFC 4443 3.3: type 3 code 0, 4 unused bytes, as much of the packet as fits 1280."""
    src = I.pkt(I.udp(100, 3), v6=True, ttl=1)
    got, _ = run([src], I.R_TIME_EXCEEDED)
    assert outputs(got) == [v6_answer(src, 14, 3, 0, 0, I.MAC_S + I.MAC_D + b"\x86\xdd")]


def test_known_answer_packet_too_big_v6_to_a_multicast_destination():
    """RFC 4443 3.2 and 2.4 e.3: type 2 code 0, the MTU in bytes 4..7; sent although the destination is multicast."""
    mc = socket.inet_pton(socket.AF_INET6, "ff0e::1:2")
    src = I.pkt(I.udp(1452, 4), v6=True, dst=mc, dmac=b"\x33\x33\x00\x01\x00\x02")
    got, _ = run([src], I.R_TOO_BIG, mtu=1400)
    assert outputs(got) == [v6_answer(src, 14, 2, 0, 1400, I.MAC_S + b"\x33\x33\x00\x01\x00\x02" + b"\x86\xdd")]
    got, _ = run([src], I.R_TIME_EXCEEDED)
    assert got["status"].tolist() == [I.MCAST]


# ------------------------------------------------------------------ 3. properties that need no model
def test_properties_of_every_output_of_the_mix():
    b, ch, code, mtu, sel, cf, want = mix("indexed", 0)
    rc, got = I.host_call(b, ch, code, cf, mtu, I.MAP, sel, 0)
    assert rc == 0
    outs = outputs(got)
    assert len(outs) == got["n_out"] > 100
    oc_t, oc_o = got["oc_hdr_type"].reshape(I.MAXH, -1), got["oc_hdr_off"].reshape(I.MAXH, -1)
    for q, o in enumerate(outs):
        i = int(got["src_index"][q])
        s = b["slab"][int(b["offsets"][i]):int(b["offsets"][i]) + int(b["lens"][i])].tobytes()
        nh = int(got["oc_n_hdrs"][q])
        assert oc_t[nh - 1, q] == I.T_ICMP
        ip, v4 = int(oc_o[nh - 2, q]), oc_t[nh - 2, q] == I.T_IPV4
        nhs = int(ch["n_hdrs"][i])
        e = [j for j in range(nhs) if ch["hdr_type"][j, i] in (I.T_IPV4, I.T_IPV6)][0]
        sip = int(ch["hdr_off"][e, i])
        seth = sip - ip
        assert o[0:6] == s[seth + 6:seth + 12] and o[6:12] == s[seth:seth + 6] and o[12:ip] == s[seth + 12:sip]
        H = 20 if v4 else 40
        msg = o[ip + H:]
        Q = len(msg) - 8
        assert msg[8:] == s[sip:sip + Q]
        if v4:
            assert rfc1071_sum(o[ip:ip + 20]) == 0xFFFF and rfc1071_sum(msg) == 0xFFFF
            assert o[ip + 16:ip + 20] == s[sip + 12:sip + 16] and struct.unpack(">H", o[ip + 2:ip + 4])[0] == len(o) - ip
            assert struct.unpack(">H", o[ip + 4:ip + 6])[0] == (65000 + q) & 0xFFFF
        else:
            assert rfc1071_sum(o[ip + 8:ip + 40] + struct.pack(">IHBB", len(msg), 0, 0, 58) + msg) == 0xFFFF
            assert o[ip + 24:ip + 40] == s[sip + 8:sip + 24] and struct.unpack(">H", o[ip + 4:ip + 6])[0] == len(msg)


# ------------------------------------------------------------------ 4. one deciding packet per status, both sides of every boundary
def ip4(L=None, w=0, src=None, proto=17, pay=None, **kw):
    return I.pkt(I.udp(40, 7) if pay is None else pay, L=L, w=w, src=src, proto=proto, **kw)


STATUS_CASES = {
    "sent": (ip4(), 1, I.SENT),
    "skipped_reason_0": (ip4(), 0, I.SKIPPED),
    "bad_reason_7": (ip4(), 7, I.BAD_REASON),
    "reason_6": (ip4(), 6, I.SENT),
    "no_ip": ((ip4()[0], [(I.T_ETHER, 0)]), 1, I.NO_IP),
    "span_ip": ((ip4()[0][:30], [(I.T_ETHER, 0), (I.T_IPV4, 14)]), 1, I.SPAN),
    "span_ether_runs_into_ip": ((ip4()[0], [(I.T_ETHER, 2), (I.T_IPV4, 14)]), 1, I.SPAN),
    "ether_after_ip_is_no_ether": ((ip4()[0], [(I.T_IPV4, 14), (I.T_ETHER, 0)]), 1, I.NO_ETHER),
    "no_ether": ((ip4()[0][14:], [(I.T_IPV4, 0)]), 1, I.NO_ETHER),
    "bad_hdr_ihl_6": (ip4(b0=0x46), 1, I.BAD_HDR),
    "bad_hdr_L_19": (ip4(L=19), 1, I.BAD_HDR),
    "L_20": (ip4(L=20), 1, I.SENT),
    "bad_hdr_v6_version_5": (I.pkt(I.udp(40), v6=True, b0=0x50), 1, I.BAD_HDR),
    "fragment_offset_1": (ip4(w=1), 1, I.FRAGMENT),
    "fragment_offset_1_mf": (ip4(w=0x2001), 1, I.FRAGMENT),
    "first_fragment_mf_offset_0": (ip4(w=0x2000), 1, I.SENT),
    "df": (ip4(w=0x4000), 2, I.SENT),
    "src_223": (ip4(src=bytes([223, 255, 255, 255])), 1, I.SENT),
    "bad_src_224": (ip4(src=bytes([224, 0, 0, 1])), 1, I.BAD_SRC),
    "bad_src_0": (ip4(src=bytes([0, 1, 2, 3])), 1, I.BAD_SRC),
    "src_1": (ip4(src=bytes([1, 0, 0, 0])), 1, I.SENT),
    "bad_src_127": (ip4(src=bytes([127, 0, 0, 1])), 1, I.BAD_SRC),
    "src_126_and_128": (ip4(src=bytes([128, 0, 0, 1])), 1, I.SENT),
    "bad_src_v6_unspecified": (I.pkt(I.udp(40), v6=True, src=bytes(16)), 1, I.BAD_SRC),
    "src_v6_last_byte_alone": (I.pkt(I.udp(40), v6=True, src=bytes(15) + b"\x01"), 1, I.SENT),
    "bad_src_v6_multicast": (I.pkt(I.udp(40), v6=True, src=b"\xff" + bytes(15)), 1, I.BAD_SRC),
    "src_v6_fe": (I.pkt(I.udp(40), v6=True, src=b"\xfe\x80" + bytes(14)), 1, I.SENT),
    "mcast_ether_group_bit": (ip4(dmac=b"\x01\x00\x5e\x01\x02\x03"), 1, I.MCAST),
    "mcast_broadcast_mac": (ip4(dmac=b"\xff" * 6), 1, I.MCAST),
    "mcast_dst_224": (ip4(dst=bytes([224, 0, 0, 1])), 1, I.MCAST),
    "dst_223": (ip4(dst=bytes([223, 0, 0, 1])), 1, I.SENT),
    "mcast_v6_dst_ff": (I.pkt(I.udp(40), v6=True, dst=b"\xff\x02" + bytes(14)), 1, I.MCAST),
    "v6_dst_ff_too_big_is_sent": (I.pkt(I.udp(40), v6=True, dst=b"\xff\x02" + bytes(14)), 2, I.SENT),
    "v6_group_mac_too_big_is_sent": (I.pkt(I.udp(40), v6=True, dmac=b"\x33\x33\0\0\0\x01"), 2, I.SENT),
    "v4_dst_224_too_big_is_mcast": (ip4(dst=bytes([224, 0, 0, 1])), 2, I.MCAST),
    "icmp_type_8": (ip4(proto=1, pay=I.icmp(8)), 1, I.SENT),
    "icmp_type_0": (ip4(proto=1, pay=I.icmp(0)), 1, I.SENT),
    "icmp_err_type_11": (ip4(proto=1, pay=I.icmp(11)), 1, I.ICMP_ERR),
    "icmp_err_type_3": (ip4(proto=1, pay=I.icmp(3)), 1, I.ICMP_ERR),
    "icmp_err_type_4": (ip4(proto=1, pay=I.icmp(4)), 1, I.ICMP_ERR),
    "icmp_err_type_5": (ip4(proto=1, pay=I.icmp(5)), 1, I.ICMP_ERR),
    "icmp_err_type_12": (ip4(proto=1, pay=I.icmp(12)), 1, I.ICMP_ERR),
    "icmp_type_13": (ip4(proto=1, pay=I.icmp(13)), 1, I.SENT),
    "icmp_err_type_byte_just_outside_L": (ip4(proto=1, pay=I.icmp(8), L=20), 1, I.ICMP_ERR),
    "icmp_type_byte_just_inside_L": (ip4(proto=1, pay=I.icmp(8), L=21), 1, I.SENT),
    "icmp_err_type_byte_outside_the_packet": (ip4(proto=1, pay=I.icmp(8), trunc=16), 1, I.ICMP_ERR),
    "type_11_under_udp_is_no_icmp": (ip4(proto=17, pay=I.icmp(11)), 1, I.SENT),
    "icmp6_err_127": (I.pkt(I.icmp(127), v6=True, proto=58), 1, I.ICMP_ERR),
    "icmp6_err_1": (I.pkt(I.icmp(1), v6=True, proto=58), 1, I.ICMP_ERR),
    "icmp6_128": (I.pkt(I.icmp(128), v6=True, proto=58), 1, I.SENT),
    "icmp6_136": (I.pkt(I.icmp(136), v6=True, proto=58), 1, I.SENT),
    "icmp6_err_137": (I.pkt(I.icmp(137), v6=True, proto=58), 1, I.ICMP_ERR),
    "icmp6_138": (I.pkt(I.icmp(138), v6=True, proto=58), 1, I.SENT),
    "icmp6_err_type_byte_missing": (I.pkt(I.icmp(128), v6=True, proto=58, trunc=16), 1, I.ICMP_ERR),
    "icmp6_err_type_byte_outside_the_payload_length": (I.pkt(I.icmp(128), v6=True, proto=58, L=0), 1, I.ICMP_ERR),
    "icmp_proto_1_under_v6_is_no_icmp": (I.pkt(I.icmp(1), v6=True, proto=1), 1, I.SENT),
}


@pytest.mark.parametrize("name", sorted(STATUS_CASES))
def test_status(name):
    item, r, st = STATUS_CASES[name]
    got, want = run([item, ip4()], np.asarray([r, 1], np.uint8), mtu=1400)
    assert got["status"].tolist() == [st, I.SENT], (name, schema.ICMPE_STATUS[got["status"][0]])
    assert got["n_out"] == (2 if st == I.SENT else 1)


def test_skipped_by_select_and_no_src_per_version():
    items = [ip4(), I.pkt(I.udp(40), v6=True), ip4()]
    got, _ = run(items, 1, select=np.asarray([1, 1, 0], np.uint8))
    assert got["status"].tolist() == [I.SENT, I.SENT, I.SKIPPED]
    got, _ = run(items, 1, cf=I.cfg(src6=None))
    assert got["status"].tolist() == [I.SENT, I.NO_SRC, I.SENT]
    got, _ = run(items, 1, cf=I.cfg(src4=None))
    assert got["status"].tolist() == [I.NO_SRC, I.SENT, I.NO_SRC]


def test_every_status_has_a_deciding_case():
    assert {st for _, _, st in STATUS_CASES.values()} | {I.NO_SRC} == set(range(I.NSTATUS))
    assert len(schema.ICMPE_STATUS) == schema.ICMPE_STATUS_COUNT == I.NSTATUS


def test_every_reason_gives_its_type_and_code():
    items = [ip4(), I.pkt(I.udp(40), v6=True)] * 6
    code = np.repeat(np.arange(1, 7, dtype=np.uint8), 2)
    got, _ = run(items, code, mtu=1300)
    outs = outputs(got)
    for q, o in enumerate(outs):
        r, v6 = 1 + q // 2, q % 2
        assert (o[14 + (40 if v6 else 20)], o[15 + (40 if v6 else 20)]) == schema.ICMP_TYPE_CODE[r][v6]
    assert schema.ICMP_TYPE_CODE == I.TYPE_CODE


# ------------------------------------------------------------------ 5. the quote's edges
@pytest.mark.parametrize("v6", [False, True])
def test_quote_edges(v6):
    H, mx = (40, 1280) if v6 else (20, 576)
    room = mx - H - 8
    items = [I.pkt(I.udp(room - H + d, d + 5), v6=v6, vlans=d % 3) for d in (-1, 0, 1)]   # Q one less, exact, clipped
    items += [I.pkt(I.udp(50, 9), v6=v6, pad=13),                  # L below len - ip_off: the padding is not quoted
              I.pkt(I.udp(300, 10), v6=v6, trunc=100),             # L above it: quoted as far as the record goes
              I.pkt(I.udp(128 - 14 - H - 8 - H, 1), v6=v6),        # out_len a multiple of 16
              I.pkt(I.udp(129 - 14 - H - 8 - H, 2), v6=v6)]        # ... and one over
    got, want = run(items, 2, mtu=1000)
    q = [len(o) - 14 - 4 * vl - H - 8 for vl, o in zip((2, 0, 1, 0, 0, 0, 0), outputs(got))]
    assert q[:3] == [room - 1, room, room] and q[3] == H + 50 and q[4] == H + 200
    assert got["out_len"][5] == 128 and got["out_len"][6] == 129 and got["bytes_out"] % 16 == 0


def test_max_sizes_and_their_limits():
    src = [I.pkt(I.udp(65535 - 20, 3)), I.pkt(I.udp(3000, 4), v6=True), I.pkt(I.udp(8, 1))]
    got, _ = run(src, 1, cf=I.cfg(max4=65535, max6=65535))
    assert got["out_len"].tolist()[:3] == [14 + 65535, 14 + 40 + 8 + 3040, 14 + 28 + 28]
    got, _ = run(src, 1, cf=I.cfg(max4=56, max6=96))
    assert got["out_len"].tolist()[:3] == [14 + 56, 14 + 96, 14 + 56]


# ------------------------------------------------------------------ 6. map, forged chains, capacities, refusals
def test_a_map_gives_what_the_explicit_reasons_give():
    b, ch, code, mtu, sel, cf, want = mix("stride", I.LAST)
    rc, a = I.host_call(b, ch, code, cf, mtu, I.MAP, sel, I.LAST)
    rc2, c = I.host_call(b, ch, I.MAP[code], cf, mtu, None, sel, I.LAST)
    assert rc == rc2 == 0
    for k in a:
        assert np.array_equal(a[k], c[k]), k
    for m, name in ((schema.ICMP_MAP_FWD, "FWD"), (schema.ICMP_MAP_FRAG, "FRAG")):
        assert m.shape == (256,) and m.dtype == np.uint8
    assert {k: int(v) for k, v in enumerate(schema.ICMP_MAP_FWD) if v} == {schema.FWD_TTL: 1, schema.FWD_MTU: 2, schema.FWD_NO_ADJ: 3}
    assert {k: int(v) for k, v in enumerate(schema.ICMP_MAP_FRAG) if v} == {schema.FRAG_DF: 2, schema.FRAG_IPV6: 2}


def test_forged_chains_and_odd_offsets():
    """An odd eth_off (Ether at 1, IP at 15), an odd P (Ether at 0, IP at 15), n_hdrs 255, sixteen rows."""
    p, _ = I.pkt(I.udp(700, 5))
    one = b"\x00" + p
    p15 = p[:14] + b"\x99" + p[14:]
    rows16 = [(I.T_VLAN, 0)] * 14 + [(I.T_ETHER, 0), (I.T_IPV4, 14)]
    full = [(I.T_ETHER, 0)] + [(I.T_VLAN, 14)] * 14 + [(I.T_IPV4, 14)]
    items = [(one, [(I.T_ETHER, 1), (I.T_IPV4, 15)]), (p15, [(I.T_ETHER, 0), (I.T_IPV4, 15)]), (p, rows16), (p, full)]
    b, ch = I.layout(items)
    ch["n_hdrs"][2] = 255
    want = I.expect(b, ch, 1, CF)
    rc, got = I.host_call(b, ch, 1, CF)
    assert rc == 0 and got["guards"] and got["status"].tolist() == [I.SENT] * 4
    I.check(got, want, got["cap"])
    assert got["oc_n_hdrs"].tolist() == [3, 3, 3, 16]


def test_capacities_exact_short_and_with_an_empty_tail():
    b, ch, code, mtu, sel, cf, want = mix("stride", I.LAST)
    k, nb = want["n_out"], want["bytes_out"]
    rc, got = I.host_call(b, ch, code, cf, mtu, I.MAP, sel, I.LAST, cap=k, dst_len=nb)
    assert rc == 0 and got["guards"]
    I.check(got, want, k)
    for cap, room in ((k - 1, nb), (k, nb - 16)):
        rc, got = I.host_call(b, ch, code, cf, mtu, I.MAP, sel, I.LAST, cap=cap, dst_len=room)
        assert rc == INVALID and got["guards"] and (got["n_out"], got["bytes_out"]) == (k, nb)
        for name in ("status", "hits"):
            assert np.array_equal(got[name], want[name]), name
        assert (got["dst"] == 0xA5).all()
    rc, got = I.host_call(b, ch, code, cf, mtu, I.MAP, sel, I.LAST, cap=k + 300, dst_len=nb + 4096)
    assert rc == 0 and got["guards"]
    I.check(got, want, k + 300)
    assert (got["dst"][nb:] == 0xA5).all()


def test_no_write_null_outputs_and_n_0():
    b, ch, code, mtu, sel, cf, want = mix("stride", I.LAST)
    rc, got = I.host_call(b, ch, code, cf, mtu, I.MAP, sel, I.LAST, flags=I.NO_WRITE)
    assert rc == 0 and got["guards"]
    I.check(got, want, 0)
    rc, got = I.host_call(b, ch, code, cf, mtu, I.MAP, sel, I.LAST, flags=I.NO_WRITE, skip=["status", "out_index", "hits"])
    assert rc == 0 and (got["n_out"], got["bytes_out"]) == (want["n_out"], want["bytes_out"])
    for skip in (["status", "out_index", "hits", "src_index", "oc_n_hdrs", "oc_hdr_type", "oc_hdr_off"], ["oc_hdr_type"], ["src_index", "oc_n_hdrs"]):
        rc, got = I.host_call(b, ch, code, cf, mtu, I.MAP, sel, I.LAST, skip=skip)
        assert rc == 0 and got["guards"]
        I.check(got, want, got["cap"], str(skip))
    b0 = dict(b, n=0, lens=b["lens"][:0])
    ch0 = {k: v[..., :0] for k, v in ch.items()}
    rc, got = I.host_call(b0, ch0, 1, cf, cap=5, dst_len=64)
    assert rc == 0 and got["guards"] and (got["n_out"], got["bytes_out"]) == (0, 0)
    assert (got["out_off"] == 0).all() and (got["out_len"] == 0).all() and (got["src_index"] == I.NONE).all()
    assert (got["oc_n_hdrs"] == 0).all() and (got["dst"] == 0xA5).all()


def refusals():
    from pktgpu import _lib
    odd = np.zeros(64, np.uint8)
    base = odd.ctypes.data
    bad = {"cfg_no_address": I.cfg(None, None), "max4_55": I.cfg(max4=55), "max6_95": I.cfg(max6=95)}
    keep = {k: I.lib_cfg(v) for k, v in bad.items()}
    r = {"null_batch": {I.A_BATCH: None}, "null_chain": {I.A_CHAIN: None}, "which_16": {I.A_WHICH: 16},
         "which_0xFE": {I.A_WHICH: 0xFE}, "flag_bit_2": {I.A_FLAGS: 2}, "flag_bit_31": {I.A_FLAGS: 1 << 31},
         "null_cfg": {I.A_CFG: None}, "code_all_256": {I.A_CODE: None, I.A_CODE_ALL: 256},
         "mtu_all_65536": {I.A_MTU: None, I.A_MTU_ALL: 65536}, "dst_misaligned": {I.A_DST: base + 8},
         "hits_misaligned": {I.A_HITS: base + 4}, "out_off_misaligned": {I.A_OUT_OFF: base + 4},
         "mtu_misaligned": {I.A_MTU: base + 1}, "null_dst": {I.A_DST: None}, "null_out_off": {I.A_OUT_OFF: None},
         "null_out_len": {I.A_OUT_LEN: None}, "out_cap_0": {I.A_CAP: 0}, "out_cap_2_32": {I.A_CAP: 1 << 32}}
    for k, c in keep.items():
        r[k] = {I.A_CFG: ctypes.byref(c)}
    for col in ("n_hdrs", "hdr_type", "hdr_off"):
        ch = _lib.PktChain(base, base, base)
        setattr(ch, col, None)
        r[f"null_chain_{col}"] = {I.A_CHAIN: ctypes.byref(ch)}
    return r, (odd, keep)


REFUSALS = sorted(refusals()[0])


@pytest.mark.parametrize("name", REFUSALS)
def test_refusals(name):
    over, keep = refusals()
    b, ch = I.layout([ip4(), ip4()])
    rc, got = I.host_call(b, ch, np.asarray([1, 2], np.uint8), CF, np.asarray([576, 576], np.uint16), over=over[name], cap=8,
                          dst_len=4096)
    assert rc == INVALID and got["guards"]
    assert (got["status"] == 0xA5).all() and (got["dst"] == 0xA5).all() and (got["hits"] == 0).all()


def test_the_limits_themselves_are_taken():
    b, ch = I.layout([ip4(), ip4()])
    for cf, code, m in ((I.cfg(max4=56, max6=96), 255, 65535), (I.cfg(src6=None, max4=65535), 1, 0), (I.cfg(src4=None, max6=65535), 1, 0)):
        rc, got = I.host_call(b, ch, code, cf, m)
        assert rc == 0
    assert ctypes.sizeof(pktgpu._lib.PktIcmpCfg) == pktgpu._lib.load().pkt_sizeof_icmp_cfg() == 28


@pytest.mark.parametrize("form", ["n_2_32", "offsets_without_lens", "stride_0", "null_slab"])
def test_batch_refusals(form):
    from pktgpu import _lib
    L = _lib.load()
    b, ch = I.layout([ip4(), ip4()])
    pb, keep = pktgpu._host_batch(_lib, b)
    if form == "n_2_32":
        pb.n = 1 << 32
    elif form == "offsets_without_lens":
        pb.lens = None
    elif form == "stride_0":
        pb.offsets, pb.stride = None, 0
    else:
        pb.slab = None
    cols = [np.ascontiguousarray(ch[k]) for k in ("n_hdrs", "hdr_type", "hdr_off")]
    pc = _lib.PktChain(*[c.ctypes.data for c in cols])
    cc = I.lib_cfg(CF)
    tot, cnt = ctypes.c_uint64(7), ctypes.c_uint64(7)
    rc = L.pkt_icmp_err_host(ctypes.byref(pb), ctypes.byref(pc), 0, schema.ICMPE_NO_WRITE, ctypes.byref(cc), None, 1, None, None,
                             0, None, None, None, None, 0, 0, None, None, None, None, None, ctypes.byref(tot), ctypes.byref(cnt))
    assert rc == INVALID and (tot.value, cnt.value) == (0, 0)


# ------------------------------------------------------------------ 7. the Python form and what takes the result
def test_python_form_and_the_next_calls():
    """Parser.icmp_errors(host=True) with fwd_status / frag_status / reason, and pkt_fwd_host / pkt_flow_key_host /
    pkt_l4_checksum over the output batch with out_chain."""
    items = [I.pkt(I.udp(1400, 1), ttl=1), I.pkt(I.udp(1400, 2), v6=True), I.pkt(I.udp(100, 3), vlans=2), I.pkt(I.udp(40, 4))]
    b, ch = I.layout(items)
    st = np.asarray([schema.FWD_TTL, schema.FWD_MTU, schema.FWD_NO_ADJ, schema.FWD_OK], np.uint8)
    e = pktgpu.Parser.icmp_errors(None, b, ch, fwd_status=st, mtu=np.asarray([0, 1280, 0, 0], np.uint16), src4=I.SRC4,
                                  src6=socket.inet_pton(socket.AF_INET6, I.SRC6), hits=True, host=True)
    assert isinstance(e, pktgpu.IcmpErrResult) and e.n_out == 3 and e.status.tolist() == [I.SENT, I.SENT, I.SENT, I.SKIPPED]
    assert e.out_index.tolist() == [0, 1, 2, I.NONE] and e.src_index.tolist() == [0, 1, 2] and int(e.hits.sum()) == 4
    want = I.expect(b, ch, st, I.cfg(max4=576, max6=1280, ttl=64), np.asarray([0, 1280, 0, 0]), schema.ICMP_MAP_FWD)
    assert [e.slab[int(o):int(o) + int(ln)].tobytes() for o, ln in zip(e.offsets, e.lens)] == want["pkts"]
    f = pktgpu.Parser.icmp_errors(None, b, ch, frag_status=np.asarray([schema.FRAG_DF, schema.FRAG_IPV6, 0, 1], np.uint8),
                                  mtu=1000, src4=I.SRC4, src6=I.SRC6, host=True, plan_only=True)
    assert f.status.tolist() == [I.SENT, I.SENT, I.SKIPPED, I.SKIPPED] and f.n_out == 2 and f.slab is None
    with pytest.raises(ValueError):
        pktgpu.Parser.icmp_errors(None, b, ch, src4=I.SRC4, host=True)
    with pytest.raises(ValueError):
        pktgpu.Parser.icmp_errors(None, b, ch, reason=1, fwd_status=st, src4=I.SRC4, host=True)
    k = e.n_out
    fwd = pktgpu.Forwarder(None, [("02:00:00:00:00:01", "02:00:00:00:00:02", 9, 1500)])
    r = fwd.run(e.batch(), e.out_chain, nexthop=np.zeros(k, np.uint32), write=False)
    assert (r["status"][:k] == pktgpu.FWD_OK).all()
    fk = pktgpu.flow_keys(e.slab, e.out_chain, which_ip=0, offsets=e.offsets, lens=e.lens)
    keys = fk["keys"].view(schema.FLOW_KEY_DTYPE).reshape(-1)
    assert keys["proto"][:k].tolist() == [1, 58, 1] and keys["ipver"][:k].tolist() == [4, 6, 4]
    assert bytes(keys["src"][0][:4]) == socket.inet_aton(I.SRC4) and bytes(keys["dst"][0][:4]) == I.A4S
    assert bytes(keys["src"][1]) == socket.inet_pton(socket.AF_INET6, I.SRC6) and bytes(keys["dst"][1]) == I.A6S
