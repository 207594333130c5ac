"""Batch pairs and expected results shared by test_compare_host.py and test_compare_device.py.

A case is a dict {"a", "b", "ignore", "chain"}: two batches over numpy arrays (slab, stride or offsets /
lens, n), up to 16 ignore specs (hdr name, occurrence, start, end) and the chain columns of `a` (from
the Python parser model pyref, None without ignores).  `expect(case)` computes pkt_compare_batch's
outputs from its definition with numpy, pair by pair: never with pkt_compare_host or the device.
"""
import os

import numpy as np

import pyref
from pktgpu import fields as F
from pktgpu import gen, schema

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EQUAL, LEN, BYTES = 0, 1, 2


def batch(slab, offsets=None, lens=None, stride=None, n=None):
    slab = np.ascontiguousarray(slab, np.uint8).reshape(-1)
    if n is None:
        n = len(offsets) if offsets is not None else slab.size // stride
    return dict(slab=slab, offsets=None if offsets is None else np.asarray(offsets, np.uint64),
                lens=None if lens is None else np.asarray(lens, np.uint32), stride=stride, n=int(n))


def case(a, b, ignore=(), chain=None):
    assert a["n"] == b["n"]
    return dict(a=a, b=b, ignore=list(ignore), chain=chain)


def extents(b):
    """pkt_batch_t's rules: (offset, length) of every packet, the length clamped to the slab end and
    to 65535."""
    out = []
    for i in range(b["n"]):
        off = int(b["offsets"][i]) if b["offsets"] is not None else i * b["stride"]
        ln = int(b["lens"][i]) if b["lens"] is not None else b["stride"]
        out.append((off, min(ln, max(0, b["slab"].size - off), 65535)))
    return out


def packets(b):
    return [b["slab"][o:o + ln].tobytes() for o, ln in extents(b)]


def chain_of(b):
    """The chain columns of a parse of b, by the Python model of the parser (slot-major)."""
    n = b["n"]
    nh = np.zeros(n, np.uint8)
    ty = np.zeros((schema.MAX_HDRS, n), np.uint8)
    of = np.zeros((schema.MAX_HDRS, n), np.uint16)
    for i, p in enumerate(packets(b)):
        hdrs = pyref.parse(p)[1]
        nh[i] = len(hdrs)
        for j, (name, o) in enumerate(hdrs):
            ty[j, i] = schema.HDR_ID[name]
            of[j, i] = o
    return dict(n_hdrs=nh, hdr_type=ty, hdr_off=of)


def spec(hdr, field, occ=0):
    s, e = F.FIELDS[schema.HDR_ID[hdr]][field]
    return (hdr, occ, s, e)


def ranges(c, i):
    """Per spec: the (first, last) ignored bit of packet i, packet-relative, or None where packet i's
    chain has no such header."""
    out = []
    ch = c["chain"]
    for hdr, occ, s, e in c["ignore"]:
        t = schema.HDR_ID[hdr] if isinstance(hdr, str) else hdr
        at = [int(ch["hdr_off"][j, i]) for j in range(min(int(ch["n_hdrs"][i]), schema.MAX_HDRS))
              if ch["hdr_type"][j, i] == t]
        out.append((8 * at[occ] + s, 8 * at[occ] + e) if occ < len(at) else None)
    return out


def expect(c):
    """(result, matching, first_diff, summary) of the case, from the definition."""
    n = c["a"]["n"]
    ea, eb = extents(c["a"]), extents(c["b"])
    res, mt, fd = np.zeros(n, np.uint8), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    for i in range(n):
        (oa, la), (ob, lb) = ea[i], eb[i]
        m = min(la, lb)
        x = c["a"]["slab"][oa:oa + m] ^ c["b"]["slab"][ob:ob + m]
        if c["ignore"]:
            bits = np.zeros(8 * m, bool)
            for r in ranges(c, i):
                if r is not None:
                    bits[r[0]:r[1] + 1] = True  # (clipped at 8 m: bits past the common bytes are dropped)
            x = x & ~np.packbits(bits)          # MSB-first, as make_header!
        bad = np.flatnonzero(x)
        mt[i] = m - bad.size
        fd[i] = bad[0] if bad.size else m
        res[i] = LEN if la != lb else BYTES if mt[i] != la else EQUAL
    nz = np.flatnonzero(res)
    summary = dict(n_equal=int((res == EQUAL).sum()), n_len=int((res == LEN).sum()),
                   n_bytes=int((res == BYTES).sum()), first_bad=int(nz[0]) if nz.size else n)
    return res, mt, fd, summary


def check(got, want, label=""):
    res, mt, fd, sm = got
    w_res, w_mt, w_fd, w_sm = want
    for name, g, w in (("result", res, w_res), ("matching", mt, w_mt), ("first_diff", fd, w_fd)):
        bad = np.flatnonzero(np.asarray(g) != w)
        assert bad.size == 0, (label, name, "first bad pairs", bad[:8], np.asarray(g)[bad[:8]], w[bad[:8]])
    if w_sm is not None:
        assert sm == w_sm, (label, sm, w_sm)


# ------------------------------------------------------------------ layouts
def indexed(pkts, rng, align=None, pad=0):
    """The packets back to back in a slab, each at a random (or the given) offset mod 16."""
    offs, pos = [], 0
    for k, p in enumerate(pkts):
        al = int(rng.integers(0, 16)) if align is None else align[k]
        pos = (pos + 15) // 16 * 16 + al
        offs.append(pos)
        pos += len(p)
    slab = rng.integers(0, 256, pos + pad, dtype=np.uint8)
    for o, p in zip(offs, pkts):
        slab[o:o + len(p)] = np.frombuffer(p, np.uint8)
    return batch(slab, offs, [len(p) for p in pkts])


def flip(p, j, mask=0x80):
    q = bytearray(p)
    q[j] ^= mask
    return bytes(q)


# ------------------------------------------------------------------ plain cases
ALIGN_LENS = [0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65]


def alignment():
    """Every (a offset mod 16, b offset mod 16) at every length of ALIGN_LENS, the pair equal and with
    one byte flipped at every position (so: at 0, at len - 1 and at every position mod 16).  Returns the
    case and the expected (result, matching, first_diff), known by construction."""
    rng = np.random.default_rng(21)
    la, res, mt, fd, ja = [], [], [], [], []
    for ln in ALIGN_LENS:
        for j in range(-1, ln):  # -1: no flip
            la.append(ln)
            ja.append(j)
            res.append(EQUAL if j < 0 else BYTES)
            mt.append(ln if j < 0 else ln - 1)
            fd.append(ln if j < 0 else j)
    k = len(la)
    la, ja = np.tile(np.array(la), 256), np.tile(np.array(ja), 256)
    al = np.repeat(np.arange(256), k)
    n = la.size
    oa = 96 * np.arange(n) + (al >> 4)
    ob = 96 * np.arange(n) + (al & 15) + 48  # b's slots are not a's: another slab position too
    A = rng.integers(0, 256, 96 * n + 64, dtype=np.uint8)
    B = rng.integers(0, 256, 96 * n + 128, dtype=np.uint8)
    for ln in ALIGN_LENS:
        idx = np.flatnonzero(la == ln)
        cols = np.arange(ln)
        B[ob[idx][:, None] + cols] = A[oa[idx][:, None] + cols]
    f = np.flatnonzero(ja >= 0)
    B[ob[f] + ja[f]] ^= rng.integers(1, 256, f.size, dtype=np.uint8)
    c = case(batch(A, oa, la), batch(B, ob, la))
    return c, (np.tile(np.array(res, np.uint8), 256), np.tile(np.array(mt, np.uint32), 256),
               np.tile(np.array(fd, np.uint32), 256))


def tiling(n):
    """n 64-byte pairs, a at fixed stride against an indexed, misaligned b; a quarter of the pairs
    differ in one to three random bytes, and pair n - 1 only in its last byte."""
    rng = np.random.default_rng(100 + n)
    a = gen.gen_c2(n, seed=n)
    pk = [a[i].tobytes() for i in range(n)]
    for i in np.flatnonzero(rng.random(n) < 0.25):
        for j in rng.integers(0, 64, int(rng.integers(1, 4))):
            pk[i] = flip(pk[i], int(j), int(rng.integers(1, 256)))
    pk[n - 1] = flip(a[n - 1].tobytes(), 63, 0x01)
    return case(batch(a, stride=64), indexed(pk, rng))


def long_among_short():
    """One 65535-byte pair and 4095 / 4096 / 4097-byte pairs among 64-byte pairs, all inside one wave's
    64 pairs (and a second wave of short ones); the long pairs equal, differing only in their last
    byte, or in a byte of their middle."""
    rng = np.random.default_rng(23)
    lens = [64] * 130
    for at, ln in ((3, 65535), (10, 4095), (11, 4096), (12, 4097), (40, 4096), (41, 4097), (63, 4095), (64, 4097)):
        lens[at] = ln
    pa = [rng.integers(0, 256, ln, dtype=np.uint8).tobytes() for ln in lens]
    pb = list(pa)
    pb[3] = flip(pa[3], 65534)
    pb[11] = flip(pa[11], 4095)
    pb[12] = flip(flip(pa[12], 4096), 2048)
    pb[41] = flip(pa[41], 16)
    pb[63] = flip(pa[63], 0)
    pb[20] = flip(pa[20], 63)
    return case(indexed(pa, rng), indexed(pb, rng))


def clamped():
    """Pairs running past slab_len on either side (compared over the clamped lengths) and slots at or
    wholly past the end (empty packets), indexed; and a fixed-stride batch whose n passes its slab."""
    rng = np.random.default_rng(29)
    A = rng.integers(0, 256, 1000, dtype=np.uint8)
    B = np.concatenate([A[:900], rng.integers(0, 256, 77, dtype=np.uint8)])  # 977 bytes
    offs = [10, 900, 1000, 5000, 999, 0, 850, 976, 977]
    a = batch(A, offs, [50, 200, 50, 10, 70000, 70000, 150, 1, 1])
    b = batch(B, offs, [50, 200, 50, 10, 70000, 70000, 150, 1, 1])
    fixed = case(batch(A, stride=64, n=18), batch(B[:970], stride=64, n=18))  # a's 15 = 40 bytes, b's = 10
    return case(a, b), fixed


def length_mismatch():
    """PKT_CMP_LEN: b cut by a snaplen (matching == the common length), b longer than a, and cut pairs
    that also differ inside the common bytes."""
    rng = np.random.default_rng(31)
    pa = [rng.integers(0, 256, ln, dtype=np.uint8).tobytes() for ln in (64, 64, 100, 1, 0, 300, 4097, 64, 33)]
    pb = [pa[0][:60], pa[1] + b"\x00" * 5, pa[2][:16], b"", b"\x07", flip(pa[5], 17)[:299], pa[6][:4096],
          flip(pa[7], 0)[:63], flip(pa[8], 31)[:32]]
    return case(indexed(pa, rng), indexed(pb, rng))


# ------------------------------------------------------------------ ignores
def mixed_packets(n3=60, seed=41):
    """C3 packets (Ether, 0-2 Vlan tags, IPv4, TCP | UDP) interleaved with the 22 reference packets (C4's
    templates: IPv6, tunnels, ARP, LLC, GRE ...), plus a Vlan-tagged IPv6 packet, a long one and a
    truncated one (no chain: n_hdrs = 0)."""
    c3 = gen.gen_c3(n3, seed=seed)
    ref = [p.to_vec() for p in gen.reference_22_packets()]
    v6 = gen.create_tcpv6_packet("00:01:02:03:04:05", "00:06:07:08:09:0a", True, 10, 3, 5, 4, 64, "AAAA::1", "BBBB::1",
                                 1234, 9090, 100, 101, 5, 0, 1, 0, 0, bytes(range(100))).to_vec()
    long_ = gen.test_tcp_packet_with_payload(bytes(i & 0xFF for i in range(5000))).to_vec()
    out = []
    for i in range(n3):
        out.append(c3[i].tobytes())
        if i < len(ref):
            out.append(bytes(ref[i]))
    return out + [bytes(v6), bytes(long_), bytes(ref[0][:20])]


def noisy(pkts, ignore, seed, cut=None):
    """The case of `pkts` against a copy with bits flipped around the ignored ranges.  Packet i, by
    its random mode (the case's "modes"): 0 unchanged; 1 flipped only inside its ignored ranges; 2 flipped in a bit next to one of its
    ranges (the case's "neighbour" set lists these packets); 3 flipped inside a range and at a random byte.  cut(i, len) = b's length for packet i."""
    rng = np.random.default_rng(seed)
    a = indexed(pkts, rng)
    c = case(a, a, ignore, chain_of(a))
    pb, neighbour = [], set()
    modes = rng.integers(0, 4, len(pkts))
    for i, p in enumerate(pkts):
        q = bytearray(p)
        rs = [r for r in ranges(c, i) if r is not None and r[0] < 8 * len(p)]
        mode = int(modes[i])

        def xor_bit(t):
            if 0 <= t < 8 * len(q):
                q[t // 8] ^= 0x80 >> (t % 8)

        if rs and mode in (1, 3):
            for lo, hi in rs:
                hi = min(hi, 8 * len(p) - 1)
                xor_bit(lo)
                xor_bit(hi)
                for t in rng.integers(lo, hi + 1, 3):
                    xor_bit(int(t))
        if rs and mode == 2:  # a neighbouring bit that no other range covers
            cand = [t for lo, hi in rs for t in (lo - 1, hi + 1)
                    if 0 <= t < 8 * len(q) and not any(l2 <= t <= h2 for l2, h2 in rs)]
            if cand:
                xor_bit(cand[int(rng.integers(0, len(cand)))])
                neighbour.add(i)
        if mode == 3 and len(q):
            q[int(rng.integers(0, len(q)))] ^= int(rng.integers(1, 256))
        q = bytes(q)
        pb.append(q if cut is None else q[:cut(i, len(q))])
    return dict(case(a, indexed(pb, rng), ignore, c["chain"]), neighbour=neighbour, modes=modes)


def ignore_cases():
    mixed = mixed_packets()
    ip4ip4 = [bytes(gen.reference_22_packets()[12].to_vec())] * 24 + [bytes(gen.reference_22_packets()[0].to_vec())] * 8
    ipv4_all = [spec("IPv4", f) for f in F.FIELDS[schema.HDR_ID["IPv4"]]]
    cs = {
        # byte-straddling fields: Vlan.vid (12 bits from bit 4), IPv4 flags (3 bits) + frag_startset (13)
        "straddle": noisy(mixed, [spec("Vlan", "vid"), spec("IPv4", "flags"), spec("IPv4", "frag_startset")], 51),
        # a 128-bit field; absent in the IPv4 packets of the batch
        "ipv6_src": noisy(mixed, [spec("IPv6", "src")], 52),
        # the inner header of an IP-in-IP packet (absent in the plain TCP packets at the end)
        "occurrence_1": noisy(ip4ip4, [spec("IPv4", "ttl", 1), spec("IPv4", "header_checksum", 1)], 53),
        # the second Vlan tag: absent in untagged and single-tagged packets
        "absent_header": noisy(mixed, [spec("Vlan", "vid", 1), spec("Vxlan", "vni"), spec("ARP", "opcode")], 54),
        # b shorter than a: the cut falls inside the ignored field of some packets (result LEN)
        "cut_field": noisy(mixed, [spec("IPv6", "src"), spec("IPv4", "src")], 55,
                           cut=lambda i, ln: ln if i % 3 else min(ln, 27 + i % 9)),
        "overlapping": noisy(mixed, [("IPv4", 0, 60, 75), ("IPv4", 0, 64, 71), ("IPv4", 0, 70, 90), ("Ether", 0, 40, 130)], 56),
        # 16 specs: the 12 fields of IPv4, and ranges that run past the header (any width is allowed): over
        # many 16-byte chunks of the long packet, and past every packet's end
        "sixteen": noisy(mixed, ipv4_all + [spec("TCP", "seq_no"), ("TCP", 0, 150, 30000), ("UDP", 0, 48, 65535),
                                            spec("Ether", "src")], 57),
    }
    assert len(cs["sixteen"]["ignore"]) == 16
    return cs


def plain_cases():
    cs = {f"tiling_{n}": tiling(n) for n in (1, 63, 64, 65, 1025, 4099)}
    cs["long_among_short"] = long_among_short()
    cs["clamped_indexed"], cs["clamped_fixed"] = clamped()
    cs["length_mismatch"] = length_mismatch()
    e = batch(np.zeros(0, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint32))
    cs["empty_batch"] = case(e, e)
    same = batch(gen.gen_c2(100, seed=3), stride=64)
    cs["same_buffer"] = case(same, same)
    return cs


_CASES = None


def all_cases():
    """name -> (case, expected): built once and shared; nothing may change them."""
    global _CASES
    if _CASES is None:
        cs = dict(plain_cases(), **ignore_cases())
        _CASES = {k: (c, expect(c)) for k, c in cs.items()}
    return _CASES


CASE_NAMES = ["tiling_1", "tiling_63", "tiling_64", "tiling_65", "tiling_1025", "tiling_4099", "long_among_short",
              "clamped_indexed", "clamped_fixed", "length_mismatch", "empty_batch", "same_buffer", "straddle",
              "ipv6_src", "occurrence_1", "absent_header", "cut_field", "overlapping", "sixteen"]
