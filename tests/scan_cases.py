"""pkt_scan_batch's yardstick and case list, shared by test_scan_host.py (pkt_scan_create_host) and
test_scan_device.py (the kernel).

The model builds no trie.  For every start position of a packet's region and every distinct pattern length it takes
the slice of that length and looks it up in a dict keyed by the patterns of that length (one dict for the exact
patterns, one for the NOCASE ones, whose keys and slices go through bytes.lower(), which changes ASCII letters
only), so it shares no construction with either implementation.  The region, the clamp and the statuses are
re-stated here from include/pktgpu.h.

A case is a dict: pats (list of (bytes, nocase, group, action)), default, batch (compare_cases.batch), region
("packet" / "payload"), chain (slot-major numpy columns, or None) and select (uint8 [n] or None).
"""
import numpy as np

from pktgpu import schema

import compare_cases as C

MISS, HIT, SKIPPED, NO_CHAIN, SPAN = range(5)
NONE = 0xFFFFFFFF
OUTPUTS = (("status", np.uint8), ("pat", np.uint32), ("off", np.uint16), ("action", np.uint32), ("sel", np.uint8),
           ("count", np.uint32), ("matched", np.uint64))
STAGE = 1024  # the bytes of the flattened chunk list a wave of the kernel stages per step (64 chunks of 16)


def pat(b, nocase=False, group=0, action=1):
    return (b.encode() if isinstance(b, str) else bytes(b), bool(nocase), group, action)


def case(pats, batch, region="packet", chain=None, select=None, default=0):
    return dict(pats=[p if isinstance(p, tuple) else pat(p) for p in pats], batch=batch, region=region, chain=chain,
                select=None if select is None else np.asarray(select, np.uint8), default=default)


def tables(pats):
    """(blob, table) as pktgpu.scan_patterns gives them, straight from the case's tuples."""
    tab = np.zeros(len(pats), schema.SCAN_PATTERN_DTYPE)
    at = 0
    for k, (b, nc, g, a) in enumerate(pats):
        tab[k] = (at, len(b), schema.SCAN_NOCASE if nc else 0, g, a, 0)
        at += len(b)
    return np.frombuffer(b"".join(p[0] for p in pats), np.uint8), tab


def region_of(c, i, length):
    """(status, r0) of packet i by the header's rule; status MISS = scanned."""
    if c["select"] is not None and not c["select"][i]:
        return SKIPPED, 0
    if c["region"] == "packet":
        return MISS, 0
    ch = c["chain"]
    nh = int(ch["n_hdrs"][i])
    if nh == 0:
        return NO_CHAIN, 0
    r0 = 0
    for j in range(min(nh, schema.MAX_HDRS)):
        t = int(ch["hdr_type"][j, i])
        if not 1 <= t <= 21:
            return SPAN, 0
        r0 = max(r0, int(ch["hdr_off"][j, i]) + schema.HDR_SIZES[t])
    return (SPAN, 0) if r0 > length else (MISS, r0)


def expect(c):
    """Every output of the case and the counters a call adds, from the definition."""
    pats, n = c["pats"], c["batch"]["n"]
    by_len = {}  # length -> (exact dict, nocase dict): slice -> [pattern indexes]
    for k, (b, nc, _, _) in enumerate(pats):
        d = by_len.setdefault(len(b), ({}, {}))
        d[1 if nc else 0].setdefault(b.lower() if nc else b, []).append(k)
    lengths = sorted(by_len)
    out = {k: np.zeros(n, dt) for k, dt in OUTPUTS}
    out["pat"][:] = NONE
    hits = np.zeros(len(pats) + 1, np.uint64)
    slab = c["batch"]["slab"]
    for i, (o, ln) in enumerate(C.extents(c["batch"])):
        st, r0 = region_of(c, i, ln)
        out["status"][i] = st
        out["action"][i] = 0 if st == SKIPPED else c["default"]
        if st != MISS:
            continue
        data = slab[o:o + ln].tobytes()
        first = {}  # pattern -> its smallest s
        count = 0
        for L in lengths:
            ex, nc = by_len[L]
            low = data.lower() if nc else None
            for s in range(r0, ln - L + 1):
                for p in ex.get(data[s:s + L], ()) if ex else ():
                    first.setdefault(p, s)
                    hits[p] += 1
                    count += 1
                for p in nc.get(low[s:s + L], ()) if nc else ():
                    first.setdefault(p, s)
                    hits[p] += 1
                    count += 1
        if not first:
            hits[len(pats)] += 1
            continue
        p = min(first)
        out["status"][i], out["pat"][i], out["off"][i], out["count"][i] = HIT, p, first[p], count
        out["action"][i] = pats[p][3]
        m = 0
        for q in first:
            m |= 1 << pats[q][2]
        out["matched"][i] = m
    out["sel"][:] = out["action"] != 0
    out["hits"] = hits
    return out


def check(got, want, label=""):
    for k in want:
        if k not in got or got[k] is None:
            continue
        g, w = np.asarray(got[k]), want[k]
        assert g.shape == w.shape, (label, k, g.shape, w.shape)
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, (label, k, "first bad", bad[:8], g[bad[:8]], w[bad[:8]])


# ------------------------------------------------------------------ layouts and texts
def fixed(pkts, stride, lens=False, tail=0):
    """Fixed stride; lens=False needs every packet to be `stride` long."""
    slab = np.zeros(len(pkts) * stride + tail, np.uint8)
    for k, p in enumerate(pkts):
        assert len(p) <= stride and (lens or len(p) == stride)
        slab[k * stride:k * stride + len(p)] = np.frombuffer(p, np.uint8)
    return C.batch(slab, None, [len(p) for p in pkts] if lens else None, stride, len(pkts))


def packed(pkts, lead=0):
    """Indexed, the packets end to end with nothing between them; the last ends at the slab's last byte."""
    offs = np.cumsum([lead] + [len(p) for p in pkts])[:-1]
    return C.batch(np.frombuffer(b"\0" * lead + b"".join(pkts), np.uint8), offs, [len(p) for p in pkts])


def text(rng, n, alphabet=b"abcd"):
    return bytes(rng.choice(np.frombuffer(alphabet, np.uint8), n).tolist())


def ether_chain(n, nh=1):
    """A forged chain: one Ether entry at 0 for every packet (r0 = 14)."""
    ty = np.zeros((schema.MAX_HDRS, n), np.uint8)
    ty[0] = schema.HDR_ID["Ether"]
    return dict(n_hdrs=np.full(n, nh, np.uint8), hdr_type=ty, hdr_off=np.zeros((schema.MAX_HDRS, n), np.uint16))


P64 = bytes(range(0xC0, 0x100))  # a 64-byte pattern no text over "abcd" holds a part of
FAMILY = ["a", "ab", "abc", "abcd"]


def sizes_cases(rng):
    pats = [pat("abca"), pat("dd", group=3, action=7), pat("CAB", nocase=True, group=5, action=0), pat("b")]
    out = {}
    for n in (1, 63, 64, 65, 257):
        out["n%d_fixed" % n] = case(pats, fixed([text(rng, 48) for _ in range(n)], 48), default=9)
        pk = [text(rng, int(rng.integers(0, 90))) for _ in range(n)]
        out["n%d_lens" % n] = case(pats, fixed(pk, 96, lens=True))
        out["n%d_indexed" % n] = case(pats, C.indexed(pk, rng))
    return out


def layout_cases(rng):
    out = {}
    pats = [pat("abcd"), pat("dcba", group=1), pat("AbAb", nocase=True, group=2)]
    pk = [text(rng, 40 + k) for k in range(48)]
    out["every_alignment"] = case(pats, C.indexed(pk, rng, align=[k % 16 for k in range(48)]))
    # adjacent packets of a packed slab spell a pattern across their boundary: no occurrence
    halves = []
    for k in range(40):
        cut = 1 + k % 7
        halves += [b"xxxx" + b"needle!!"[:cut], b"needle!!"[cut:] + b"yy"]
    out["packed_boundary"] = case([pat("needle!!"), pat("!!xx"), pat("yyxx")], packed(halves, lead=3))
    out["empty_packets"] = case(pats + [pat("a")], packed([b"", b"a", b"", b"", text(rng, 30), b""] * 12))
    pk = [b"\x11" * 14 + text(rng, k % 5) for k in range(70)]
    out["r0_equals_r1"] = case(pats + [pat("\x11")], packed(pk), "payload", ether_chain(70))
    big = bytearray(text(rng, 65535))
    big[-64:] = P64
    out["one_65535"] = case([pat(P64, action=5)], C.indexed([bytes(big)], rng, align=[5]))
    out["long_among_short"] = case([pat(P64), pat("abcdabcd")], C.indexed([text(rng, 20)] * 30 + [bytes(big)] + [text(rng, 33)] * 40, rng))
    return out


def position_cases(rng):
    out = {}
    hdr = b"\x22" * 14
    # at r0, ending at r1, one byte short
    pk = [hdr + b"abcde" + text(rng, 20, b"xy"), hdr + text(rng, 20, b"xy") + b"abcde", hdr + text(rng, 21, b"xy") + b"abcd",
          hdr[:10] + b"abcde", b"abcde" + hdr + b"xyxy"]
    for region in ("packet", "payload"):
        out["edges_" + region] = case([pat("abcde"), pat("\x22\x22\x22", group=9)], packed(pk * 13), region, ether_chain(65))
    # a 64-byte pattern at every offset 0..79 of a packet, the packets at every alignment: every chunk boundary
    pk = []
    for k in range(80):
        p = bytearray(text(rng, 160))
        p[k:k + 64] = P64
        pk.append(bytes(p))
    out["p64_every_chunk_boundary"] = case([pat(P64, group=63, action=0xFFFFFFFF)], C.indexed(pk, rng, align=[(3 * k) % 16 for k in range(80)]))
    # the wave's staging boundary: stride 2 * STAGE, so every packet starts a staging step and its byte STAGE is the
    # next step's first; the pattern starts at STAGE - 63 .. STAGE
    pk = []
    for k in range(65):
        p = bytearray(text(rng, 2 * STAGE))
        p[STAGE - 63 + (k % 64):STAGE + 1 + (k % 64)] = P64
        p[2 * STAGE - 64:] = P64 if k % 2 else p[2 * STAGE - 64:]
        pk.append(bytes(p))
    out["staging_boundary"] = case([pat(P64), pat(P64[:17], group=1), pat(P64[40:], group=2)], fixed(pk, 2 * STAGE))
    long = bytearray(text(rng, 5 * STAGE + 77))
    for k in range(1, 6):
        long[k * STAGE - 3 - 7 * k:k * STAGE - 3 - 7 * k + 64] = P64
    out["staging_boundary_one_packet"] = case([pat(P64), pat(P64[:40])], C.indexed([bytes(long)], rng, align=[0]))
    return out


def pattern_cases(rng):
    out = {}
    pk = [text(rng, int(rng.integers(0, 200))) for _ in range(70)]
    b = C.indexed(pk, rng)
    out["one_byte"] = case([pat("c", group=7, action=3)], b)
    out["family"] = case([pat(f, group=k, action=10 + k) for k, f in enumerate(FAMILY)], b)
    out["family_reversed"] = case([pat(f, group=k, action=10 + k) for k, f in enumerate(reversed(FAMILY))], b)
    out["duplicates"] = case([pat("abc", group=1, action=0), pat("abc", group=2, action=5), pat("abc", nocase=True, group=3, action=6),
                              pat("ABC", nocase=True, group=4)], b)
    out["aa_in_aaaa"] = case(["aa"], packed([b"aaaa", b"aaa", b"aa", b"a", b""]))
    http = [b"GET / HTTP/1.1", b"get /x", b"Get it", b"gEt", b"GE", b"xxGETxGET /", b"POST /GET", b"[GET /]{get}"]
    out["nocase_mix"] = case([pat("Get"), pat("get", nocase=True, group=1), pat("GET /", group=2), pat("[get", nocase=True, group=3),
                              pat("{GET", nocase=True, group=4), pat("z@[`{", nocase=True, group=5)], packed(http * 9 + [b"Z@[`{", b"z@;`{"]))
    binp = [b"\x00", b"\xff\xff", b"\x00\xff\x00", b"\xff\x00\x00\x00"]
    out["bytes_00_ff"] = case([pat(x, group=k) for k, x in enumerate(binp)],
                              C.indexed([text(rng, int(rng.integers(0, 64)), b"\x00\xff") for _ in range(66)], rng))
    p = bytearray(text(rng, 300))
    p[100:164] = P64
    out["one_64_byte"] = case([pat(P64)], packed([bytes(p), bytes(p[:163]), bytes(p[101:]), bytes(p[100:164])]))
    out["npats_0"] = case([], b, default=4)
    return out


def limits_case(rng, n=257):
    """8192 patterns, 131072 bytes: 16 random bytes each, a quarter NOCASE; some planted."""
    raw = rng.integers(0, 256, (schema.SCAN_MAX_PATTERNS, 16), dtype=np.uint8)
    raw[1::2, :2] = raw[0::2, :2]  # shared prefixes
    pats = [pat(raw[k].tobytes(), nocase=k % 4 == 3, group=k % 64, action=k) for k in range(schema.SCAN_MAX_PATTERNS)]
    pk = []
    for i in range(n):
        p = bytearray(rng.integers(0, 256, int(rng.integers(0, 120)), dtype=np.uint8).tobytes())
        for _ in range(i % 3):
            k = int(rng.integers(0, len(pats)))
            at = int(rng.integers(0, max(1, len(p) - 16)))
            p[at:at + 16] = pats[k][0].swapcase() if pats[k][1] else pats[k][0]
        pk.append(bytes(p))
    return case(pats, C.indexed(pk, rng), default=1 << 31)


def status_cases(rng):
    out = {}
    n = 130
    pk = [b"\x33" * 14 + text(rng, int(rng.integers(0, 40))) for _ in range(n)]
    ch = ether_chain(n)
    sel = np.ones(n, np.uint8)
    for i in range(n):
        k = i % 10
        if k == 3:
            sel[i] = 0
        elif k == 4:
            ch["n_hdrs"][i] = 0
        elif k == 5:
            ch["hdr_type"][0, i] = (0, 22, 255)[i % 3]                 # outside 1..21
        elif k == 6:
            ch["hdr_off"][0, i] = len(pk[i]) - 13                      # r0 = r1 + 1
        elif k == 7:
            ch["n_hdrs"][i] = 255                                      # cut to 16 entries: rows 1.. hold type 0
        elif k == 8:
            ch["n_hdrs"][i], ch["hdr_type"][1, i], ch["hdr_off"][1, i] = 2, schema.HDR_ID["Vlan"], 2   # the maximum, not the last
    out["five_statuses"] = case([pat("ab", action=2), pat("cd", group=1, action=0)], packed(pk), "payload", ch, sel, default=6)
    out["select_packet"] = case([pat("ab"), pat("\x33", group=2)], packed(pk), "packet", None, sel)
    return out


def gre_no_inner():
    """Ether / IPv4 / GRE with checksum, key and sequence number and a protocol no parser takes: the list ends with
    the wire-EARLIEST option (quirk Q2), the payload starts after the wire-latest."""
    import edit_cases as E
    p = bytearray(E.gre_options()[:50])
    p[36:38] = b"\x12\x34"
    return bytes(p) + b"payload-abcd"


def real_chain_cases(rng):
    import match_cases as M
    out = {}
    pats = [pat("\x00\x00", group=1), pat("a"), pat("\x08\x00", group=2), pat("E", nocase=True, group=3), pat("abcd", group=4)]
    for name, pkts in (("ref22", C.packets(M.ref22_batch())), ("mix", M.random_mix(rng, 150) + [gre_no_inner()])):
        b = C.indexed(pkts, rng)
        out["real_" + name] = case(pats, b, "payload", C.chain_of(b))
    return out


def random_differential(seed=5, n=2000):
    """The issue's differential: packets of 0..300 bytes over "abcd" in mixed case, 24 patterns of 5..9 bytes, half
    of them NOCASE."""
    rng = np.random.default_rng(seed)
    pats = [pat(text(rng, int(rng.integers(5, 10))), nocase=k % 2 == 1, group=k % 7, action=k % 5) for k in range(24)]
    pk = []
    for _ in range(n):
        t = np.frombuffer(text(rng, int(rng.integers(0, 301))), np.uint8).copy()
        up = rng.integers(0, 8, t.size) == 0
        t[up] -= 0x20
        pk.append(t.tobytes())
    return case(pats, C.indexed(pk, rng), default=3)


_CACHE = {}


def all_cases():
    """{name: case}, built once; expect() results are cached by expected()."""
    if "cases" not in _CACHE:
        rng = np.random.default_rng(20)
        cs = {}
        for f in (sizes_cases, layout_cases, position_cases, pattern_cases, status_cases, real_chain_cases):
            cs.update(f(rng))
        cs["limits"] = limits_case(rng)
        _CACHE["cases"] = cs
    return _CACHE["cases"]


NAMES = (["n%d_%s" % (n, k) for n in (1, 63, 64, 65, 257) for k in ("fixed", "lens", "indexed")] +
         ["every_alignment", "packed_boundary", "empty_packets", "r0_equals_r1", "one_65535", "long_among_short",
          "edges_packet", "edges_payload", "p64_every_chunk_boundary", "staging_boundary", "staging_boundary_one_packet",
          "one_byte", "family", "family_reversed", "duplicates", "aa_in_aaaa", "nocase_mix", "bytes_00_ff", "one_64_byte",
          "npats_0", "five_statuses", "select_packet", "real_ref22", "real_mix", "limits"])


def expected(name):
    key = ("want", name)
    if key not in _CACHE:
        _CACHE[key] = expect(all_cases()[name])
    return _CACHE[key]


def host_call(c, want=None, hits=True):
    """The case through pkt_scan_create_host / pkt_scan_batch -> (outputs dict with "hits", info)."""
    import pktgpu
    sc = pktgpu.Scanner(None, tables(c["pats"]), default=c["default"])
    r = sc.run(c["batch"], c["chain"], c["region"], c["select"], **({} if want is None else {"want": want}), hits=hits)
    info = sc.info
    sc.close()
    return {k: getattr(r, k) for k, _ in OUTPUTS + (("hits", None),)}, info
