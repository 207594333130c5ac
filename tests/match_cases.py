"""Batches, rule programs and expected results shared by test_match_host.py and test_match_device.py.

The yardstick is independent of the library: `Evaluator` reads packet bytes and chain rows and applies the
contract of include/pktgpu.h (the pkt_match section) with Python ints, pyref.bit_range_py for the field values and
pyref.parse (through l4_cases.chain_of) for the chains.  Nothing here calls pkt_match_host or the device.  A
program is a dict(terms=[(hdr_type, occurrence, start, end, op, flags, a, b)], rules=[(first_term, nterms,
action)], default=action): the C structs' members as plain tuples, so shared and overlapping term ranges can be
written down; `nested` builds one from [(action, [term, ...])].
"""
import os
import struct

import numpy as np

from pktgpu import fields, gen, schema

import compare_cases as C
import edit_cases as E
import flow_cases as F
import l4_cases as L4
import pktgen_templates as T
import pyref
from compare_cases import batch, extents, indexed

HAS, EQ, RANGE, LEN = range(4)
NOT = 1
NONE = 0xFF
M64 = (1 << 64) - 1
HID = schema.HDR_ID
SIZES = schema.HDR_SIZES


# ------------------------------------------------------------------ programs
def term(hdr, occ, field, op, a=0, b=None, neg=False):
    """A term tuple.  field: a name of pktgpu.fields, a (start, end) pair, or None (HAS)."""
    t = HID[hdr] if isinstance(hdr, str) else hdr
    s, e = (0, 0) if field is None else fields.FIELDS[t][field] if isinstance(field, str) else field
    if b is None:
        b = M64 if op == EQ else a
    return (t, occ, s, e, op, NOT if neg else 0, a & M64, b & M64)


def has(hdr, occ=0, neg=False):
    return term(hdr, occ, None, HAS, 0, 0, neg)


def length(lo, hi, neg=False):
    return (0, 0, 0, 0, LEN, NOT if neg else 0, lo, hi)


def nested(rules, default=0):
    terms, rr = [], []
    for action, tl in rules:
        rr.append((len(terms), len(tl), action))
        terms.extend(tl)
    return dict(terms=terms, rules=rr, default=default)


def to_ctypes(prog):
    """(PktMatchTerm array, PktMatchRule array): what pktgpu.match and Parser.match_program take as they are."""
    from pktgpu import _lib
    ta = (_lib.PktMatchTerm * max(1, len(prog["terms"])))(*[
        _lib.PktMatchTerm(_lib.PktFieldSpec(t, occ, s, e, 0), op, fl, 0, 0, a, b) for t, occ, s, e, op, fl, a, b in prog["terms"]])
    ra = (_lib.PktMatchRule * max(1, len(prog["rules"])))(*[_lib.PktMatchRule(*r) for r in prog["rules"]])
    if not prog["terms"]:
        ta = (_lib.PktMatchTerm * 0)()
    if not prog["rules"]:
        ra = (_lib.PktMatchRule * 0)()
    return ta, ra


# ------------------------------------------------------------------ the yardstick
class Evaluator:
    """One batch and chain; run(prog) -> the six outputs and the (op, NOT, raw) triples that occurred."""

    def __init__(self, b, ch):
        self.b, self.n = b, b["n"]
        self.ext = extents(b)
        self.pk = [b["slab"][o:o + ln].tobytes() for o, ln in self.ext]
        self.rows = [F.chain_rows(ch, i) for i in range(self.n)]
        self.memo = {}

    def header(self, i, t, occ):
        """The offset of packet i's occ-th header of type t when it is present, else None."""
        at = [o for ty, o in self.rows[i] if ty == t]
        if occ >= len(at) or at[occ] + SIZES[t] > self.ext[i][1]:
            return None
        return at[occ]

    def raw(self, i, tm):
        t, occ, s, e, op, fl, a, b = tm
        if op == LEN:
            return a <= self.ext[i][1] <= b
        key = (i, t, occ, s, e, op == HAS)
        if key not in self.memo:
            ho = self.header(i, t, occ)
            self.memo[key] = None if ho is None else True if op == HAS else pyref.bit_range_py(self.pk[i][ho:ho + SIZES[t]], s, e)
        v = self.memo[key]
        if v is None:
            return False
        if op == HAS:
            return True
        if op == EQ:
            return ((v ^ a) & b & ((1 << (e - s + 1)) - 1)) == 0
        return a <= v <= b

    def run(self, prog):
        n, nr = self.n, len(prog["rules"])
        res = dict(rule=np.zeros(n, np.uint8), action=np.zeros(n, np.uint32), select=np.zeros(n, np.uint8),
                   matched=np.zeros(n, np.uint64), hits=np.zeros(nr + 1, np.uint64), bytes=np.zeros(nr + 1, np.uint64))
        cover = set()
        for i in range(n):
            tv = {}
            bits = 0
            for r, (f0, k, _) in enumerate(prog["rules"]):
                ok = True
                for q in range(f0, f0 + k):  # every term, no short cut: the coverage counts them all
                    if q not in tv:
                        tm = prog["terms"][q]
                        rw = self.raw(i, tm)
                        cover.add((tm[4], tm[5], rw))
                        tv[q] = rw != bool(tm[5] & NOT)
                    ok = ok and tv[q]
                if ok:
                    bits |= 1 << r
            first = (bits & -bits).bit_length() - 1 if bits else NONE
            act = prog["rules"][first][2] if bits else prog["default"]
            res["rule"][i], res["action"][i], res["select"][i], res["matched"][i] = first, act, act != 0, bits
            res["hits"][nr if first == NONE else first] += 1
            res["bytes"][nr if first == NONE else first] += self.ext[i][1]
        res["cover"] = cover
        return res


OUT = ("rule", "action", "select", "matched", "hits", "bytes")


def check(got, want, label=""):
    for name in OUT:
        if got.get(name) is None:
            continue
        g = np.asarray(got[name])
        assert g.shape == want[name].shape, (label, name, g.shape, want[name].shape)
        bad = np.flatnonzero(g != want[name])
        assert bad.size == 0, (label, name, "first bad", bad[:8], g[bad[:8]], want[name][bad[:8]])


# ------------------------------------------------------------------ packets
SRC = ["10.1.%d.7" % k for k in range(4)]
DST = ["172.16.%d.9" % k for k in range(4)]
DPORTS = [53, 80, 443, 8080]


def ip4(s):
    return struct.unpack(">I", bytes(int(x) for x in s.split(".")))[0]


def special_packets(rng):
    """Every shape the issue lists, a few of each."""
    out = []
    for l4 in ("TCP", "UDP", "ICMP"):
        for v6 in (False, True):
            for vlans in (0, 1, 2):
                out.append(L4.pkt(l4, v6, vlans=vlans, payload=L4.rnd(rng, int(rng.integers(0, 40))),
                                  sport=int(rng.integers(1024, 65536)), dport=DPORTS[int(rng.integers(0, 4))],
                                  frag=0x4000 if vlans else 0x2000))
    out += [F.vxlan(rng, i) for i in range(3)]                     # inner IPv4 at 64, inner TCP at 84: past 80 bytes
    ip = bytes(gen.reference_22_packets()[0].to_vec())[14:]
    out.append(E.tagged(10, ip, last=0x0800))                      # Ether + 10 Vlan: IPv4 at slot 11, TCP at 12
    out.append(E.sixteen_headers())
    out.append(E.eth(0x8847) + b"".join(struct.pack(">I", (100 + k) << 12 | (0x100 if k == 9 else 0) | 64) for k in range(10))
               + ip)                                               # an MPLS stack 10 deep
    out.append(E.gre_options())
    out.append(bytes(T.template_bytes("greip4")))
    out.append(bytes(T.template_bytes("arp_req")))
    out.append(bytes(T.template_bytes("tcp"))[:20])                # truncated: n_hdrs 0
    return out


def random_mix(rng, n):
    sp = special_packets(rng)
    out = []
    for k in range(n):
        if k % 10 == 9:
            out.append(sp[int(rng.integers(0, len(sp)))])
            continue
        l4 = ("TCP", "UDP", "ICMP")[int(rng.integers(0, 3))] if k % 7 else "UDP"
        v6 = k % 5 == 4
        out.append(L4.pkt(l4, v6, vlans=int(rng.integers(0, 3)), payload=L4.rnd(rng, int(rng.integers(0, 30))),
                          sport=int(rng.integers(1000, 1100)) if k % 3 else int(rng.integers(1, 65536)),
                          dport=DPORTS[int(rng.integers(0, 4))],
                          src=None if v6 else SRC[int(rng.integers(0, 4))], dst=None if v6 else DST[int(rng.integers(0, 4))]))
    return out


def ref22_batch():
    buf = np.fromfile(os.path.join(C.GOLD, "ref22.pcap"), np.uint8)
    offs, lens, at = [], [], 24
    while at + 16 <= buf.size:
        ln = struct.unpack_from("<I", buf, at + 8)[0]
        offs.append(at + 16)
        lens.append(ln)
        at += 16 + ln
    assert len(offs) == 22
    return batch(buf, offs, lens)


# ------------------------------------------------------------------ hand-written programs
def acl():
    """A 16-rule 5-tuple ACL: rule s + 4 d takes SRC[s]/24 -> DST[d]/24 (rule 15: any destination), TCP on even
    rules and UDP on odd ones, source ports 1000..65535, destination ports 0..1023 (8080 falls through)."""
    rules = []
    for r in range(16):
        s, d = r % 4, r // 4
        rules.append((100 + r if r % 3 else 0,  # some rules drop (action 0)
                      [term("IPv4", 0, "src", EQ, ip4(SRC[s]), 0xFFFFFF00),
                       term("IPv4", 0, "dst", EQ, ip4(DST[d]), 0 if r == 15 else 0xFFFFFF00),
                       term("IPv4", 0, "protocol", EQ, 6 if r % 2 == 0 else 17),
                       term("TCP" if r % 2 == 0 else "UDP", 0, "src", RANGE, 1000, 65535),
                       term("TCP" if r % 2 == 0 else "UDP", 0, "dst", RANGE, 0, 1023)]))
    return nested(rules, default=7)


def refs30():
    """30 distinct (hdr_type, occurrence) references, numbered in order of first appearance: the first 16 (rules
    0-3) are the ones a kernel may resolve up front, the rest (rules 4-9) come when a term first names them:
    after earlier rules have failed or matched lanes, some deeper than chain slot 4 (Vlan 9-12, MPLS 5 and 9, a
    VXLAN packet's inner Ether / IPv4 / TCP), twice in a row, alternating, and again in a later rule."""
    return nested([
        (1, [has("Dot3"), has("LLC"), has("SNAP"), has("STP")]),
        (2, [has("GRE"), has("GREKey"), has("GRESequenceNum"), has("GREChksumOffset")]),
        (3, [has("ERSPAN2", 0, True), has("ERSPAN3", 0, True), has("ERSPANPLATFORM", 0, True), has("ARP")]),
        (4, [term("Vlan", 0, "vid", RANGE, 0, 4095), has("Vlan", 1), has("Vlan", 2), has("Vlan", 3), length(200, 65535)]),
        (5, [term("Vlan", 9, "vid", EQ, 109), term("Vlan", 9, "etype", EQ, 0x0800)]),
        (6, [term("MPLS", 9, "bos", EQ, 1), term("MPLS", 5, "label", RANGE, 0, (1 << 20) - 1), term("MPLS", 9, "ttl", EQ, 64)]),
        (7, [term("IPv4", 1, "ttl", RANGE, 1, 255), term("Ether", 1, "etype", EQ, 0x0800), term("TCP", 0, "dst", RANGE, 0, 65535),
             term("Vxlan", 0, "vni", RANGE, 0, (1 << 24) - 1), term("UDP", 0, "dst", EQ, 4789)]),
        (8, [has("Vlan", 12), term("Vlan", 10, "vid", RANGE, 100, 120), has("Vlan", 11)]),
        (9, [term("IPv6", 0, (64, 127), EQ, 0xAAAA << 48), has("ICMP", 0, True), has("IPv4", 0, True)]),
        (10, [term("IPv4", 0, "protocol", EQ, 17), term("UDP", 0, "dst", RANGE, 0, 1023), term("Vlan", 9, "vid", EQ, 109, neg=True)]),
    ], default=0)


def hand_programs(ref_len):
    """name -> program.  ref_len: a packet length that occurs, for the LEN edges."""
    P = {}
    P["no_rules"] = nested([], default=5)
    P["zero_term_rule"] = nested([(0, [has("ARP")]), (9, [])], default=3)
    for neg in (False, True):
        s = "_not" if neg else ""
        P["has" + s] = nested([(1, [has("TCP", 0, neg)]), (2, [has("Vlan", 1, neg)]), (3, [has("IPv4", 1, neg)])])
        P["eq" + s] = nested([(1, [term("IPv4", 0, "protocol", EQ, 17, neg=neg)]),
                              (2, [term("IPv4", 0, "src", EQ, ip4(SRC[1]), 0xFFFFFF00, neg=neg)]),
                              (3, [term("Ether", 0, "etype", EQ, 0x8100, neg=neg)])], default=0)
        P["range" + s] = nested([(1, [term("UDP", 0, "dst", RANGE, 50, 100, neg=neg)]),
                                 (2, [term("TCP", 0, "src", RANGE, 1024, 40000, neg=neg)])], default=4)
        P["len" + s] = nested([(1, [length(ref_len, ref_len, neg)]), (2, [length(0, ref_len - 1, neg)]),
                               (3, [length(ref_len + 1, 65535, neg)]), (4, [length(ref_len - 1, ref_len + 1, neg)])])
    P["edges"] = nested([
        (1, [term("IPv4", 0, (49, 49), EQ, 1)]),                       # a 1-bit field: DF
        (2, [term("IPv4", 0, (50, 50), EQ, 1)]),                       # MF
        (3, [term("Ether", 0, "dst", EQ, int.from_bytes(gen.to_mac_bytes(E.M1), "big"))]),   # a 48-bit MAC
        (4, [term("Ether", 0, (4, 67), EQ, int.from_bytes(gen.to_mac_bytes(E.M1) + gen.to_mac_bytes(E.M2), "big") >> 28 & M64)]),
        (5, [term("Ether", 0, (4, 67), RANGE, 0, M64 >> 1)]),          # 64 bits off a byte boundary: nine bytes
        (6, [term("IPv6", 0, (64, 127), EQ, 0xAAAA << 48), term("IPv6", 0, (128, 191), EQ, 1)]),  # both halves of AAAA::1
        (7, [term("IPv6", 0, (192, 255), EQ, 0xBBBB << 48)]),          # a /64 prefix
        (8, [term("Vlan", 1, "vid", EQ, 11)]),                         # occurrence 1: the second Vlan
        (9, [term("IPv4", 1, "ttl", RANGE, 1, 255)]),                  # the inner IPv4
        (10, [term("TCP", 0, "dst", EQ, 0, 0)]),                   # an EQ with mask 0: present
        (11, [term("UDP", 0, "dst", RANGE, 443, 443)]),                # lo == hi
        (12, [term("UDP", 0, "dst", RANGE, 444, 443)]),                # lo > hi: never
        (13, [term("UDP", 0, "dst", RANGE, 444, 443, neg=True)]),      # ... and its NOT: always
    ])
    P["deep"] = nested([(1, [term("Vlan", 9, "vid", EQ, 109)]), (2, [term("MPLS", 9, "bos", EQ, 1)]),
                        (3, [term("Vlan", 12, "vid", RANGE, 0, 4095)]), (4, [term("IPv4", 0, "ttl", RANGE, 0, 255), has("Vlan", 5)]),
                        (5, [has("Vxlan"), term("TCP", 0, "dst", RANGE, 0, 65535)]),  # the VXLAN packets' inner TCP, at byte 84
                        (6, [has("GREKey"), term("GREKey", 0, (0, 31), EQ, 77)]), (7, [has("GRE")])])
    P["stp_last_bit"] = nested([(1, [term("STP", 0, (279, 279), EQ, 1)]), (2, [term("STP", 0, (279, 279), EQ, 0)])])
    P["first_match_order"] = nested([(1, [has("IPv4")]), (2, [has("TCP")]), (3, [has("Ether")]), (0, [has("UDP")])], default=8)
    # 64 rules, rule 63 set for most packets; 256 terms; rules that share terms and overlap
    t256 = [term("UDP", 0, "dst", RANGE, 0, 65535 - k) for k in range(200)] + [has("Ether")] * 55 + [has("IPv4", 0, True)]
    P["terms256"] = dict(terms=t256, rules=[(0, 200, 1), (200, 56, 2), (199, 2, 3), (0, 256, 4), (255, 1, 5)], default=0)
    r64 = [(1000 + r, [term("IPv4", 0, "ttl", RANGE, r, 64 + r)] if r < 63 else [has("Ether")]) for r in range(64)]
    P["rules64"] = nested(r64)
    sh = [has("IPv4"), term("IPv4", 0, "protocol", EQ, 6), has("TCP"), term("TCP", 0, "dst", EQ, 80), has("Vlan")]
    P["shared_terms"] = dict(terms=sh, rules=[(0, 4, 1), (0, 2, 2), (1, 3, 3), (4, 1, 4), (0, 1, 5), (0, 5, 6)], default=0)
    P["acl"] = acl()
    P["refs30"] = refs30()
    return P


def random_program(rng, ev):
    """A program whose values come from the batch itself, so that terms are sometimes true."""
    pool = [("IPv4", 0, "src"), ("IPv4", 0, "dst"), ("IPv4", 0, "protocol"), ("IPv4", 0, "ttl"), ("IPv4", 1, "src"),
            ("IPv6", 0, (64, 127)), ("IPv6", 0, "next_hdr"), ("TCP", 0, "src"), ("TCP", 0, "dst"), ("UDP", 0, "dst"),
            ("UDP", 0, "src"), ("Vlan", 0, "vid"), ("Vlan", 1, "vid"), ("Ether", 0, "etype"), ("Ether", 0, (4, 67)),
            ("ICMP", 0, "icmp_type"), ("TCP", 1, "dst"), ("Vxlan", 0, "vni"), ("MPLS", 3, "label")]
    rules = []
    for _ in range(int(rng.integers(1, 24))):
        tl = []
        for _ in range(int(rng.integers(0, 5))):
            kind, neg = int(rng.integers(0, 4)), bool(rng.integers(0, 4) == 0)
            if kind == LEN:
                lo = int(rng.integers(0, 120))
                tl.append(length(lo, lo + int(rng.integers(0, 60)), neg))
                continue
            hdr, occ, f = pool[int(rng.integers(0, len(pool)))]
            if kind == HAS:
                tl.append(has(hdr, occ, neg))
                continue
            s, e = fields.FIELDS[HID[hdr]][f] if isinstance(f, str) else f
            v = None
            for _ in range(8):  # a value some packet holds
                i = int(rng.integers(0, ev.n))
                ho = ev.header(i, HID[hdr], occ)
                if ho is not None:
                    v = pyref.bit_range_py(ev.pk[i][ho:ho + SIZES[HID[hdr]]], s, e)
                    break
            v = int(rng.integers(0, 1 << 16)) if v is None else v
            w = e - s + 1
            if kind == EQ:
                mask = M64 if rng.integers(0, 2) else (M64 << int(rng.integers(0, w + 1))) & M64
                tl.append(term(hdr, occ, (s, e), EQ, v ^ (int(rng.integers(0, 4)) == 0), mask, neg))
            else:
                d = int(rng.integers(0, 1 << min(w, 12)))
                tl.append(term(hdr, occ, (s, e), RANGE, max(0, v - d), min(v + d, (1 << w) - 1), neg))
        rules.append((int(rng.integers(0, 5)), tl))
    return nested(rules, default=int(rng.integers(0, 3)))


def odd_chains(rng):
    """Chains that are no parse of the batch: a header that ends at len (present) or one byte past it (absent),
    offsets past the packet, n_hdrs = 200, an STP header for the longest header's last bit."""
    hp = [L4.pkt("TCP", payload=L4.rnd(rng, 12)) for _ in range(8)]  # 66 bytes
    rows = [L4.hdrs_of(p) for p in hp]
    E_, I4, TC, UD = HID["Ether"], HID["IPv4"], HID["TCP"], HID["UDP"]
    rows[0] = [(E_, 0), (I4, 14), (TC, 46)]            # TCP ends at 66 == len: present
    rows[1] = [(E_, 0), (I4, 14), (TC, 47)]            # ... at len + 1: absent
    rows[2] = [(E_, 0), (I4, 60000), (TC, 65535)]      # past the packet
    rows[3] = [(HID["STP"], 31), (HID["STP"], 32), (UD, 58), (UD, 59)]  # STP ends at 66 / 67; UDP at 66 / 67
    rows[4] = [(I4, 14)] * 16
    rows[5] = [(HID["Vlan"], 2 * k) for k in range(14)] + [(I4, 14), (UD, 34)]
    b = indexed(hp, rng)
    ch = F.chain_from(8, rows)
    ch["n_hdrs"][6] = 200                              # taken as 16: rows 3.. are zeros (type 0: no header's)
    return b, ch


ODD_PROGRAM = nested([
    (1, [has("TCP")]), (2, [has("TCP", 0, True), has("IPv4")]), (3, [term("STP", 0, (279, 279), RANGE, 0, 1)]),
    (4, [has("STP", 1)]), (5, [has("UDP", 0), has("UDP", 1, True)]), (6, [term("IPv4", 15, "ttl", EQ, 64)]),
    (7, [term("Vlan", 13, (0, 31), RANGE, 0, M64)]), (8, [term("UDP", 0, "dst", RANGE, 0, 65535)]), (9, [has("Ether")])], default=11)


# ------------------------------------------------------------------ the case list
def build():
    """name -> (batch, chain, program).  The evaluators are shared per batch (all_cases)."""
    rng = np.random.default_rng(64)
    cs = {}
    sp = special_packets(rng)
    mb = indexed(sp + [L4.pkt("UDP", src=SRC[1], dport=80), L4.pkt("UDP", dport=443)], rng)
    mch = L4.chain_of(mb)
    ref_len = len(sp[0])
    for name, prog in hand_programs(ref_len).items():
        cs["mix_" + name] = (mb, mch, prog)
    ob, och = odd_chains(rng)
    cs["odd_chains"] = (ob, och, ODD_PROGRAM)
    cs["odd_chains_stp"] = (ob, och, hand_programs(66)["stp_last_bit"])
    cs["odd_chains_len"] = (ob, och, hand_programs(66)["len"])
    rb = ref22_batch()
    rch = L4.chain_of(rb)
    for name in ("has", "edges", "deep", "first_match_order"):
        cs["ref22_" + name] = (rb, rch, hand_programs(ref_len)[name])
    xb = indexed(random_mix(rng, 2000), rng)
    xch = L4.chain_of(xb)
    cs["random_acl"] = (xb, xch, acl())
    cs["random_rules64"] = (xb, xch, hand_programs(ref_len)["rules64"])
    cs["random_refs30"] = (xb, xch, refs30())
    ev = Evaluator(xb, xch)
    for k in range(20):
        cs[f"random_{k:02d}"] = (xb, xch, random_program(rng, ev))
    cs["empty_batch"] = (batch(np.zeros(0, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint32)),
                         F.chain_from(0, []), acl())
    return cs


HAND = ["no_rules", "zero_term_rule", "has", "eq", "range", "len", "has_not", "eq_not", "range_not", "len_not", "edges", "deep",
        "stp_last_bit", "first_match_order", "terms256", "rules64", "shared_terms", "acl", "refs30"]
CASE_NAMES = (["mix_" + h for h in HAND] + ["odd_chains", "odd_chains_stp", "odd_chains_len"] +
              ["ref22_" + h for h in ("has", "edges", "deep", "first_match_order")] + ["random_acl", "random_rules64", "random_refs30"] +
              [f"random_{k:02d}" for k in range(20)] + ["empty_batch"])

_CASES = None


def all_cases():
    """name -> (batch, chain, program, expected): built once and shared; nothing may change them."""
    global _CASES
    if _CASES is None:
        evs = {}
        _CASES = {}
        for name, (b, ch, prog) in build().items():
            ev = evs.setdefault(id(b), Evaluator(b, ch))
            _CASES[name] = (b, ch, prog, ev.run(prog))
        assert sorted(_CASES) == sorted(CASE_NAMES), sorted(set(_CASES) ^ set(CASE_NAMES))
    return _CASES


def relaid(b, kind, shift=0):
    """The batch's packets in another layout: "indexed" = the same offsets moved up by `shift` bytes (same
    packets, same lengths); "stride64" / "stride128" = a fixed-stride slab with lens = min(len, stride)."""
    ext = extents(b)
    if kind == "indexed":
        slab = np.concatenate([np.full(shift, 0xEE, np.uint8), b["slab"]])
        return batch(slab, [o + shift for o, _ in ext], [ln for _, ln in ext])
    st = 64 if kind == "stride64" else 128
    slab = np.full(st * len(ext), 0xEE, np.uint8)
    lens = []
    for i, (o, ln) in enumerate(ext):
        k = min(ln, st)
        slab[i * st:i * st + k] = b["slab"][o:o + k]
        lens.append(k)
    return batch(slab, None, lens, stride=st, n=len(ext))


_RELAID = {}


def relaid_want(name, kind):
    """The case's batch as a fixed-stride slab and what the yardstick says to it (evaluators shared per batch)."""
    b, ch, prog, _ = all_cases()[name]
    key = (id(b), kind)
    if key not in _RELAID:
        rb = relaid(b, kind)
        _RELAID[key] = (rb, Evaluator(rb, ch))
    rb, ev = _RELAID[key]
    return rb, ev.run(prog)


def head(b, ch, want, n, cut=True):
    """The first n packets of an indexed batch, the slab ending with the last of them (cut), with their chain and
    the expected outputs (the counters recounted)."""
    nr = want["hits"].size - 1
    ext = extents(b)[:n]
    end = max(o + ln for o, ln in ext) if cut else b["slab"].size
    hb = batch(b["slab"][:end], [o for o, _ in ext], [ln for _, ln in ext])
    hch = dict(n_hdrs=ch["n_hdrs"][:n].copy(), hdr_type=np.ascontiguousarray(ch["hdr_type"][:, :n]),
               hdr_off=np.ascontiguousarray(ch["hdr_off"][:, :n]))
    w = {k: want[k][:n] for k in ("rule", "action", "select", "matched")}
    idx = np.where(w["rule"] == NONE, nr, w["rule"]).astype(np.int64)
    w["hits"] = np.bincount(idx, minlength=nr + 1).astype(np.uint64)
    w["bytes"] = np.bincount(idx, weights=[ln for _, ln in ext], minlength=nr + 1).astype(np.uint64)
    return hb, hch, w
