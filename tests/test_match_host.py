"""pkt_match_host (pktgpu.match), the CPU twin of the rule-table kernel, against match_cases' yardstick: every
case in the indexed layout at every slab alignment and as fixed-stride 64 / 128 slabs, every NULL-output
combination, accumulating counters, the length clamps, the program refusals, and the select mask feeding
pktgpu.pcap_write.  No device."""
import ctypes
import itertools

import numpy as np
import pytest

import pktgpu
from pktgpu import _lib, schema

import match_cases as M

INVALID = -1
OUTS = ("rule", "action", "select", "matched")


def host(b, ch, prog, outputs=OUTS, hits=True, bytes=True):
    return pktgpu.match(b["slab"], ch, M.to_ctypes(prog), prog["default"], stride=b["stride"], n=b["n"], offsets=b["offsets"],
                        lens=b["lens"], outputs=outputs, hits=hits, bytes=bytes)


def test_yardstick_is_not_vacuous():
    assert hasattr(_lib.load(), "pkt_match_host")  # the yardstick judges a library that has the call
    cs = M.all_cases()
    cover = set().union(*[w["cover"] for _, _, _, w in cs.values()])
    for op in (M.HAS, M.EQ, M.RANGE, M.LEN):
        for neg in (0, M.NOT):
            assert (op, neg, True) in cover and (op, neg, False) in cover, (op, neg)
    w = cs["random_acl"][3]
    assert (w["hits"] > 0).all()  # every rule is some packet's first match, and "none" occurs
    assert ((w["matched"] & (w["matched"] - np.uint64(1))) != 0).any()  # two or more rules match one packet
    assert int(cs["mix_rules64"][3]["matched"].max()) >> 63 == 1
    assert len(cs["mix_terms256"][2]["terms"]) == 256 and len(cs["mix_rules64"][2]["rules"]) == 64
    # the hand-made chains: present at len, absent one byte on
    w = cs["odd_chains"][3]
    # (packet 2's IPv4 lies past the packet: only has(Ether), rule 8; packet 3: STP 0, UDP 0 without UDP 1, UDP.dst)
    assert w["rule"][:4].tolist() == [0, 1, 8, 2] and w["matched"][3] == 0b10010100


@pytest.mark.parametrize("name", M.CASE_NAMES)
def test_cases(name):
    b, ch, prog, want = M.all_cases()[name]
    M.check(host(b, ch, prog), want, name)
    if b["n"] == 0:
        return
    for shift in range(16):
        M.check(host(M.relaid(b, "indexed", shift), ch, prog), want, f"{name} + {shift}")
    for kind in ("stride64", "stride128"):
        rb, rw = M.relaid_want(name, kind)
        M.check(host(rb, ch, prog), rw, f"{name} {kind}")


def test_null_outputs_and_counters():
    b, ch, prog, want = M.all_cases()["mix_acl"]
    for k in range(5):
        for outs in itertools.combinations(OUTS, k):
            for hb in itertools.product((True, None), repeat=2):
                got = host(b, ch, prog, outputs=outs, hits=hb[0], bytes=hb[1])
                assert set(got) == set(outs) | ({"hits"} if hb[0] else set()) | ({"bytes"} if hb[1] else set())
                M.check(got, want, f"{outs} {hb}")
    # they accumulate: two calls into the same arrays, sum(hits) grows by n each time
    b, ch, prog, want = M.all_cases()["random_acl"]
    hits, byt = np.zeros(17, np.uint64), np.zeros(17, np.uint64)
    for call in (1, 2):
        host(b, ch, prog, outputs=(), hits=hits, bytes=byt)
        assert int(hits.sum()) == call * b["n"]
        assert np.array_equal(hits, call * want["hits"]) and np.array_equal(byt, call * want["bytes"])
    assert int(want["bytes"].sum()) == sum(ln for _, ln in M.extents(b))


def test_length_clamps():
    # lens past the slab end and past 65535: LEN terms and bytes see the clamped length
    slab = np.zeros(70000 + 100, np.uint8)
    b = M.batch(slab, [0, 70000, 70090, 70100, 80000], [70000, 200, 10, 5, 5])
    ch = M.F.chain_from(5, [[]] * 5)
    prog = M.nested([(1, [M.length(65535, 65535)]), (2, [M.length(100, 100)]), (3, [M.length(10, 10)]), (4, [M.length(0, 0)])])
    got = host(b, ch, prog)
    assert got["rule"].tolist() == [0, 1, 2, 3, 3]
    assert got["bytes"].tolist() == [65535, 100, 10, 0, 0]
    M.check(got, M.Evaluator(b, ch).run(prog), "clamps")


def raw_call(terms, nterms, rules, nrules, n=1):
    slab = np.zeros(64, np.uint8)
    b = _lib.PktBatch(slab.ctypes.data, 64, None, None, 64, 0, n)
    cols = (np.zeros(1, np.uint8), np.zeros(16, np.uint8), np.zeros(16, np.uint16))
    ch = _lib.PktChain(*[c.ctypes.data for c in cols])
    rule = np.full(1, 0x77, np.uint8)
    rc = _lib.load().pkt_match_host(terms, nterms, rules, nrules, 0, ctypes.byref(b), ctypes.byref(ch), rule.ctypes.data,
                                    None, None, None, None, None)
    return rc, int(rule[0])


def bad_programs():
    """(label, terms, nterms, rules, nrules): every refusal of pkt_match_create."""
    T, R, F = _lib.PktMatchTerm, _lib.PktMatchRule, _lib.PktFieldSpec
    ok = T(F(3, 0, 72, 79, 0), schema.MATCH_EQ, 0, 0, 0, 6, 0xFF)
    one = (R * 1)(R(0, 1, 1))

    def t1(t):
        return (T * 1)(t)
    out = [("65 rules", t1(ok), 1, (R * 65)(*[R(0, 1, 1)] * 65), 65),
           ("257 terms", (T * 257)(*[ok] * 257), 257, one, 1),
           ("range past nterms", t1(ok), 1, (R * 1)(R(1, 1, 1)), 1),
           ("range past nterms (2)", t1(ok), 1, (R * 1)(R(0, 2, 1)), 1),
           ("unknown op", t1(T(F(3, 0, 72, 79, 0), 4, 0, 0, 0, 6, 0xFF)), 1, one, 1),
           ("unknown flag", t1(T(F(3, 0, 72, 79, 0), schema.MATCH_EQ, 2, 0, 0, 6, 0xFF)), 1, one, 1),
           ("reserved", t1(T(F(3, 0, 72, 79, 0), schema.MATCH_EQ, 0, 1, 0, 6, 0xFF)), 1, one, 1),
           ("reserved2", t1(T(F(3, 0, 72, 79, 0), schema.MATCH_EQ, 0, 0, 1, 6, 0xFF)), 1, one, 1),
           ("field.reserved", t1(T(F(3, 0, 72, 79, 1), schema.MATCH_EQ, 0, 0, 0, 6, 0xFF)), 1, one, 1),
           ("hdr_type 0", t1(T(F(0, 0, 0, 7, 0), schema.MATCH_EQ, 0, 0, 0, 6, 0xFF)), 1, one, 1),
           ("hdr_type 22", t1(T(F(22, 0, 0, 7, 0), schema.MATCH_RANGE, 0, 0, 0, 6, 0xFF)), 1, one, 1),
           ("HAS hdr_type 22", t1(T(F(22, 0, 0, 0, 0), schema.MATCH_HAS, 0, 0, 0, 0, 0)), 1, one, 1),
           ("HAS hdr_type 0", t1(T(F(0, 0, 0, 0, 0), schema.MATCH_HAS, 0, 0, 0, 0, 0)), 1, one, 1),
           ("end < start", t1(T(F(3, 0, 80, 79, 0), schema.MATCH_EQ, 0, 0, 0, 6, 0xFF)), 1, one, 1),
           ("end past header", t1(T(F(3, 0, 152, 160, 0), schema.MATCH_EQ, 0, 0, 0, 6, 0xFF)), 1, one, 1),
           ("width 65", t1(T(F(4, 0, 64, 128, 0), schema.MATCH_RANGE, 0, 0, 0, 6, 0xFF)), 1, one, 1),
           ("LEN with a field", t1(T(F(3, 0, 0, 0, 0), schema.MATCH_LEN, 0, 0, 0, 6, 0xFF)), 1, one, 1),
           ("LEN with bits", t1(T(F(0, 0, 0, 7, 0), schema.MATCH_LEN, 0, 0, 0, 6, 0xFF)), 1, one, 1),
           ("null terms", None, 1, one, 1),
           ("null rules", t1(ok), 1, None, 1)]
    return out


def good_edge_programs():
    T, R, F = _lib.PktMatchTerm, _lib.PktMatchRule, _lib.PktFieldSpec
    return [("HAS ignores its bits", (T * 1)(T(F(3, 0, 900, 5, 0), schema.MATCH_HAS, 0, 0, 0, 1, 2)), 1, (R * 1)(R(0, 1, 1)), 1),
            ("width 64 to the last bit", (T * 1)(T(F(4, 0, 256, 319, 0), schema.MATCH_RANGE, 1, 0, 0, 5, 4)), 1, (R * 1)(R(0, 1, 1)), 1),
            ("no rules, null pointers", None, 0, None, 0),
            ("64 rules of no terms", None, 0, (R * 64)(*[R(0, 0, 1)] * 64), 64)]


def test_program_refusals():
    for label, terms, nt, rules, nr in bad_programs():
        rc, rule = raw_call(terms, nt, rules, nr)
        assert rc == INVALID and rule == 0x77, label
        assert raw_call(terms, nt, rules, nr, n=0)[0] == INVALID, label  # the program is checked before the batch
    for label, terms, nt, rules, nr in good_edge_programs():
        rc, rule = raw_call(terms, nt, rules, nr)
        assert rc == 0 and rule != 0x77, label


def test_empty_batch_and_bad_batches():
    b, ch, prog, want = M.all_cases()["empty_batch"]
    hits = np.full(17, 5, np.uint64)
    got = host(b, ch, prog, hits=hits, bytes=None)
    assert got["rule"].size == 0 and (hits == 5).all()
    ta, ra = M.to_ctypes(prog)
    L = _lib.load()
    slab = np.zeros(64, np.uint8)
    cols = (np.zeros(1, np.uint8), np.zeros(16, np.uint8), np.zeros(16, np.uint16))
    ch1 = _lib.PktChain(*[c.ctypes.data for c in cols])
    good = _lib.PktBatch(slab.ctypes.data, 64, None, None, 64, 0, 1)
    out = np.zeros(4, np.uint64)

    def call(bt, chn, matched=None, hits=None, byt=None):
        return L.pkt_match_host(ta, len(ta), ra, len(ra), 0, bt, chn, None, None, None, matched, hits, byt)
    assert call(ctypes.byref(good), ctypes.byref(ch1)) == 0  # every output NULL
    assert call(None, ctypes.byref(ch1)) == INVALID and call(ctypes.byref(good), None) == INVALID
    assert call(ctypes.byref(_lib.PktBatch(slab.ctypes.data, 64, None, None, 64, 0, 1 << 32)), ctypes.byref(ch1)) == INVALID
    assert call(ctypes.byref(_lib.PktBatch(slab.ctypes.data, 64, None, None, 0, 0, 1)), ctypes.byref(ch1)) == INVALID
    assert call(ctypes.byref(_lib.PktBatch(slab.ctypes.data, 64, out.ctypes.data, None, 64, 0, 1)), ctypes.byref(ch1)) == INVALID
    assert call(ctypes.byref(_lib.PktBatch(None, 64, None, None, 64, 0, 1)), ctypes.byref(ch1)) == INVALID
    assert call(ctypes.byref(good), ctypes.byref(_lib.PktChain(cols[0].ctypes.data, None, cols[2].ctypes.data))) == INVALID
    for k in range(3):  # matched, hits, bytes off an 8-byte boundary
        ptrs = [None] * 3
        ptrs[k] = out.ctypes.data + 4
        assert call(ctypes.byref(good), ctypes.byref(ch1), *ptrs) == INVALID


def test_struct_sizes():
    L = _lib.load()
    assert L.pkt_sizeof_match_term() == 32 == ctypes.sizeof(_lib.PktMatchTerm)
    assert L.pkt_sizeof_match_rule() == 8 == ctypes.sizeof(_lib.PktMatchRule)
    assert (schema.MATCH_MAX_RULES, schema.MATCH_MAX_TERMS, schema.MATCH_NONE, schema.MATCH_NOT) == (64, 256, 0xFF, 1)


def test_python_term_forms():
    """Parser.match_program's term syntax gives the same structs as the tuples of match_cases."""
    rules = [(7, [("IPv4", 0, "src", "==", M.ip4("10.1.1.7"), 0xFFFFFF00), ("UDP", 0, "dst", "in", 50, 100),
                  (schema.HDR_ID["TCP"], 0, (0, 15), "not in", 1, 2), ("len", "not in", 0, 59), ("Vlan", 1, None, "has"),
                  ("IPv4", 0, "protocol", "!=", 6), ("ARP", 0, None, "not has")]), (0, [])]
    ta, nt, ra, nr = pktgpu.match_arrays(rules)
    want = [M.term("IPv4", 0, "src", M.EQ, M.ip4("10.1.1.7"), 0xFFFFFF00), M.term("UDP", 0, "dst", M.RANGE, 50, 100),
            M.term("TCP", 0, (0, 15), M.RANGE, 1, 2, neg=True), M.length(0, 59, True), M.has("Vlan", 1),
            M.term("IPv4", 0, "protocol", M.EQ, 6, neg=True), M.has("ARP", 0, True)]
    assert (nt, nr) == (7, 2) and (ra[0].first_term, ra[0].nterms, ra[0].action, ra[1].nterms) == (0, 7, 7, 0)
    for t, w in zip(ta, want):
        assert (t.field.hdr_type, t.field.occurrence, t.field.start, t.field.end, t.op, t.flags, t.a, t.b) == w
    with pytest.raises(ValueError):
        pktgpu.match_arrays([(1, [("IPv4", 0, "src", "~=", 1)])])
    b, ch, _, _ = M.all_cases()["mix_acl"]
    got = pktgpu.match(b["slab"], ch, rules, default=3, offsets=b["offsets"], lens=b["lens"])
    M.check(got, M.Evaluator(b, ch).run(dict(M.nested([(7, want), (0, [])]), default=3)), "term forms")


def test_select_feeds_pcap_write():
    b, ch, prog, want = M.all_cases()["mix_eq"]
    sel = host(b, ch, prog, outputs=("select",), hits=None, bytes=None)["select"]
    assert 0 < int(sel.sum()) < b["n"] and np.array_equal(sel, want["select"])
    cap = pktgpu.pcap_write(b["slab"], offsets=b["offsets"], lens=b["lens"], select=sel)
    buf = cap[0] if isinstance(cap, tuple) else cap
    offs, lens = pktgpu.pcap_index(np.asarray(buf))
    pk = M.C.packets(b)
    keep = [pk[i] for i in np.flatnonzero(want["select"])]
    assert [bytes(np.asarray(buf)[int(o):int(o) + int(ln)]) for o, ln in zip(offs, lens)] == keep
