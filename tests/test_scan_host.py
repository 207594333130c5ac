"""pkt_scan_create_host / pkt_scan_batch on host memory (no GPU): scan_cases' list against its independent model,
every refusal's code and text, the counters' identities, and PAYLOAD's r0 against the parse's payload_off.  The host
handle runs the compiler, the walk, the region rule and the result of pktgpu_scan.hpp, which the kernel shares."""
import ctypes

import numpy as np
import pytest

import pktgpu
from pktgpu import _lib, schema

import compare_cases as C
import match_cases as M
import pyref
import scan_cases as S


@pytest.mark.parametrize("name", S.NAMES)
def test_case_equals_model(name):
    c = S.all_cases()[name]
    got, info = S.host_call(c)
    want = S.expected(name)
    S.check(got, want, name)
    assert info["npatterns"] == len(c["pats"]) and info["placement"] == schema.SCAN_PLACE_GLOBAL
    assert info["max_len"] == max([len(p[0]) for p in c["pats"]], default=0)
    # the identities: a call adds sum(count) to hits[0..npats) and the MISS packets to hits[npats]
    assert int(got["hits"][:-1].sum()) == int(got["count"].sum(dtype=np.uint64))
    assert int(got["hits"][-1]) == int((got["status"] == S.MISS).sum())


def test_names_cover_the_list():
    assert sorted(S.NAMES) == sorted(S.all_cases())


def test_random_differential():
    c = S.random_differential()
    want = S.expect(c)
    share = float((want["status"] == S.HIT).mean())
    assert 0.25 <= share <= 0.75, share                      # not vacuous
    assert float((want["count"] >= 3).mean()) >= 0.01
    got, _ = S.host_call(c)
    S.check(got, want, "random")


def test_hits_accumulate_and_null_outputs():
    c = S.all_cases()["family"]
    want = S.expected("family")
    sc = pktgpu.Scanner(None, S.tables(c["pats"]))
    hits = np.full(len(c["pats"]) + 1, 5, np.uint64)
    for _ in range(2):
        sc.run(c["batch"], None, "packet", want=(), hits=hits)   # hits alone
    assert np.array_equal(hits, 5 + 2 * want["hits"])
    for k, _ in S.OUTPUTS:                                       # each output alone
        r = sc.run(c["batch"], None, "packet", want=(k,))
        S.check({k: getattr(r, k)}, {k: want[k]}, k)
    r = sc.run(c["batch"], None, "packet", want=())              # nothing asked for: succeeds
    assert r.status is None and r.hits is None


def test_info_counts_states():
    sc = pktgpu.Scanner(None, ["abc", "abd", "x"], nocase=[False, False, True])
    assert sc.info == dict(npatterns=3, nstates=2 + 4 + 1, max_len=3, placement=0, table_bytes=sc.info["table_bytes"])
    # NOCASE and exact patterns sharing prefixes live in two tries: the states add, they do not multiply
    one = pktgpu.Scanner(None, ["getgetgetget"]).info["nstates"]
    both = pktgpu.Scanner(None, ["getgetgetget", "GetGetGetGet", "GETGETGETGET"], nocase=[False, True, True]).info["nstates"]
    assert both == 2 * one - 2
    assert pktgpu.Scanner(None, []).info["nstates"] == 2


def test_create_refusals():
    L = _lib.load()
    blob = np.frombuffer(b"abcdefgh" * 16, np.uint8)
    h = ctypes.c_void_p()

    def rc(tab, nbytes=blob.size, bp=blob.ctypes.data, n=None, tp=0):
        n = tab.size if n is None else n
        r = L.pkt_scan_create_host(bp, nbytes, (tab.ctypes.data if tab.size else None) if tp == 0 else tp, n, 0, ctypes.byref(h))
        if r == 0:
            L.pkt_scan_destroy(h)
            return 0, ""
        assert not h.value
        return r, L.pkt_scan_last_error(None).decode()

    def one(**kw):
        t = np.zeros(2, schema.SCAN_PATTERN_DTYPE)
        t["len"] = 4
        for k, v in kw.items():
            t[k][1] = v
        return t

    assert rc(one()) == (0, "")
    for kw, word in ((dict(len=0), "len"), (dict(len=65), "len"), (dict(off=125), "nbytes"), (dict(flags=2), "flag"),
                     (dict(group=64), "group"), (dict(reserved=1), "reserved")):
        r, msg = rc(one(**kw))
        assert r == -1 and msg.startswith("pkt_scan_create: pattern 1") and word in msg, (kw, msg)
    assert rc(one(len=64, off=64))[0] == 0 and rc(one(off=124))[0] == 0                      # the edges are legal
    r, msg = rc(np.zeros(0, schema.SCAN_PATTERN_DTYPE), n=schema.SCAN_MAX_PATTERNS + 1, tp=blob.ctypes.data)
    assert r == -1 and "PKT_SCAN_MAX_PATTERNS" in msg
    r, msg = rc(np.zeros(0, schema.SCAN_PATTERN_DTYPE), n=3)
    assert r == -1 and "null patterns" in msg
    r, msg = rc(one(), bp=None)
    assert r == -1 and "null bytes" in msg
    big = np.zeros(2049, schema.SCAN_PATTERN_DTYPE)                                           # 2049 * 64 bytes
    big["len"] = 64
    r, msg = rc(big)
    assert r == -1 and "PKT_SCAN_MAX_BYTES" in msg
    assert rc(big[:2048])[0] == 0
    assert L.pkt_scan_create_host(None, 0, None, 0, 0, None) == -1
    assert rc(np.zeros(0, schema.SCAN_PATTERN_DTYPE), nbytes=0, bp=None) == (0, "")           # npats == 0 is legal
    assert L.pkt_sizeof_scan_pattern() == 16 == schema.SCAN_PATTERN_DTYPE.itemsize
    with pytest.raises(ValueError, match="pkt_scan_create"):
        pktgpu.Scanner(None, [b""])


def test_batch_refusals():
    L = _lib.load()
    c = S.all_cases()["edges_payload"]
    sc = pktgpu.Scanner(None, S.tables(c["pats"]))
    b, keep = pktgpu._host_batch(_lib, c["batch"])
    n = b.n
    cols = [np.ascontiguousarray(c["chain"][k]) for k in ("n_hdrs", "hdr_type", "hdr_off")]
    ch = _lib.PktChain(*[x.ctypes.data for x in cols])
    out = np.zeros(n + 1, np.uint64)
    st = np.full(n, 0x77, np.uint8)

    def rc(batch=b, chain=ch, region=1, matched=None, hits=None):
        r = L.pkt_scan_batch(sc._t, ctypes.byref(batch), None if chain is None else ctypes.byref(chain), region, None,
                             st.ctypes.data, None, None, None, None, None, matched, hits, None)
        return r, L.pkt_scan_last_error(sc._t).decode() if r else ""

    assert rc() == (0, "")
    assert rc(chain=None, region=0) == (0, "")                          # PACKET: the chain may be NULL
    st[:] = 0x77
    assert rc(chain=None) == (-1, "pkt_scan_batch: null chain with PKT_SCAN_PAYLOAD")
    for k in range(3):
        p = [x.ctypes.data for x in cols]
        p[k] = None
        assert rc(chain=_lib.PktChain(*p)) == (-1, "pkt_scan_batch: null chain column")
    assert rc(region=2) == (-1, "pkt_scan_batch: unknown region")
    assert rc(matched=out.ctypes.data + 4) == (-1, "pkt_scan_batch: matched / hits not 8-byte aligned")
    assert rc(hits=out.ctypes.data + 1) == (-1, "pkt_scan_batch: matched / hits not 8-byte aligned")
    huge = _lib.PktBatch()
    huge.slab, huge.slab_len, huge.stride, huge.n = b.slab, b.slab_len, 64, 1 << 32
    assert rc(batch=huge) == (-1, "pkt_scan_batch: n >= 2^32")
    for bad, msg in ((dict(offsets=b.offsets, lens=None, stride=0), "offsets without lens"),
                     (dict(offsets=None, lens=None, stride=0), "stride 0"),
                     (dict(offsets=b.offsets, lens=b.lens, stride=0, slab=None), "null slab")):
        x = _lib.PktBatch()
        x.slab, x.slab_len, x.n = bad.get("slab", b.slab), b.slab_len, n
        x.offsets, x.lens, x.stride = bad["offsets"], bad["lens"], bad["stride"]
        assert rc(batch=x) == (-1, "pkt_scan_batch: " + msg)
    assert (st == 0x77).all()                                           # a refusal writes nothing
    empty = _lib.PktBatch()
    assert rc(batch=empty) == (0, "") and rc(batch=empty, chain=_lib.PktChain()) == (0, "")   # n == 0 succeeds
    assert L.pkt_scan_batch(None, ctypes.byref(b), None, 0, *([None] * 10)) == -1
    assert L.pkt_scan_batch(sc._t, None, None, 0, *([None] * 10)) == -1
    assert schema.SCAN_STATUS == ["MISS", "HIT", "SKIPPED", "NO_CHAIN", "SPAN"]
    assert (pktgpu.SCAN_MISS, pktgpu.SCAN_SPAN, pktgpu.SCAN_NONE) == (0, 4, 0xFFFFFFFF)


def r0_of(pkts):
    """PAYLOAD's r0 per packet, observed: with the 256 one-byte patterns every byte of the region is one occurrence,
    so count = r1 - r0."""
    b = C.indexed(pkts, np.random.default_rng(1))
    c = S.case([S.pat(bytes([v])) for v in range(256)], b, "payload", C.chain_of(b))
    got, _ = S.host_call(c)
    return c, got


def test_payload_r0_is_the_parse_payload_off():
    pkts = C.packets(M.ref22_batch()) + [S.gre_no_inner()]
    assert len(pkts) == 23
    c, got = r0_of(pkts)
    types = c["chain"]["hdr_type"][:, 22][:int(c["chain"]["n_hdrs"][22])].tolist()
    assert types[-1] == schema.HDR_ID["GREChksumOffset"] and len(types) == 6      # the wire-earliest option is last
    seen = 0
    for i, p in enumerate(pkts):
        status, hdrs, poff, plen = pyref.parse(p)
        if not hdrs:
            assert got["status"][i] == S.NO_CHAIN
            continue
        assert poff + plen == len(p)
        assert len(p) - int(got["count"][i]) == poff, (i, got["count"][i], poff)
        assert got["status"][i] == (S.HIT if plen else S.MISS)
        seen += 1
    assert seen >= 20 and len(pkts[22]) - int(got["count"][22]) == 50
