"""pkt_dispatch_host and pkt_reorder_host (pktgpu.dispatch / pktgpu.reorder), the CPU twins of the per-queue
batch kernels, against dispatch_cases' yardstick: every case, every NULL-output combination, every refusal (-1,
outputs untouched), and the reorder over ref22.pcap and a random mix at every source alignment, with cuts, empty
positions, empty segments, the unwritten tail and any subset of columns.  The raw calls write into arrays filled
with 0x77, so that a byte the call must not write is seen.  No device."""
import ctypes

import numpy as np
import pytest

import pktgpu
from pktgpu import _lib, schema

import compare_cases as C
import dispatch_cases as D

INVALID = -1
DT = dict(bucket=np.uint16, perm=np.uint32, rank=np.uint32, start=np.uint64)


def ptr(a):
    return a.ctypes.data if a is not None and a.size else None


def raw_dispatch(c, outputs=D.OUTPUT_SETS[15], n=None, nb=None, table=-1, tlen=None, start_shift=0):
    """pkt_dispatch_host into 0x77-filled arrays -> (rc, {name: array})."""
    key = np.ascontiguousarray(c["key"], np.uint32)
    n = key.size if n is None else n
    nb = c["nb"] if nb is None else nb
    tab = c["table"] if isinstance(table, int) else table
    sel = None if c["select"] is None else np.ascontiguousarray(c["select"], np.uint8)
    res = {k: D.filled(min(n, key.size) if k != "start" else min(nb, 300) + 2 + 1, DT[k]) for k in outputs}
    args = [ptr(res.get(k)) for k in ("bucket", "perm", "rank")]
    st = res["start"].ctypes.data + start_shift if "start" in res else None
    rc = _lib.load().pkt_dispatch_host(nb, ptr(tab) if tab is not None else None, (tab.size if tab is not None else 0)
                                       if tlen is None else tlen, ptr(key), ptr(sel), n, *args, st)
    return rc, res


def test_yardstick_is_not_vacuous():
    assert hasattr(_lib.load(), "pkt_dispatch_host") and hasattr(_lib.load(), "pkt_reorder_host")
    cs = D.dispatch_cases()
    names = [c["name"] for c in cs]
    assert len(set(names)) == len(names)
    w = D.expect_dispatch(np.array([2, 0, 9, 2, 1, 0], np.uint32), 3)
    assert w["perm"].tolist() == [1, 5, 4, 0, 3, 2] and w["start"].tolist() == [0, 2, 3, 5, 6]
    assert w["bucket"].tolist() == [2, 0, 0xFFFF, 2, 1, 0] and w["rank"].tolist() == [3, 0, 5, 4, 2, 1]
    w = D.expect_dispatch(np.array([0x80000001, 3, 2], np.uint32), 2, table=[1, D.DROP], select=[1, 1, 0])
    assert w["bucket"].tolist() == [D.DROP, D.DROP, D.DROP]
    w = D.expect_dispatch(np.array([0x80000002, 3, 2], np.uint32), 2, table=[1, D.DROP], select=[1, 1, 0])
    assert w["bucket"].tolist() == [1, D.DROP, D.DROP] and w["start"].tolist() == [0, 0, 1, 3]


@pytest.mark.parametrize("c", D.dispatch_cases(), ids=lambda c: c["name"])
def test_dispatch_cases(c):
    want = D.expect_dispatch(c["key"], c["nb"], c["table"], c["select"])
    rc, got = raw_dispatch(c)
    assert rc == 0
    got["start"] = got["start"][:c["nb"] + 2]
    D.check_dispatch(got, want, c["name"])
    D.check_dispatch(pktgpu.dispatch(c["key"], c["nb"], c["table"], c["select"]), want, c["name"] + " (wrapper)")


def test_n_1000_is_a_permutation_and_stable():
    c = next(c for c in D.dispatch_cases() if c["name"] == "table_128_4_full")
    got = pktgpu.dispatch(c["key"], c["nb"], c["table"])
    assert np.array_equal(np.sort(got["perm"]), np.arange(1000))
    st = got["start"].astype(np.int64)
    for b in range(c["nb"] + 1):
        seg = got["perm"][st[b]:st[b + 1]].astype(np.int64)
        assert (np.diff(seg) > 0).all()
        assert (got["bucket"][seg] == (b if b < c["nb"] else D.DROP)).all()


def test_every_null_output_combination():
    c = next(c for c in D.dispatch_cases() if c["name"] == "direct_3_select")
    want = D.expect_dispatch(c["key"], c["nb"], c["table"], c["select"])
    for outs in D.OUTPUT_SETS:
        rc, got = raw_dispatch(c, outs)
        assert rc == 0 and set(got) == set(outs)
        if "start" in got:
            assert (got["start"][c["nb"] + 2:].view(np.uint8) == D.FILL).all()
            got["start"] = got["start"][:c["nb"] + 2]
        D.check_dispatch(got, want, str(outs))


def test_start_is_written_not_added_to():
    c = D.dispatch_cases()[0]
    want = D.expect_dispatch(c["key"], c["nb"], c["table"], c["select"])
    for _ in range(2):
        rc, got = raw_dispatch(c, ("start",))  # (the fill is not zero)
        assert rc == 0 and np.array_equal(got["start"][:c["nb"] + 2], want["start"])


def test_dispatch_refusals_leave_outputs_untouched():
    c = D.dcase("r", np.arange(8) % 3, 3)
    big = np.zeros(8192, np.uint16)
    bad = [dict(nb=0), dict(nb=257), dict(table=np.zeros(3, np.uint16)), dict(table=big), dict(table=big[:1], tlen=0),
           dict(table=np.array([0, 3], np.uint16)), dict(table=np.array([0, 0xFFFE], np.uint16)),
           dict(n=1 << 32), dict(start_shift=4)]
    for kw in bad:
        rc, got = raw_dispatch(c, **kw)
        assert rc == INVALID, kw
        for k, a in got.items():
            assert (a.view(np.uint8) == D.FILL).all(), (kw, k)
    # a NULL key with n > 0
    start = D.filled(5, np.uint64)
    assert _lib.load().pkt_dispatch_host(3, None, 0, None, None, 4, None, None, None, start.ctypes.data) == INVALID
    assert (start.view(np.uint8) == D.FILL).all()
    with pytest.raises(ValueError):
        pktgpu.dispatch(np.arange(4), 0)
    # n == 0: start zero-filled, nothing else; all outputs NULL: nothing
    assert _lib.load().pkt_dispatch_host(3, None, 0, None, None, 0, None, None, None, start.ctypes.data) == 0
    assert start.tolist() == [0] * 5
    assert _lib.load().pkt_dispatch_host(3, None, 0, None, None, 7, None, None, None, None) == INVALID  # (key first)


# ------------------------------------------------------------------ reorder
def raw_reorder(b, perm, cols, want_cols, seg, nseg, slot, dst_short=0, dst_shift=0, m=None, perm_null=False,
                out_len_without_dst=False, out_only=None):
    """pkt_reorder_host into 0x77-filled arrays -> (rc, dst, out_len, {column: array})."""
    perm = np.ascontiguousarray(perm, np.uint32)
    m = perm.size if m is None else m
    ma = min(m, 4096)  # (what is allocated: a refused m >= 2^32 writes nothing)
    bs, keep = pktgpu._host_batch(_lib, b) if b is not None else (_lib.PktBatch(), None)
    raw = D.filled(ma * (slot or 0) + 32, np.uint8)
    o = (-raw.ctypes.data) % 16 + dst_shift
    dst = raw[o:o + ma * (slot or 0) - dst_short] if slot else None
    out_len = D.filled(ma, np.uint32) if slot or out_len_without_dst else None
    ci, co, oc, held = _lib.PktOut(), _lib.PktOut(), {}, []
    for c in want_cols:
        a = np.ascontiguousarray(cols[c])
        held.append(a)
        shp = schema.column_shape(c, ma)
        oc[c] = D.filled((schema.MAX_HDRS * ma,) if c in ("hdr_type", "hdr_off") and nseg else shp, a.dtype)
        if c != out_only:
            setattr(ci, c, a.ctypes.data)
        setattr(co, c, oc[c].ctypes.data)
    sg = None if seg is None else np.ascontiguousarray(seg, np.uint64)
    rc = _lib.load().pkt_reorder_host(ctypes.byref(bs), ctypes.byref(ci), None if perm_null else ptr(perm), m, ptr(sg), nseg,
                                      dst.ctypes.data if dst is not None else None, dst.size if dst is not None else 0,
                                      slot or 0, ptr(out_len), ctypes.byref(co))
    return rc, (raw, o, dst), out_len, oc


@pytest.mark.parametrize("c", D.reorder_cases(), ids=lambda c: c["name"])
def test_reorder_cases(c):
    b, cols = D.sources()[c["src"]]
    want = D.expect_reorder(b, c["perm"], {k: cols[k] for k in c["cols"]}, c["seg"], c["nseg"], c["slot"])
    rc, (raw, o, dst), out_len, oc = raw_reorder(b, c["perm"], cols, c["cols"], c["seg"], c["nseg"], c["slot"])
    assert rc == 0
    D.check_reorder(dst, out_len, oc, want, c["name"])
    if dst is not None:  # nothing around dst
        assert (raw[:o] == D.FILL).all() and (raw[o + dst.size:] == D.FILL).all()


@pytest.mark.parametrize("al", range(16))
def test_reorder_every_source_alignment(al):
    b0, cols = D.sources()["ref22"]
    b = D.aligned(b0, al)
    assert all(int(x) % 16 == al for x in b["offsets"])
    rng = np.random.default_rng(al)
    perm = rng.permutation(b["n"] + 2).astype(np.uint32)  # two empty positions
    for slot in (48, 1536):
        want = D.expect_reorder(b, perm, {}, None, 0, slot)
        rc, (raw, o, dst), out_len, oc = raw_reorder(b, perm, cols, (), None, 0, slot)
        assert rc == 0
        D.check_reorder(dst, out_len, oc, want, f"align {al} slot {slot}")
    assert want["out_len"].max() > 48  # 48 cut some packet, 1536 none


def test_reorder_wrapper_and_segments():
    b, cols = D.sources()["mix"]
    n = b["n"]
    rng = np.random.default_rng(3)
    key = rng.integers(0, 5, n).astype(np.uint32)  # 4 drops
    d = pktgpu.dispatch(key, 4)
    chain = {k: cols[k] for k in ("n_hdrs", "hdr_type", "hdr_off")}
    r = pktgpu.reorder(d["perm"], b["slab"], offsets=b["offsets"], lens=b["lens"], columns=chain, start=d["start"], slot=1536)
    assert r["nseg"] == 4 and r["slab"].ctypes.data % 16 == 0
    segs = pktgpu.segments(d["start"], r)
    pk = C.packets(b)
    assert sum(s["n"] for s in segs) == int(d["start"][4]) < n
    for q, s in enumerate(segs):
        src = np.flatnonzero(key == q)
        assert s["n"] == src.size and s["stride"] == 1536
        sb = C.batch(s["slab"], lens=s["lens"], stride=s["stride"], n=s["n"])
        assert C.packets(sb) == [pk[i] for i in src]
        for j, i in enumerate(src):  # the segment's chain is slot-major over ITS packets
            nh = int(cols["n_hdrs"][i])
            assert s["chain"]["n_hdrs"][j] == nh
            assert np.array_equal(s["chain"]["hdr_type"][:nh, j], cols["hdr_type"][:nh, i])
            assert np.array_equal(s["chain"]["hdr_off"][:nh, j], cols["hdr_off"][:nh, i])
        # and what the host calls take: the match twin over the segment = over the whole batch, gathered
        if s["n"]:
            import match_cases as M
            prog = M.acl()
            whole = pktgpu.match(b["slab"], chain, M.to_ctypes(prog), prog["default"], offsets=b["offsets"], lens=b["lens"])
            part = pktgpu.match(s["slab"], s["chain"], M.to_ctypes(prog), prog["default"], stride=s["stride"], n=s["n"], lens=s["lens"])
            assert np.array_equal(part["rule"], whole["rule"][src]) and np.array_equal(part["matched"], whole["matched"][src])


def test_reorder_refusals_leave_outputs_untouched():
    b, cols = D.sources()["ref22"]
    n = b["n"]
    perm = np.arange(n, dtype=np.uint32)
    seg = np.array([0, n], np.uint64)
    cs = ("n_hdrs", "hdr_off")
    bad = [dict(slot=8), dict(slot=24), dict(slot=1536, dst_shift=8), dict(slot=64, dst_short=1), dict(m=1 << 32, slot=64),
           dict(nseg=258, seg=np.zeros(259, np.uint64)), dict(nseg=1, seg=None), dict(perm_null=True),
           dict(slot=None, out_len_without_dst=True), dict(out_only="hdr_off"),
           dict(b=dict(slab=b["slab"], stride=0, n=n, offsets=None, lens=None))]
    for kw in bad:
        kw = dict(kw)
        bb = kw.pop("b", b)
        slot = kw.pop("slot", 64)
        sg, ns = kw.pop("seg", seg), kw.pop("nseg", 1)
        rc, (raw, o, dst), out_len, oc = raw_reorder(bb, perm, cols, cs, sg, ns, slot, **kw)
        assert rc == INVALID, kw
        assert (raw == D.FILL).all() and (out_len is None or (out_len.view(np.uint8) == D.FILL).all()), kw
        for c, a in oc.items():
            assert (a.view(np.uint8) == D.FILL).all(), (kw, c)
    # a NULL slab with slab_len > 0, and offsets without lens: straight structs
    L = _lib.load()
    dst = pktgpu._aligned_zeros(64 * n)
    dst[:] = D.FILL
    offs = np.ascontiguousarray(b["offsets"], np.uint64)
    for bs in (_lib.PktBatch(None, 100, None, None, 64, 0, n), _lib.PktBatch(b["slab"].ctypes.data, b["slab"].size, offs.ctypes.data, None, 0, 0, n)):
        assert L.pkt_reorder_host(ctypes.byref(bs), None, perm.ctypes.data, n, None, 0, dst.ctypes.data, dst.size, 64, None, None) == INVALID
        assert (dst == D.FILL).all()
    # m == 0 succeeds, and so does a call without dst or columns
    bs, keep = pktgpu._host_batch(_lib, b)
    assert L.pkt_reorder_host(ctypes.byref(bs), None, None, 0, None, 0, dst.ctypes.data, dst.size, 64, None, None) == 0
    assert L.pkt_reorder_host(ctypes.byref(bs), None, perm.ctypes.data, n, None, 0, None, 0, 0, None, None) == 0
    assert (dst == D.FILL).all()
