"""pkt_meter_create_host / pkt_meter_batch / _reset / _export on host pointers (Parser.meters(host=True) is not needed:
pktgpu.Meters(None, ...)): the host handle, which runs the same inline refill, decision and DSCP stores as the kernels
(pktgpu_meter.hpp), against meter_cases' model in Python integers, exactly.  No GPU."""
import ctypes

import numpy as np
import pytest

import pktgpu
from pktgpu import _lib, schema

import meter_cases as M
import nat_cases as N


def put(a):
    return np.ascontiguousarray(a).copy()


def get(a):
    return None if a is None else np.asarray(a)


def pair(cfgs, adjust=0):
    return pktgpu.Meters(None, cfgs, adjust), M.Model(cfgs, adjust)


def play(sc, label):
    m, model = pair(sc["cfgs"], sc["adjust"])
    return M.play(m, model, sc["calls"], put, get, label), m, model


def test_abi():
    L = _lib.load()
    assert L.pkt_sizeof_meter_cfg() == 32 == schema.METER_CFG_DTYPE.itemsize == ctypes.sizeof(_lib.PktMeterCfg)
    assert L.pkt_sizeof_meter_state() == 72 == schema.METER_STATE_DTYPE.itemsize == ctypes.sizeof(_lib.PktMeterState)
    assert L.pkt_abi_version() == 5


@pytest.mark.parametrize("name", M.NAMED)
def test_named(name):
    outs, _, _ = play(M.named_cached()[name], name)
    col = np.concatenate([o["color"] for o in outs])
    if name == "edge_cost_equals_level":
        assert list(col) == [M.GREEN, M.GREEN]
    if name == "edge_cost_one_unit_above":
        assert list(col) == [M.GREEN, M.RED]
    if name == "edge_refill_lands_on_cap":
        assert list(col) == [M.GREEN, M.GREEN, M.GREEN, M.YELLOW]
    if name == "edge_spill_fills_x":
        assert list(col) == [M.GREEN, M.YELLOW, M.GREEN, M.GREEN, M.YELLOW, M.RED]
    if name == "edge_spill_one_unit_short":
        assert list(col) == [M.GREEN, M.YELLOW, M.GREEN, M.GREEN, M.RED]
    if name == "all_red":
        assert (col == M.RED).all()
    if name == "edge_cost_0":
        assert list(col) == [M.GREEN] * 4 + [M.RED]  # the last one costs a byte, and both bursts are 0
    if name == "edge_adjust_min":
        assert (col == M.GREEN).all()
    if name in ("edge_wave_max_gain", "edge_wave_max_gain_drained"):
        assert (col[-260:] == M.GREEN).all()
    if name == "edge_wave_max_gain_cost":
        assert (col == M.RED).all()
    if name in ("overload_srtcm", "overload_trtcm"):
        assert list(col[:9]) == [M.GREEN, M.RED] * 4 + [M.GREEN] and (col[0::2] == M.GREEN).all() and (col[1::2] == M.RED).all()
    if name.startswith("step_bad_"):
        pos = 64 + int(name.split("_")[2])
        assert col[pos] == M.RED and (np.delete(col, pos) == M.GREEN).all()


@pytest.mark.parametrize("nmeters", M.SIZES_M)
@pytest.mark.parametrize("n", M.SIZES_N)
def test_sizes(n, nmeters):
    outs, _, _ = play(M.sizes(n, nmeters), f"n={n} nmeters={nmeters}")
    if n >= 2047 and nmeters > 1:
        assert len(set(outs[0]["color"])) == 4  # every colour occurs in the mix


def whole_and_split(make, cut):
    cfgs, call = M.cached("split", M.split_case)
    n = call["b"]["n"]
    m1, model1 = make(cfgs)
    one = M.play(m1, model1, [call], put, get, "whole")[0]
    m2, model2 = make(cfgs)
    two = M.play(m2, model2, [M.head(call, 0, cut), M.head(call, cut, n)], put, get, f"cut {cut}")
    for k in M.NAMES:
        assert np.array_equal(np.concatenate([two[0][k], two[1][k]]), one[k]), k
    for k in ("hits", "bytes"):
        assert np.array_equal(two[0][k] + two[1][k] - (M.H0 if k == "hits" else M.Y0), one[k]), k
    M.same_state(m2.export(), m1.export(), f"cut {cut}")


@pytest.mark.parametrize("cut", M.SPLITS)
def test_split_property(cut):
    whole_and_split(lambda cfgs: pair(cfgs, 20), cut)


def test_meters_are_independent():
    """A meter's packets alone, on a fresh handle, get what they got in the mix."""
    cfgs, call = M.cached("split", M.split_case)
    m, model = pair(cfgs, 20)
    mix = M.play(m, model, [call], put, get, "mix")[0]
    k = int(np.bincount(call["meter"][call["meter"] < 300]).argmax())
    mine = np.flatnonzero((call["meter"] == k) & (call["select"] != 0))
    sub = dict(call, b=M.C.batch(call["b"]["slab"], offsets=call["b"]["offsets"][mine], lens=call["b"]["lens"][mine]))
    for f in ("meter", "time", "in_color", "select"):
        sub[f] = call[f][mine]
    m2, model2 = pair(cfgs, 20)
    alone = M.play(m2, model2, [sub], put, get, "alone")[0]
    assert np.array_equal(alone["color"], mix["color"][mine])
    M.same_state(m2.export()[k:k + 1], m.export()[k:k + 1], 'alone')


def test_fresh_handles_agree_and_reset_restores():
    cfgs, call = M.cached("split", M.split_case)
    m1, model = pair(cfgs, 0)
    fresh = m1.export()
    assert (fresh["c"] == m1.cfgs["cbs"].astype(np.uint64) * M.UNIT).all() and (fresh["x"] == m1.cfgs["xbs"].astype(np.uint64) * M.UNIT).all()
    assert not fresh["last"].any() and not fresh["packets"].any() and not fresh["bytes"].any()
    a = M.play(m1, model, [call], put, get, "first")[0]
    m2, model2 = pair(cfgs, 0)
    b = M.play(m2, model2, [call], put, get, "second")[0]
    for k in M.NAMES + ("hits", "bytes"):
        assert np.array_equal(a[k], b[k]), k
    M.same_state(m1.export(), m2.export(), 'fresh handles')
    m1.reset()
    model.reset()
    M.same_state(m1.export(), fresh, 'reset')
    c = M.play(m1, model, [call], put, get, "after reset")[0]
    assert np.array_equal(a["color"], c["color"])
    part = m1.export(first=7, count=5)
    M.same_state(part, m1.export()[7:12], 'part')
    assert m1.export(first=300, count=0).size == 0


# ------------------------------------------------------------------ remark
def ip_ok(p, t, o):
    return t != M.T_IPV4 or N.ip_error(p, o) == 0


@pytest.mark.parametrize("kind", ["indexed", "stride"])
@pytest.mark.parametrize("which_ip", [0, 1, M.LAST])
def test_remark(which_ip, kind):
    cfgs, call = M.remark_call(which_ip, kind)
    m, model = pair(cfgs)
    got = M.play(m, model, [call], put, get, f"remark which={which_ip} {kind}")[0]
    b, chain = call["b"], call["chain"]
    before, after = M.C.packets(b), M.C.packets(dict(b, slab=got["slab"]))
    assert got["marked"].sum() >= (2 if which_ip == 1 else 40)  # a second IP entry: the tunnel packet and a forged chain
    cols = []
    for i, (p, q) in enumerate(zip(before, after)):
        ipe = M.find_ip(chain, i, which_ip)
        if not got["marked"][i]:
            assert p == q, i
            continue
        t, o = ipe
        k = int(call["meter"][i])
        dscp = int(m.cfgs["dscp"][k][got["color"][i]])
        cols.append(int(got["color"][i]))
        if t == M.T_IPV4:
            assert q[o + 1] >> 2 == dscp and q[o + 1] & 3 == p[o + 1] & 3, i            # the DSCP written, ECN kept
            assert N.ip_error(q, o) == N.ip_error(p, o), i                              # valid stays valid, wrong as wrong
            same = [j for j in range(len(p)) if j not in (o + 1, o + 10, o + 11)]
        else:
            tc = (q[o] & 0x0F) << 4 | q[o + 1] >> 4
            assert tc >> 2 == dscp and tc & 3 == (p[o + 1] >> 4) & 3 and q[o] >> 4 == p[o] >> 4 and q[o + 1] & 0xF == p[o + 1] & 0xF, i
            same = [j for j in range(len(p)) if j not in (o, o + 1)]
        assert all(p[j] == q[j] for j in same), i
    assert which_ip == 1 or len(set(cols)) == 3
    # the colour and passed never depend on headers: the same call without MARK and without a chain
    m2, model2 = pair(cfgs)
    plain = M.play(m2, model2, [dict(call, chain=None, mark=False)], put, get, "no mark")[0]
    assert np.array_equal(plain["color"], got["color"]) and np.array_equal(plain["passed"], got["passed"])
    assert not plain["marked"].any() and np.array_equal(plain["slab"], b["slab"])


def test_remark_on_the_tunnel_packet():
    cfgs, call = M.remark_call(0)
    i = len(M.remark_items()) - 9  # the VXLAN packet
    p = M.C.packets(call["b"])[i]
    ips = [o for t, o in M.remark_items()[i][1] if t == M.T_IPV4]
    assert len(ips) == 2
    for which, o in ((0, ips[0]), (1, ips[1]), (M.LAST, ips[1])):
        m, model = pair(cfgs)
        got = M.play(m, model, [dict(call, which_ip=which, meter=0)], put, get, f"vxlan {which}")[0]
        q = M.C.packets(dict(call["b"], slab=got["slab"]))[i]
        assert got["marked"][i] and q[o + 1] >> 2 == 46 and [j for j in range(len(p)) if p[j] != q[j]][0] == o + 1


# ------------------------------------------------------------------ outputs and refusals
def test_null_outputs():
    cfgs, call = M.remark_call(0)
    for mask in range(8):
        outs = tuple(k for j, k in enumerate(M.NAMES) if mask >> j & 1)
        for counters in (None, True):
            m, model = pair(cfgs)
            want = model.run(call["b"], call["chain"], meter=call["meter"], now=1, mark=True)
            b = dict(call["b"], slab=put(call["b"]["slab"]))
            r = m.run(b, call["chain"], meter=call["meter"], now=1, mark=True, outputs=outs, counters=counters)
            for k in M.NAMES:
                assert (getattr(r, k) is None) == (k not in outs)
                if k in outs:
                    assert np.array_equal(getattr(r, k), want[k]), k
            assert np.array_equal(b["slab"], want["slab"])
            if counters:
                assert np.array_equal(r.hits, want["hits"]) and np.array_equal(r.bytes, want["bytes"])
            M.same_state(m.export(), model.export())


BAD_CFGS = [dict(cir=(1 << 40) + 1, cbs=1), dict(cir=1, pir=(1 << 40) + 1, cbs=1), dict(cir=1, cbs=(1 << 26) + 1),
            dict(cir=1, cbs=1, xbs=(1 << 26) + 1), dict(cir=1, cbs=1, mode=2), dict(cir=1, cbs=1, action=(0, 3, 0)),
            dict(cir=1, cbs=1, dscp=(0, 0, 64))]


@pytest.mark.parametrize("bad", range(len(BAD_CFGS) + 3))
def test_create_refusals(bad):
    L = _lib.load()
    good = pktgpu.meter_cfgs([M.cfg(1 << 40, 1 << 26, 1 << 26, pir=1 << 40)] * 3)
    h = ctypes.c_void_p()
    assert L.pkt_meter_create_host(good.ctypes.data, 3, 0, ctypes.byref(h)) == 0
    L.pkt_meter_destroy(h)
    if bad < len(BAD_CFGS):
        arr = good.copy()
        arr[1:2] = pktgpu.meter_cfgs([BAD_CFGS[bad]])
        args = (arr.ctypes.data, 3)
    elif bad == len(BAD_CFGS):
        arr = good.copy()
        arr["flags"][2] = 2
        args = (arr.ctypes.data, 3)
    else:
        args = ((good.ctypes.data, 0), (None, 3))[bad - len(BAD_CFGS) - 1]
    assert L.pkt_meter_create_host(*args, 0, ctypes.byref(h)) == -1
    assert L.pkt_meter_last_error(None).decode().startswith("pkt_meter_create_host: ")
    assert not h.value
    with pytest.raises(ValueError, match="pkt_meter_create_host"):
        pktgpu.Meters(None, [])
    assert L.pkt_meter_create_host(good.ctypes.data, (1 << 24) + 1, 0, ctypes.byref(h)) == -1


def test_call_refusals():
    L = _lib.load()
    cfgs, call = M.remark_call(0)
    m, model = pair(cfgs)
    b, keep = pktgpu._host_batch(_lib, call["b"])
    ch = call["chain"]
    chain = _lib.PktChain(ch["n_hdrs"].ctypes.data, ch["hdr_type"].ctypes.data, ch["hdr_off"].ctypes.data)
    words = np.zeros(16, np.uint64)
    ok = dict(b=ctypes.byref(b), chain=ctypes.byref(chain), which=0, flags=1, meter=None, time=None, hits=None, nbytes=None)

    def call_with(**kw):
        a = dict(ok, **kw)
        return L.pkt_meter_batch(m._t, a["b"], a["chain"], a["which"], a["flags"], 0, a["meter"], 0, a["time"], None, None,
                                 None, None, None, a["hits"], a["nbytes"], None)

    before = m.export()
    assert call_with(flags=0, chain=None, which=77) == 0  # without MARK neither is looked at
    m.reset()
    bad_n = _lib.PktBatch.from_buffer_copy(b)
    bad_n.n = 1 << 32
    no_lens = _lib.PktBatch.from_buffer_copy(b)
    no_lens.lens = None
    no_slab = _lib.PktBatch.from_buffer_copy(b)
    no_slab.slab = None
    no_col = _lib.PktChain(ch["n_hdrs"].ctypes.data, None, ch["hdr_off"].ctypes.data)
    for kw in (dict(b=None), dict(b=ctypes.byref(bad_n)), dict(flags=2), dict(flags=3), dict(chain=None), dict(which=16),
               dict(which=0xFE), dict(hits=words.ctypes.data + 4), dict(nbytes=words.ctypes.data + 1),
               dict(time=words.ctypes.data + 4), dict(meter=words.ctypes.data + 2), dict(b=ctypes.byref(no_lens)),
               dict(b=ctypes.byref(no_slab)), dict(chain=ctypes.byref(no_col))):
        assert call_with(**kw) == -1, kw
        assert L.pkt_meter_last_error(m._t).decode().startswith("pkt_meter_batch: "), kw
    assert call_with(which=M.LAST) == 0
    m.reset()
    M.same_state(m.export(), before, 'refusals')
    empty = _lib.PktBatch()
    assert L.pkt_meter_batch(m._t, ctypes.byref(empty), None, 0, 0, 0, None, 0, None, None, None, None, None, None, None,
                             None, None) == 0  # n == 0
    assert L.pkt_meter_export(m._t, 3, 3, words.ctypes.data) == -1
    assert L.pkt_meter_export(m._t, 0, 1, None) == -1
    assert L.pkt_meter_batch(None, ctypes.byref(b), None, 0, 0, 0, None, 0, None, None, None, None, None, None, None, None,
                             None) == -1
    with pytest.raises(ValueError, match="chain"):
        m.run(call["b"], None, mark=True)


def test_ns_from_sec_usec():
    sec, usec = np.asarray([0, 1, 0xFFFFFFFF], np.uint32), np.asarray([0, 999999, 999999], np.uint32)
    ns = pktgpu.ns_from_sec_usec(sec, usec)
    assert ns.dtype == np.uint64 and [int(x) for x in ns] == [0, 1999999000, 0xFFFFFFFF * 10 ** 9 + 999999000]
