"""pkt_meter_create / pkt_meter_batch / _reset / _export on the device (Parser.meters / Meters.run): the kernels of
pktgpu_meter.hip against meter_cases' sequential model, exactly: colour, passed, marked, hits, bytes, the whole slab and
the exported state, on the cases test_meter_host.py holds the host handle to.  The arithmetic is covered on the CPU (the
host twin runs the same inline code); here it is the grouping by meter across radix passes, tiles and waves, the runs
walked by a lane or by a wave 64 packets a step, the state carried from step to step and from call to call, the
stores at every alignment and the counters.  The slab lies between two guard regions filled with 0xA5."""
import numpy as np
import pytest

import pktgpu
from pktgpu import schema

import meter_cases as M
import nat_cases as N
import fwd_cases as W

pytestmark = pytest.mark.gpu
GUARD = 4096


@pytest.fixture(scope="module")
def P():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible")
    return pktgpu.Parser(0)


def put(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def get(t):
    import torch
    torch.cuda.synchronize()
    return None if t is None else t.cpu().numpy()


class Guarded:
    """put_slab that lays the slab between two 0xA5 regions and checks them afterwards."""

    def __init__(self):
        self.made = []

    def __call__(self, a):
        import torch
        big = torch.full((GUARD + (a.size + 15) // 16 * 16 + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        slab = big[GUARD:GUARD + a.size]
        slab.copy_(put(a))
        self.made.append((big, a.size))
        return slab

    def intact(self):
        return all(bool((big[:GUARD] == 0xA5).all()) and bool((big[GUARD + n:] == 0xA5).all()) for big, n in self.made)


def pair(P, cfgs, adjust=0):
    return P.meters(cfgs, adjust), M.Model(cfgs, adjust)


def play(P, sc, label):
    m, model = pair(P, sc["cfgs"], sc["adjust"])
    g = Guarded()
    outs = M.play(m, model, sc["calls"], put, get, label, put_slab=g)
    assert g.intact(), "a byte outside the slab was written"
    return outs, m, model


@pytest.mark.parametrize("name", M.NAMED)
def test_named(P, name):
    outs = play(P, M.named_cached()[name], name)[0]
    col = np.concatenate([o["color"] for o in outs])
    if name in ("overload_srtcm", "overload_trtcm"):  # a long run whose every step fails the scan and is walked
        assert (col[0::2] == M.GREEN).all() and (col[1::2] == M.RED).all()
    if name in ("edge_wave_max_gain", "edge_wave_max_gain_drained"):
        assert (col[-260:] == M.GREEN).all()


@pytest.mark.parametrize("nmeters", M.SIZES_M)
@pytest.mark.parametrize("n", M.SIZES_N)
def test_sizes(P, n, nmeters):
    play(P, M.sizes(n, nmeters), f"n={n} nmeters={nmeters}")


@pytest.mark.parametrize("cut", M.SPLITS)
def test_split_property(P, cut):
    cfgs, call = M.cached("split", M.split_case)
    n = call["b"]["n"]
    m1, model1 = pair(P, cfgs, 20)
    one = M.play(m1, model1, [call], put, get, "whole")[0]
    m2, model2 = pair(P, cfgs, 20)
    two = M.play(m2, model2, [M.head(call, 0, cut), M.head(call, cut, n)], put, get, f"cut {cut}")
    for k in M.NAMES:
        assert np.array_equal(np.concatenate([two[0][k], two[1][k]]), one[k]), k
    for k in ("hits", "bytes"):
        assert np.array_equal(two[0][k] + two[1][k] - (M.H0 if k == "hits" else M.Y0), one[k]), k
    M.same_state(m2.export(), m1.export(), f"cut {cut}")


def test_fresh_handles_agree_and_reset_restores(P):
    cfgs, call = M.cached("split", M.split_case)
    m1, model = pair(P, cfgs)
    fresh = m1.export()
    M.same_state(fresh, model.export(), "create")
    a = M.play(m1, model, [call], put, get, "first")[0]
    m2, model2 = pair(P, cfgs)
    b = M.play(m2, model2, [call], put, get, "second")[0]
    for k in M.NAMES + ("hits", "bytes"):
        assert np.array_equal(a[k], b[k]), k
    M.same_state(m1.export(), m2.export(), "fresh handles")
    m1.reset()
    model.reset()
    M.same_state(m1.export(), fresh, "reset")
    c = M.play(m1, model, [call], put, get, "after reset")[0]
    assert np.array_equal(a["color"], c["color"])
    M.same_state(m1.export(first=7, count=5), m1.export()[7:12], "part")
    assert m1.export(first=300, count=0).size == 0


def test_meters_are_independent(P):
    """A meter's packets alone, on a fresh handle, get what they got in the mix."""
    cfgs, call = M.cached("split", M.split_case)
    m, model = pair(P, cfgs, 20)
    mix = M.play(m, model, [call], put, get, "mix")[0]
    k = int(np.bincount(call["meter"][call["meter"] < 300]).argmax())
    mine = np.flatnonzero((call["meter"] == k) & (call["select"] != 0))
    sub = dict(call, b=M.C.batch(call["b"]["slab"], offsets=call["b"]["offsets"][mine], lens=call["b"]["lens"][mine]))
    for f in ("meter", "time", "in_color", "select"):
        sub[f] = call[f][mine]
    m2, model2 = pair(P, cfgs, 20)
    alone = M.play(m2, model2, [sub], put, get, "alone")[0]
    assert np.array_equal(alone["color"], mix["color"][mine])
    M.same_state(m2.export()[k:k + 1], m.export()[k:k + 1], "alone")


@pytest.mark.parametrize("kind", ["indexed", "stride"])
@pytest.mark.parametrize("which_ip", [0, 1, M.LAST])
def test_remark(P, which_ip, kind):
    cfgs, call = M.remark_call(which_ip, kind)
    play(P, M.scenario(cfgs, call), f"remark which={which_ip} {kind}")
    # the colour and passed never depend on headers: the same call without MARK and without a chain
    got = play(P, M.scenario(cfgs, dict(call, chain=None, mark=False)), "no mark")[0][0]
    assert not got["marked"].any() and np.array_equal(got["slab"], call["b"]["slab"])


def test_remark_many_packets_every_alignment(P):
    """More packets than a block, every alignment and both IP versions in every wave, long and short runs."""
    cfgs, call = M.remark_call(0)
    items = (M.remark_items() * 9)[:700]
    b, chain = N.layout(items, "indexed")
    rng = np.random.default_rng(8)
    play(P, M.scenario(cfgs, dict(b=b, chain=chain, meter=rng.integers(0, 6, b["n"]).astype(np.uint32), now=1, mark=True,
                                  which_ip=M.LAST)), "remark 700")


def test_null_outputs(P):
    import torch
    cfgs, call = M.remark_call(0)
    b, chain = call["b"], call["chain"]
    for mask in range(8):
        outs = tuple(k for j, k in enumerate(M.NAMES) if mask >> j & 1)
        for counters in (None, True):
            m, model = pair(P, cfgs)
            want = model.run(b, chain, meter=call["meter"], now=1, mark=True)
            db = dict(slab=put(b["slab"]), offsets=put(b["offsets"]), lens=put(b["lens"]))
            r = m.run(db, {k: put(v) for k, v in chain.items()}, meter=put(call["meter"]), now=1, mark=True, outputs=outs,
                      counters=counters)
            torch.cuda.synchronize()
            for k in M.NAMES:
                assert (getattr(r, k) is None) == (k not in outs)
                if k in outs:
                    assert np.array_equal(get(getattr(r, k)), want[k]), k
            assert np.array_equal(get(db["slab"]), want["slab"])
            if counters:
                assert np.array_equal(get(r.hits), want["hits"]) and np.array_equal(get(r.bytes), want["bytes"])
            M.same_state(m.export(), model.export(), f"outputs {outs}")


def test_refusals(P):
    import ctypes
    from pktgpu import _lib
    L = P._L
    h = ctypes.c_void_p()
    bad = pktgpu.meter_cfgs([dict(cir=1, cbs=1, mode=2)])
    assert L.pkt_meter_create(P._ctx, bad.ctypes.data, 1, 0, ctypes.byref(h)) == -1
    assert L.pkt_ctx_last_error(P._ctx).decode().startswith("pkt_meter_create: ")
    assert L.pkt_meter_create(P._ctx, bad.ctypes.data, 0, 0, ctypes.byref(h)) == -1 and not h.value
    cfgs, call = M.remark_call(0)
    m = P.meters(cfgs)
    slab = put(call["b"]["slab"])
    b = P._batch(slab[1:], None, None, put(call["b"]["offsets"]), put(call["b"]["lens"]))
    s = P._stream(None)
    rc = L.pkt_meter_batch(m._t, ctypes.byref(b), None, 0, 0, 0, None, 0, None, None, None, None, None, None, None, None, s)
    assert rc == -1 and L.pkt_meter_last_error(m._t).decode() == "pkt_meter_batch: slab not 16-byte aligned"
    assert L.pkt_ctx_last_error(P._ctx).decode() == "pkt_meter_batch: slab not 16-byte aligned"
    b = P._batch(slab, None, None, put(call["b"]["offsets"]), put(call["b"]["lens"]))
    for flags, chain, which in ((2, None, 0), (1, None, 0), (1, ctypes.byref(P._chain({k: put(v) for k, v in call["chain"].items()})), 16)):
        assert L.pkt_meter_batch(m._t, ctypes.byref(b), chain, which, flags, 0, None, 0, None, None, None, None, None, None,
                                 None, None, s) == -1
        assert L.pkt_meter_last_error(m._t).decode().startswith("pkt_meter_batch: ")
    M.same_state(m.export(), M.Model(cfgs).export(), "after refusals")


@pytest.mark.parametrize("nmeters", [3, 70000])
def test_past_the_chunk_of_2_20_packets(P, nmeters):
    """A call is taken 2^20 packets at a time and the state carries over.  The Python model would take too long here:
    the yardstick is the host handle, which test_meter_host.py holds to the model."""
    n = (1 << 20) + 2049
    rng = np.random.default_rng(nmeters)
    cfgs = M.mixed_cfgs(nmeters, rng)
    if nmeters > 1000:
        cfgs["cir"] //= 1 + (1 << 20) // nmeters // 20  # a share of the traffic turns yellow and red
    meter = rng.integers(0, nmeters + nmeters // 50 + 2, n).astype(np.uint32)
    time = (1000 + np.cumsum(rng.integers(0, 3000, n))).astype(np.uint64)
    ic = (rng.random(n) < 0.001).astype(np.uint8)
    b = M.plain(rng.integers(40, 200, n))
    host, dev = pktgpu.Meters(None, cfgs, 20), P.meters(cfgs, 20)
    want = host.run(b, meter=meter, time=time, in_color=ic, counters=True)
    db = dict(slab=put(b["slab"]), offsets=put(b["offsets"]), lens=put(b["lens"]))
    got = dev.run(db, meter=put(meter), time=put(time), in_color=put(ic), counters=True)
    for k in M.NAMES + ("hits", "bytes"):
        assert np.array_equal(get(getattr(got, k)), getattr(want, k)), k
    assert (np.bincount(want.color, minlength=4) > 1000).all()
    M.same_state(dev.export(), host.export(), "past the chunk")


def test_chain_columns_from_parse_and_fragment(P):
    """The chain columns a parse gives, and the out chain of fragment, feed the remark with no second parse."""
    import torch
    def no_df(item):
        p, hdrs = item
        o = [o for t, o in hdrs if t == M.T_IPV4][0]
        q = bytearray(p)
        q[o + 6] &= 0xBF
        return W.fix_csum(bytes(q), o), hdrs

    items = [no_df(W.v4(vlans=k % 3, payload=b"q" * (300 + 40 * k))) for k in range(40)] + [W.v6(vlans=k % 2) for k in range(8)]
    b, chain = N.layout(items, "indexed")
    cfgs = [M.cfg(0, 2000, 3000, dscp=(8, 16, 24), **M.MARK_ALL)] * 3
    db = dict(slab=put(b["slab"]), offsets=put(b["offsets"]), lens=put(b["lens"]))
    res = P.parse(db["slab"], offsets=db["offsets"], lens=db["lens"])
    dch = {c: res[c] for c in ("n_hdrs", "hdr_type", "hdr_off")}
    hch = {c: get(v) for c, v in dch.items()}
    meter = np.arange(b["n"], dtype=np.uint32) % 3
    m, model = pair(P, cfgs)
    want = model.run(b, hch, meter=meter, now=5, mark=True)
    r = m.run(db, dch, meter=put(meter), now=5, mark=True)
    M.check(dict(color=get(r.color), passed=get(r.passed), marked=get(r.marked), slab=get(db["slab"])), want, "parse")
    assert want["marked"].all() and len(set(want["color"])) == 3
    f = P.fragment(db, dch, mtu=200)
    k = f.n_out
    assert k > b["n"]
    fb = dict(slab=f.slab, offsets=f.offsets[:k].contiguous(), lens=f.lens[:k].contiguous())
    fch = {c: (v[:k] if v.dim() == 1 else v[:, :k]).contiguous() for c, v in f.out_chain.items()}
    hb = M.C.batch(get(f.slab), offsets=get(fb["offsets"]), lens=get(fb["lens"]))
    want = model.run(hb, {c: get(v) for c, v in fch.items()}, meter=1, now=9, mark=True)
    r = m.run(fb, fch, meter=1, now=9, mark=True)
    M.check(dict(color=get(r.color), passed=get(r.passed), marked=get(r.marked), slab=get(f.slab)), want, "fragment")
    assert want["marked"].all()
    M.same_state(m.export(), model.export(), "fragment")


def test_pipeline_flow_table_meter_pcap_write(P):
    """flow_keys -> FlowTable.update -> meters.run(meter=flow_id, time=the capture's stamps) -> pcap_write(select=passed)."""
    import torch
    rng = np.random.default_rng(12)
    flows = [N.mk(("TCP", "UDP")[k & 1], f"10.0.{k}.1", 1000 + k, "198.51.100.7", 80, payload=b"p" * (20 * k)) for k in range(12)]
    items = [flows[int(k)] for k in rng.integers(0, 12, 500)] + [W.without(W.v4(), M.T_IPV4)] * 3
    b, chain = N.layout(items, "indexed")
    n = b["n"]
    db = dict(slab=put(b["slab"]), offsets=put(b["offsets"]), lens=put(b["lens"]))
    dch = {c: put(v) for c, v in chain.items()}
    sec = np.full(n, 1700000000, np.uint32) + (np.arange(n) // 250).astype(np.uint32)
    usec = ((np.arange(n) % 250) * 4000).astype(np.uint32)
    slots = 256
    table = pktgpu.FlowTable(P, slots)
    keys = P.flow_keys(db["slab"], dch, offsets=db["offsets"], lens=db["lens"])
    flow_id, upd = table.update(keys)
    cfgs = [M.cfg(cir=2000, cbs=700, xbs=500, action=(M.PASS, M.PASS, M.DROP))] * slots
    m, model = pair(P, cfgs, adjust=20)
    time = pktgpu.ns_from_sec_usec(put(sec), put(usec))
    r = m.run(db, meter=flow_id, time=time)
    hid = get(flow_id)
    assert (hid[-3:] == pktgpu.FLOW_NONE).all() and len(set(hid[:-3])) == 12
    want = model.run(b, meter=hid, time=pktgpu.ns_from_sec_usec(sec, usec))
    M.check(dict(color=get(r.color), passed=get(r.passed), marked=get(r.marked)), want, "pipeline")
    assert (want["color"][-3:] == M.UNMETERED).all() and 0 < want["passed"].sum() < n
    M.same_state(m.export(), model.export(), "pipeline")
    cap, k, offs, lens, src = P.pcap_write(db["slab"], offsets=db["offsets"], lens=db["lens"], select=r.passed)
    assert k == int(want["passed"].sum()) and np.array_equal(get(src)[:k], np.flatnonzero(want["passed"]))
