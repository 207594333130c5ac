"""pkt_flow_key_host and the host flow table (pktgpu.flow_keys, FlowTable(None, slots)) against flow_cases'
yardstick: a pure-Python key builder, a bitwise Toeplitz pinned to the Microsoft RSS table
(tests/golden/rss_vectors.json) and a dict model of the table.  No device."""
import ctypes

import numpy as np
import pytest

import pktgpu
from pktgpu import _lib, schema

import flow_cases as F
import l4_cases as L4
from compare_cases import indexed


def keys_of(c, **over):
    b, o = c["batch"], dict(c["opt"], **over)
    return pktgpu.flow_keys(b["slab"], c["chain"], o["which_ip"], o["symmetric"], o["ports"], F.SEED, F.RSS_KEY,
                            stride=b["stride"], n=b["n"], offsets=b["offsets"], lens=b["lens"])


def test_yardstick_is_pinned():
    F.pin_yardstick()
    L = _lib.load()
    assert L.pkt_sizeof_flow_key() == ctypes.sizeof(_lib.PktFlowKey) == schema.FLOW_KEY_DTYPE.itemsize == 40
    assert L.pkt_sizeof_flow_record() == ctypes.sizeof(_lib.PktFlowRecord) == schema.FLOW_RECORD_DTYPE.itemsize == 80


@pytest.mark.parametrize("name", F.CASE_NAMES)
def test_cases(name):
    c, want = F.all_cases()[name]
    F.check(keys_of(c), want, name)


def test_every_flag_combination_on_the_protocol_mix():
    c, _ = F.all_cases()["protocols"]
    for which in (0, 1, F.LAST):
        for sym in (False, True):
            for ports in (False, True):
                F.check(keys_of(c, which_ip=which, symmetric=sym, ports=ports),
                        F.expect(c, which_ip=which, symmetric=sym, ports=ports), f"{which} {sym} {ports}")


def test_both_directions_share_key_hash_and_rss():
    c, want = F.all_cases()["symmetric"]
    got = keys_of(c)
    for a, b in ((0, 1), (3, 4), (6, 7), (8, 9), (11, 12), (14, 15), (16, 17), (18, 19)):
        assert got["keys"][a].tobytes() == got["keys"][b].tobytes() and got["hash"][a] == got["hash"][b]
        assert got["rss"][a] == got["rss"][b] and {int(got["dir"][a]), int(got["dir"][b])} == {0, 1}, (a, b)
    assert got["dir"][2] == 0 and got["dir"][10] == 0  # equal endpoints


def test_rss_matches_the_microsoft_vectors():
    """The library against the published table and, through test_cases, against the Python Toeplitz that
    test_yardstick_is_pinned holds to the same table."""
    key, vec, pk = F.rss_packets()
    b = indexed(pk, np.random.default_rng(3))
    ch = L4.chain_of(b)
    for ports, col in ((True, "with_ports"), (False, "addr_only")):
        got = pktgpu.flow_keys(b["slab"], ch, ports=ports, rss_key=key, offsets=b["offsets"], lens=b["lens"])
        assert got["rss"].tolist() == [int(v[col], 16) for v in vec], (ports, [hex(x) for x in got["rss"]])
    assert "rss" not in pktgpu.flow_keys(b["slab"], ch, offsets=b["offsets"], lens=b["lens"])


def raw_call(c, r=(), outputs=(True,) * 6, rss_key=F.RSS_KEY):
    """pkt_flow_key_host with argument positions replaced -> (rc, outputs)."""
    L = _lib.load()
    b, keep = pktgpu._host_batch(_lib, c["batch"])
    ch = _lib.PktChain(*[np.ascontiguousarray(c["chain"][k]).ctypes.data for k in ("n_hdrs", "hdr_type", "hdr_off")])
    n = b.n
    shapes = (((n, 40), np.uint8), (n, np.uint64), (n, np.uint32), (n, np.uint8), (n, np.uint32), (n, np.uint8))
    out = [np.full(s, 0x77, dt) if w else None for (s, dt), w in zip(shapes, outputs)]
    rk = ctypes.create_string_buffer(rss_key, 40) if rss_key else None
    o = c["opt"]
    a = [ctypes.byref(b), ctypes.byref(ch), o["which_ip"], (1 if o["symmetric"] else 0) | (0 if o["ports"] else 2), F.SEED, rk,
         *[None if x is None else x.ctypes.data for x in out]]
    for k, v in dict(r).items():
        a[k] = v
    return L.pkt_flow_key_host(*a), dict(zip(("keys", "hash", "rss", "dir", "plen", "status"), out)), (b, ch, keep)


def test_null_outputs():
    for name in ("protocols", "c2_stride64_65", "span_lens"):
        c, want = F.all_cases()[name]
        for drop in range(6):
            outputs = tuple(k != drop for k in range(6))
            rc, got, _ = raw_call(c, outputs=outputs)
            assert rc == 0
            F.check(got, want, f"{name} without output {drop}")
        rc, got, _ = raw_call(c, outputs=(False,) * 6, rss_key=None)
        assert rc == 0


def test_refusals():
    c, want = F.all_cases()["c2_stride64_65"]
    rc, got, (b, ch, keep) = raw_call(c)
    assert rc == 0
    huge = _lib.PktBatch(b.slab, b.slab_len, None, None, 64, 0, 1 << 32)
    no_slab = _lib.PktBatch(None, b.slab_len, None, None, 64, 0, 65)
    stride0 = _lib.PktBatch(b.slab, b.slab_len, None, None, 0, 0, 65)
    four = np.zeros(4, np.uint64)
    no_lens = _lib.PktBatch(b.slab, b.slab_len, four.ctypes.data, None, 0, 0, 4)
    no_col = _lib.PktChain(ch.n_hdrs, None, ch.hdr_off)
    bad = [{0: None}, {1: None}, {1: ctypes.byref(no_col)}, {0: ctypes.byref(huge)}, {0: ctypes.byref(no_slab)},
           {0: ctypes.byref(stride0)}, {0: ctypes.byref(no_lens)}, {2: 16}, {2: 0xFE}, {3: 4}, {3: 0x80000001}, {5: None},
           {6: got["keys"].ctypes.data + 1}]
    for r in bad:
        rc, out, _ = raw_call(c, r)
        assert rc == -1, sorted(r)
        assert all((x == 0x77).all() for k, x in out.items() if not (6 in r and k == "keys")), sorted(r)
    empty = _lib.PktBatch(b.slab, b.slab_len, None, None, 64, 0, 0)
    assert raw_call(c, {0: ctypes.byref(empty)})[0] == 0
    assert raw_call(c, {2: 15})[0] == 0 and raw_call(c, {5: None}, outputs=(True, True, False, True, True, True))[0] == 0
    with pytest.raises(ValueError):
        pktgpu.flow_keys(c["batch"]["slab"], c["chain"], which_ip=16, stride=64)
    with pytest.raises(ValueError):
        pktgpu.flow_keys(c["batch"]["slab"], c["chain"], rss_key=b"short", stride=64)


# ------------------------------------------------------------------ the table
def run_both(table, model, k, weight="plen", base=0):
    """One update on the table and the model: statuses equal, the partition by flow_id equal to the model's."""
    fid, upd = table.update(k, weight=weight, base=base)
    w = k[weight] if isinstance(weight, str) else weight
    flow, want = model.update(k["keys"], k["hash"], k.get("dir"), w, k.get("status"), base)
    assert np.array_equal(np.asarray(upd), want), np.flatnonzero(np.asarray(upd) != want)[:8]
    assert F.same_partition(fid, flow)
    return np.asarray(fid), np.asarray(upd)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_table_against_the_model(n):
    rng = np.random.default_rng(n)
    for n_flows in (1, max(1, n // 7), n):  # one flow only; a few packets per flow; all packets distinct
        t, m = pktgpu.FlowTable(None, 8192), F.TableModel(8192)
        k, f = F.traffic(rng, n, n_flows)
        fid, upd = run_both(t, m, k)
        assert (upd == F.UPD_OK).all() and t.count() == len(set(f.tolist())) == len(m.e)
        F.check_records(t.flows(), m.records(), f"{n} {n_flows}")
        if n_flows == 1:
            r = t.flows()
            assert r["pkts"].sum() == n and r["bytes"].sum() == int(k["plen"].sum()) and r["first"][0] == 0
        t.close()


def test_three_updates_and_a_falling_base():
    rng = np.random.default_rng(8)
    t, m = pktgpu.FlowTable(None, 1024), F.TableModel(1024)
    k, _ = F.traffic(rng, 900, 200)
    k["status"][::13] = 2  # SKIPPED
    parts = [{c: v[a:b] for c, v in k.items()} for a, b in ((0, 300), (300, 301), (301, 900))]
    for p, base in zip(parts, (0, 1000, 5000)):
        run_both(t, m, p, base=base)
    F.check_records(t.flows(), m.records())
    with pytest.raises(RuntimeError):
        t.update(parts[0], base=5598)      # the high-water mark is 5000 + 599
    assert t.count() == len(m.e)
    run_both(t, m, parts[1], base=5599)
    run_both(t, m, parts[0], weight=None, base=1 << 40)   # no bytes counted
    run_both(t, m, {c: v for c, v in parts[2].items() if c in ("keys", "hash")}, weight=None, base=1 << 41)  # NULL dir, status
    F.check_records(t.flows(), m.records())
    t.close()


def test_slots_64_filled_and_overfilled():
    rng = np.random.default_rng(64)
    t, m = pktgpu.FlowTable(None, 64), F.TableModel(64)
    k, f = F.traffic(rng, 640, 64)
    fid, upd = run_both(t, m, k)
    assert (upd == F.UPD_OK).all() and t.count() == 64          # exactly full: no FULL
    F.check_records(t.flows(), m.records())
    t.clear()
    k, f = F.traffic(rng, 650, 65)
    fid, upd = t.update(k)
    lost = set(f[upd == F.UPD_FULL].tolist())
    assert len(lost) == 1 and (upd[f == lost.pop()] == F.UPD_FULL).all()  # exactly one flow's packets
    F.check_full(t, k, upd, fid, 64)
    fid2, upd2 = t.update(k, base=650)                           # the same flow loses again
    assert np.array_equal(upd2, upd) and np.array_equal(fid2, fid)
    F.check_full(t, {c: np.concatenate([v, v]) for c, v in k.items()}, np.concatenate([upd, upd]), np.concatenate([fid, fid]), 64)
    t.close()


def test_tag_bits_make_collisions():
    """tag_bits = 2 leaves three tags (0 is mapped to 1), so a table can hold three flows at most: the model
    must show at least one COLLISION and all three flows OK there; at tag_bits = 3 (seven tags) it must show
    at least one COLLISION and at least four OK flows.  Asserted on the model first, then on the table."""
    rng = np.random.default_rng(2)
    for bits, min_ok in ((2, 3), (3, 4)):
        k, f = F.traffic(rng, 400, 24)
        m = F.TableModel(256, bits)
        flow, want = m.update(k["keys"], k["hash"], k["dir"], k["plen"], k["status"], 0)
        assert (want == F.UPD_COLLISION).any() and len(set(flow[flow >= 0].tolist())) >= min_ok
        t = pktgpu.FlowTable(None, 256)
        t.set_tag_bits(bits)
        fid, upd = t.update(k)
        assert np.array_equal(upd, want) and F.same_partition(fid, flow) and (fid[upd == F.UPD_COLLISION] == F.NONE).all()
        F.check_records(t.flows(), m.records(), f"tag_bits {bits}")
        with pytest.raises(RuntimeError):
            t.set_tag_bits(64)             # not on a table that has seen an update
        t.clear()
        t.set_tag_bits(64)
        fid, upd = t.update(k)
        assert (upd == F.UPD_OK).all() and t.count() == 24
        t.close()


def test_export_cap_clear_and_refusals():
    rng = np.random.default_rng(5)
    t, m = pktgpu.FlowTable(None, 128), F.TableModel(128)
    k, _ = F.traffic(rng, 300, 40)
    fid, upd = run_both(t, m, k)
    full, cnt = t.export()
    assert cnt == 40 and len(full) == 40
    part, cnt = t.export(cap=7)
    assert cnt == 40 and part.tobytes() == full[:7].tobytes()   # ascending slot order, the first `cap`
    none, cnt = t.export(cap=0)
    assert cnt == 40 and len(none) == 0
    # flow_id is the slot: the packets of the j-th exported record carry the j-th lowest slot
    slots = np.unique(fid)
    for j in (0, 17, 39):
        i = int(np.flatnonzero(fid == slots[j])[0])
        assert full["key"][j].tobytes() == k["keys"][i].tobytes()
    t.clear()
    assert t.count() == 0 and len(t.flows()["first"]) == 0
    run_both(t, F.TableModel(128), k)                           # base starts again from 0
    L = _lib.load()
    h = ctypes.c_void_p()
    for slots in (0, 32, 96, 1 << 29):
        assert L.pkt_flow_table_create_host(slots, ctypes.byref(h)) == -1
    args, out, keep = t._update_args(k)
    assert L.pkt_flow_table_update(t._t, None, *args[1:], None) == -1
    assert L.pkt_flow_table_update(t._t, args[0], None, *args[2:], None) == -1
    assert L.pkt_flow_table_update(t._t, args[0] + 4, *args[1:], None) == -1      # keys not 8-byte aligned
    assert L.pkt_flow_table_update(t._t, *args[:5], 1 << 32, 1 << 50, None, None, None) == -1
    assert L.pkt_flow_table_update(None, *args, None) == -1
    assert L.pkt_flow_table_set_tag_bits(t._t, 0) == -1 and L.pkt_flow_table_set_tag_bits(t._t, 65) == -1
    assert b"bits" in L.pkt_flow_table_last_error(t._t)
    assert L.pkt_flow_table_update(t._t, *args[:5], 0, 1 << 50, None, None, None) == 0  # n == 0 moves the mark
    with pytest.raises(RuntimeError):
        t.update(k, base=5)
    assert t.count() == 40
    t.close()


def test_keys_from_packets_into_the_table():
    """flow_keys' dict straight into update: the symmetric case's connections, bytes by direction."""
    c, want = F.all_cases()["symmetric"]
    k = keys_of(c)
    t, m = pktgpu.FlowTable(None, 64), F.TableModel(64)
    run_both(t, m, k)
    r = t.flows()
    F.check_records(r, m.records())
    assert (r["pkts"][0] == [1, 1]).all() and r["bytes"][0].tolist() == [int(k["plen"][0]), int(k["plen"][1])]
    c, want = F.all_cases()["span_lens"]
    k = keys_of(c)
    fid, upd = run_both(t, m, k, base=100)
    assert (upd[want["status"] != 0] == F.UPD_SKIPPED).all()
    t.close()
