"""pkt_reasm_host (the CPU twin of pktgpu_reasm.hip: the classification, the joined header and the refusals of
pktgpu_reasm.hpp, which the kernels share; the grouping by a sort and a walk) against reasm_cases' yardstick, an
independent Python model written from the text of include/pktgpu.h, and against what each case writes down."""
import ctypes

import numpy as np
import pytest

import pktgpu
from pktgpu import schema

import compare_cases as C
import frag_cases as G
import reasm_cases as R

INVALID = -1
# argument positions of pkt_reasm_host
A_BATCH, A_CHAIN, A_WHICH, A_FLAGS, A_SELECT, A_STATUS, A_INDEX, A_DST, A_DST_LEN, A_CAP, A_OFF, A_LEN, A_SRC, A_NFRAG, \
    A_OCHAIN, A_HITS = range(16)


def run(items, select=None, which=0, flags=0, kind="indexed", **kw):
    b, ch = R.layout(items, kind)
    want = R.expect(b, ch, select, which, flags)
    rc, got = R.host_call(b, ch, select, which, flags, **kw)
    return rc, got, want, b, ch


# ------------------------------------------------------------------ 1. the case list, both layouts
@pytest.mark.parametrize("kind", ["indexed", "stride"])
@pytest.mark.parametrize("name", R.CASES)
def test_cases(name, kind):
    c = R.get_case(name)
    rc, got, want, b, _ = run(c["items"], c["select"], c["which"], kind=kind)
    assert rc == 0 and got["guards"]
    if kind == "indexed" and b["n"] >= 16:
        assert {int(o) % 16 for o in b["offsets"][:16]} == set(range(16))
    R.check(got, want, got["cap"], name)
    R.check_case(name, c, got, want)
    assert int(got["hits"].sum()) == b["n"]


def test_a_known_answer_written_out_by_hand():
    """Two fragments of a 30-byte payload, the second one first: one output at the place of the first fragment, which
    arrives last; total length 50, flags and offset 0, and a header that sums to 0xFFFF again."""
    pay = bytes(range(30))
    rc, got, want, _, _ = run([R.mkfrag(pay, 24, 6, False, 0x4242), R.mkfrag(pay, 0, 24, True, 0x4242)])
    assert rc == 0 and got["status"].tolist() == [R.JOINED, R.JOINED] and got["out_index"].tolist() == [0, 0]
    assert (got["n_out"], got["bytes_out"]) == (1, 64) and got["src_index"].tolist() == [1] and got["nfrag"].tolist() == [2]
    p = got["dst"][:64].tobytes()
    assert got["out_len"].tolist() == [64] and p[34:64] == pay
    assert R.be16(p, 16) == 50 and R.be16(p, 20) == 0 and R.be16(p, 18) == 0x4242 and G.rfc1071(p[14:34]) == 0xFFFF
    assert p[:14] == R.l2(False) and got["oc_n_hdrs"].tolist() == [2]


# ------------------------------------------------------------------ 2. the shapes the kernels' boundaries ask for
def test_one_datagram_of_300_eight_byte_fragments():
    orig = R.dgram(G.pattern(2400, 5), 0x0A01)
    g = R.frags(orig, 28)
    assert len(g) == 300
    for order in ("reversed", "shuffled"):
        rc, got, want, _, _ = run(R.arrange([g], order))
        assert rc == 0 and got["guards"] and (want["status"] == R.JOINED).all() and got["nfrag"].tolist() == [300]
        R.check(got, want, got["cap"], order)
        assert got["dst"][:got["out_len"][0]].tobytes() == R.original(orig)


def one_key(n, spoil):
    pay = G.pattern(8 * n, 3)
    g = [R.mkfrag(pay, 8 * k, 8, k + 1 < n, 0x0B01) for k in range(n)]
    g = R.arrange([g], "shuffled", seed=9)
    if spoil:
        g[n // 2] = g[n // 3]
    return g


@pytest.mark.parametrize("spoil", [False, True])
def test_900_packets_sharing_one_key(spoil):
    rc, got, want, _, _ = run(one_key(900, spoil))
    assert rc == 0 and got["guards"]
    assert (want["status"] == (R.PENDING if spoil else R.JOINED)).all() and got["n_out"] == (0 if spoil else 1)
    R.check(got, want, got["cap"], "one key")


def mixed():
    return R.cached("mix600", lambda: R.mix(600))


def test_mix_against_the_model_with_select():
    items, sel = mixed()
    rc, got, want, _, _ = run(items, sel)
    assert rc == 0 and got["guards"]
    counts = np.bincount(want["status"], minlength=R.NSTATUS)
    assert all(counts[s] >= 3 for s in (R.WHOLE, R.JOINED, R.PENDING, R.SKIPPED, R.NO_IP, R.BAD_HDR)), counts
    R.check(got, want, got["cap"], "mix")
    assert int(got["hits"].sum()) == len(items)
    assert sum(k > 1 for k in want["nfrag"]) >= 10


# ------------------------------------------------------------------ 3. call-level behaviour
def test_only_joined_and_no_write_totals():
    items, sel = mixed()
    for flags in (0, R.ONLY_JOINED):
        rc, got, want, b, ch = run(items, sel, flags=flags)
        assert rc == 0
        R.check(got, want, got["cap"], f"flags {flags}")
        rc, plan = R.host_call(b, ch, sel, flags=flags | R.NO_WRITE)
        assert rc == 0 and plan["guards"] and "dst" not in plan
        assert (plan["n_out"], plan["bytes_out"]) == (got["n_out"], got["bytes_out"])
        for k in ("status", "out_index", "hits"):
            assert np.array_equal(plan[k], got[k]), k
    assert (want["out_index"][want["status"] == R.WHOLE] == R.NONE).all() and all(k > 1 for k in want["nfrag"])


NULLABLE = ["status", "out_index", "src_index", "nfrag", "oc_n_hdrs", "oc_hdr_type", "oc_hdr_off", "hits"]


@pytest.mark.parametrize("mask", list(range(256)))
def test_null_output_combinations(mask):
    items, sel = R.cached("mix150", lambda: R.mix(150, seed=5))
    skip = [k for j, k in enumerate(NULLABLE) if mask >> j & 1]
    rc, got, want, _, _ = run(items, sel, skip=skip)
    assert rc == 0 and got["guards"]
    R.check(got, want, got["cap"], str(skip))


def test_null_out_chain_itself():
    items, sel = R.cached("mix150", lambda: R.mix(150, seed=5))
    rc, got, want, _, _ = run(items, sel, over={A_OCHAIN: None})
    assert rc == 0 and got["guards"] and (got["oc_n_hdrs"] == 0xA5).all()
    got = {k: v for k, v in got.items() if not k.startswith("oc_")}
    R.check(got, want, got["cap"], "no out_chain")


def test_empty_tail_up_to_out_cap_and_dst_untouched_past_the_total():
    items, sel = R.cached("mix150", lambda: R.mix(150, seed=5))
    b, ch = R.layout(items)
    want = R.expect(b, ch, sel)
    cap, room = want["n_out"] + 77, want["bytes_out"] + 4096
    rc, got = R.host_call(b, ch, sel, cap=cap, dst_len=room)
    assert rc == 0 and got["guards"]
    R.check(got, want, cap)
    assert (got["dst_rest"][want["bytes_out"]:] == 0xA5).all()


def test_overflow_returns_both_totals_for_each_cause():
    items, sel = R.cached("mix150", lambda: R.mix(150, seed=5))
    b, ch = R.layout(items)
    want = R.expect(b, ch, sel)
    for cap, room in ((want["n_out"] - 1, want["bytes_out"]), (want["n_out"], want["bytes_out"] - 1), (want["n_out"], want["bytes_out"] - 16)):
        rc, got = R.host_call(b, ch, sel, cap=cap, dst_len=room)
        assert rc == INVALID and got["guards"]
        assert (got["n_out"], got["bytes_out"]) == (want["n_out"], want["bytes_out"])
        for k in ("status", "hits"):
            assert np.array_equal(got[k], want[k]), k
    rc, got = R.host_call(b, ch, sel, cap=want["n_out"], dst_len=want["bytes_out"])
    assert rc == 0
    R.check(got, want, want["n_out"])


def test_n_0_and_n_1():
    b, ch = R.layout([R.dgram(G.pattern(100, 1), 1)])
    b0 = dict(b, n=0, offsets=b["offsets"][:0], lens=b["lens"][:0])
    ch0 = {k: v[..., :0] for k, v in ch.items()}
    rc, got = R.host_call(b0, ch0, cap=5, dst_len=64)
    assert rc == 0 and got["guards"] and (got["n_out"], got["bytes_out"]) == (0, 0)
    assert (got["out_off"] == 0).all() and (got["out_len"] == 0).all() and (got["src_index"] == R.NONE).all()
    assert (got["nfrag"] == 0).all() and (got["oc_n_hdrs"] == 0).all() and (got["dst_rest"] == 0xA5).all()
    rc, got = R.host_call(b0, ch0, flags=R.NO_WRITE)
    assert rc == 0 and (got["n_out"], got["bytes_out"]) == (0, 0)
    for item, st in ((R.dgram(G.pattern(100, 1), 1), R.WHOLE), (R.mkfrag(G.pattern(100, 1), 0, 48, True, 1), R.PENDING)):
        rc, got, want, _, _ = run([item])
        assert rc == 0 and got["guards"] and got["status"].tolist() == [st] and got["n_out"] == (1 if st == R.WHOLE else 0)
        R.check(got, want, got["cap"], "n = 1")


def refusals():
    from pktgpu import _lib
    odd = np.zeros(64, np.uint8)
    base = odd.ctypes.data
    r = {"null_batch": {A_BATCH: None}, "null_chain": {A_CHAIN: None}, "which_16": {A_WHICH: 16}, "which_0xFE": {A_WHICH: 0xFE},
         "flag_bit_4": {A_FLAGS: 4}, "flag_bit_31": {A_FLAGS: 1 << 31}, "dst_misaligned": {A_DST: base + 8},
         "hits_misaligned": {A_HITS: base + 4}, "out_off_misaligned": {A_OFF: base + 4}, "null_dst": {A_DST: None},
         "null_out_off": {A_OFF: None}, "null_out_len": {A_LEN: None}, "out_cap_0": {A_CAP: 0}, "out_cap_2_32": {A_CAP: 1 << 32}}
    for col in ("n_hdrs", "hdr_type", "hdr_off"):
        ch = _lib.PktChain(base, base, base)
        setattr(ch, col, None)
        r[f"null_chain_{col}"] = {A_CHAIN: ctypes.byref(ch)}
    return r, (odd,)


REFUSALS = sorted(refusals()[0])


@pytest.mark.parametrize("name", REFUSALS)
def test_refusals(name):
    over, keep = refusals()
    b, ch = R.layout(R.five(0x0201))
    rc, got = R.host_call(b, ch, over=over[name], cap=8, dst_len=4096)
    assert rc == INVALID and got["guards"]
    assert (got["status"] == 0xA5).all() and (got["dst_rest"] == 0xA5).all() and (got["hits"] == 0).all()


@pytest.mark.parametrize("form", ["n_2_32", "offsets_without_lens", "stride_0", "null_slab"])
def test_batch_refusals(form):
    from pktgpu import _lib
    L = _lib.load()
    b, ch = R.layout(R.five(0x0201))
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
    tot, cnt = ctypes.c_uint64(7), ctypes.c_uint64(7)
    rc = L.pkt_reasm_host(ctypes.byref(pb), ctypes.byref(pc), 0, schema.REASM_NO_WRITE, None, None, None, None, 0, 0, None, None,
                          None, None, None, None, ctypes.byref(tot), ctypes.byref(cnt))
    assert rc == INVALID and (tot.value, cnt.value) == (0, 0)


# ------------------------------------------------------------------ 4. Parser.reassemble, and the next calls take the output
def test_reassemble_host_sizes_itself_and_gives_the_pending_mask():
    items, sel = mixed()
    b, ch = R.layout(items)
    want = R.expect(b, ch, sel)
    r = pktgpu.Parser.reassemble(None, b, ch, select=sel, hits=True, host=True)
    assert (r.n_out, r.bytes_out) == (want["n_out"], want["bytes_out"]) and np.array_equal(r.status, want["status"])
    assert np.array_equal(r.pending, want["status"] == R.PENDING) and r.pending.any()
    assert np.array_equal(r.hits, want["hits"]) and np.array_equal(r.out_index, want["out_index"])
    got = dict(dst=r.slab, out_off=r.offsets, out_len=r.lens, src_index=r.src_index, nfrag=r.nfrag, n_out=r.n_out, bytes_out=r.bytes_out,
               oc_n_hdrs=r.out_chain["n_hdrs"], oc_hdr_type=r.out_chain["hdr_type"], oc_hdr_off=r.out_chain["hdr_off"])
    R.check(got, want, max(1, r.n_out), "Parser.reassemble")
    plan = pktgpu.Parser.reassemble(None, b, ch, select=sel, plan_only=True, host=True)
    assert (plan.n_out, plan.bytes_out) == (r.n_out, r.bytes_out) and plan.slab is None
    with pytest.raises(ValueError):
        pktgpu.Parser.reassemble(None, b, ch, select=sel, out_cap=r.n_out - 1, dst_bytes=r.bytes_out, host=True)


def test_l4_checksum_is_ok_over_the_joined_datagram_and_fragment_before():
    orig = R.udp_dgram(1000, 0x0C01, seed=2)
    g = R.frags(orig, 576)
    b, ch = R.layout([g[1], g[0]])
    before = pktgpu.l4_checksum(b["slab"], C.chain_of(b), offsets=b["offsets"], lens=b["lens"])
    assert (before["status"] == pktgpu.L4_FRAGMENT).all()
    r = pktgpu.Parser.reassemble(None, b, ch, host=True)
    assert r.n_out == 1 and r.slab[:r.lens[0]].tobytes() == orig[0]
    ob = C.batch(r.slab, r.offsets[:1], r.lens[:1])
    after = pktgpu.l4_checksum(ob["slab"], C.chain_of(ob), offsets=ob["offsets"], lens=ob["lens"])
    assert after["status"].tolist() == [pktgpu.L4_OK]
