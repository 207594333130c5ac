"""pkt_extract_fields, pkt_set_fields, pkt_set_fields_csum, pkt_ipv4_update_checksum, pkt_ipv4_checksum_batch and
pkt_broadcast: the kernels of pktgpu_rewrite.hip against rewrite_cases' yardstick (Python integers; checked against
the C oracle on the CPU by test_rewrite_cases.py), one test per (case, call).  The slab and every output lie
between 4096-byte guard regions filled with 0xA5 (the slab's guard starts at byte slab_len, not at the next
multiple of 16) and the outputs start as 0x77, so that a byte the call must not write is seen; chain, index and
value inputs are compared with their originals after the call.  Every comparison is byte for byte."""
import ctypes

import numpy as np
import pytest

import pktgpu

import rewrite_cases as R

pytestmark = pytest.mark.gpu
GUARD = 4096
FILL = 0x77


@pytest.fixture(scope="module")
def P():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible")
    return pktgpu.Parser(0)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


class Guarded:
    """Buffers of the given sizes in one 0xA5-filled device allocation, GUARD bytes before and after each (buffer k
    starts shifts[k] bytes past a 16-byte boundary); fills[k] is a byte value or the buffer's bytes."""

    def __init__(self, sizes, fills, shifts=None):
        self.at, pos = [], GUARD
        for k, s in enumerate(sizes):
            pos += shifts[k] if shifts else 0
            self.at.append((pos, s))
            pos = (pos + s + 15) // 16 * 16 + GUARD
        h = np.full(pos, 0xA5, np.uint8)
        for (p, s), f in zip(self.at, fills):
            h[p:p + s] = f
        self.t = dev(h)
        assert self.t.data_ptr() % 16 == 0

    def ptr(self, k):
        return self.t.data_ptr() + self.at[k][0]

    def view(self, k):
        p, s = self.at[k]
        return self.t[p:p + s]

    def read(self):
        """([each buffer's bytes], every guard byte still 0xA5)."""
        import torch
        torch.cuda.synchronize()
        h = self.t.cpu().numpy()
        bufs = [h[p:p + s].copy() for p, s in self.at]
        for p, s in self.at:
            h[p:p + s] = 0xA5
        return bufs, bool((h == 0xA5).all())


_INPUTS = {}


def inputs(name):
    """The case's index, chain and value arrays on the device, once per case."""
    if name not in _INPUTS:
        c = R.case(name)
        b = c["batch"]
        _INPUTS[name] = dict(offsets=None if b["offsets"] is None else dev(b["offsets"]),
                             lens=None if b["lens"] is None else dev(b["lens"]),
                             chain={k: dev(v) for k, v in c["chain"].items()}, values=[dev(v) for v in c["values"]])
    return _INPUTS[name]


def inputs_unchanged(name):
    c, d = R.case(name), inputs(name)
    b = c["batch"]
    same = all(np.array_equal(d["chain"][k].cpu().numpy(), v) for k, v in c["chain"].items())
    same &= all(np.array_equal(t.cpu().numpy(), v) for t, v in zip(d["values"], c["values"]))
    for k in ("offsets", "lens"):
        same &= d[k] is None or np.array_equal(d[k].cpu().numpy(), b[k])
    return bool(same)


def spec_array(P, specs):
    sp = (P._lib.PktFieldSpec * max(1, len(specs)))()
    for k, (t, occ, s, e) in enumerate(specs):
        sp[k] = P._lib.PktFieldSpec(t, occ, s, e, 0)
    return sp


def ptr_array(ptrs):
    return (ctypes.c_void_p * max(1, len(ptrs)))(*ptrs)


def slab_between_guards(P, name):
    b, d = R.case(name)["batch"], inputs(name)
    g = Guarded([b["slab"].size], [b["slab"]])
    return g, P._batch(g.view(0), b["n"], b["stride"], d["offsets"], d["lens"]), P._chain(d["chain"])


def run_write(P, name, call):
    """A setter / refresh call on a fresh guarded copy of the slab -> (rc, the slab afterwards, guards intact)."""
    c, d = R.case(name), inputs(name)
    g, b, ch = slab_between_guards(P, name)
    st = P._stream(None)
    if call.startswith("update"):
        rc = P._L.pkt_ipv4_update_checksum(P._ctx, ctypes.byref(b), ctypes.byref(ch), int(call[-1]), st)
    else:
        sp, vp = spec_array(P, c["specs"]), ptr_array([v.data_ptr() for v in d["values"]])
        if call == R.SET:
            rc = P._L.pkt_set_fields(P._ctx, ctypes.byref(b), ctypes.byref(ch), sp, len(c["specs"]), vp, st)
        else:
            rc = P._L.pkt_set_fields_csum(P._ctx, ctypes.byref(b), ctypes.byref(ch), sp, len(c["specs"]), vp, int(call[-1]), st)
    (slab,), intact = g.read()
    return rc, slab, intact


def run_get(P, name, out_of=None, found="all"):
    """pkt_extract_fields with spec k writing output buffer out_of[k] (default: its own); found = "all", None (a
    NULL array) or the index of the one spec given a NULL found pointer.
    -> (rc, [values buffer], [found buffer], output guards intact, slab unchanged and its guards intact)."""
    c = R.case(name)
    n, k = c["batch"]["n"], len(c["specs"])
    out_of = list(range(k)) if out_of is None else out_of
    nb = max(out_of) + 1
    g, b, ch = slab_between_guards(P, name)
    out = Guarded([8 * n] * nb + [n] * nb, [FILL] * (2 * nb))
    vp = ptr_array([out.ptr(o) for o in out_of])
    fp = None if found is None else ptr_array([None if found == j else out.ptr(nb + o) for j, o in enumerate(out_of)])
    rc = P._L.pkt_extract_fields(P._ctx, ctypes.byref(b), ctypes.byref(ch), spec_array(P, c["specs"]), k, vp, fp, P._stream(None))
    bufs, intact = out.read()
    (slab,), slab_ok = g.read()
    return (rc, [x.view(np.uint64) for x in bufs[:nb]], bufs[nb:], intact,
            slab_ok and np.array_equal(slab, c["batch"]["slab"]))


def same(got, want, label):
    bad = np.flatnonzero(np.asarray(got) != want)
    assert bad.size == 0, (label, "first bad", bad[:8], np.asarray(got)[bad[:8]], np.asarray(want)[bad[:8]])


# ------------------------------------------------------------------ cases a - h
@pytest.mark.parametrize("name,call", R.CALLS)
def test_case(P, name, call):
    c = R.case(name)
    want = R.expected(name, call)
    if call == R.GET:
        rc, vals, found, intact, slab_ok = run_get(P, name)
        assert rc == 0 and intact and slab_ok
        for k, sp in enumerate(c["specs"]):   # by the caller's index, however the library groups the specs
            same(vals[k], want[0][k], (name, "values", k, sp))
            same(found[k], want[1][k], (name, "found", k, sp))
    else:
        rc, slab, intact = run_write(P, name, call)
        assert rc == 0
        same(slab, want, (name, call))
        assert intact
    assert inputs_unchanged(name)


@pytest.mark.parametrize("name", ["shapes-gaps-257", "shapes-s64-65", "counts-gaps-33", "sweep-gaps"])
def test_null_found_leaves_the_fill(P, name):
    c = R.case(name)
    want = R.expected(name, R.GET)
    rc, vals, found, intact, slab_ok = run_get(P, name, found=None)
    assert rc == 0 and intact and slab_ok
    assert all((f == FILL).all() for f in found)
    for k in range(len(c["specs"])):
        same(vals[k], want[0][k], (name, "values", k))
    for skip in (0, len(c["specs"]) - 1, len(c["specs"]) // 2):
        rc, vals, found, intact, slab_ok = run_get(P, name, found=skip)
        assert rc == 0 and intact and slab_ok
        for k in range(len(c["specs"])):
            same(vals[k], want[0][k], (name, "values", k))
            if k == skip:
                assert (found[k] == FILL).all(), (name, skip)
            else:
                same(found[k], want[1][k], (name, "found", k, "without", skip))


@pytest.mark.parametrize("k", [k for k in R.NSPECS if k >= 2])
@pytest.mark.parametrize("layout", ["gaps", "s64"])
def test_shared_output_pointers_keep_the_callers_order(P, layout, k):
    """Specs 2j and 2j + 1 write the same values and found arrays: what is left is the later spec's result."""
    name = f"counts-{layout}-{k}"
    want = R.expected(name, R.GET)
    out_of = R.alias_outputs(k)
    rc, vals, found, intact, slab_ok = run_get(P, name, out_of=out_of)
    assert rc == 0 and intact and slab_ok
    differ = 0
    for o in range(max(out_of) + 1):
        last = max(j for j in range(k) if out_of[j] == o)
        same(vals[o], want[0][last], (name, "values of buffer", o))
        same(found[o], want[1][last], (name, "found of buffer", o))
        differ += any(not np.array_equal(want[0][j], want[0][last]) for j in range(k) if out_of[j] == o)
    assert differ >= (k // 2 + 1) // 2   # the order matters: the earlier spec's result is another


# ------------------------------------------------------------------ i. checksum batch
@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("stride", R.CSUM_STRIDES)
@pytest.mark.parametrize("n", R.CSUM_N)
def test_checksum_batch(P, n, stride, shift):
    buf, want, differ, _ = R.csum_case(n, stride)
    assert n < 63 or differ >= n / 8
    g = Guarded([buf.size, 2 * n], [buf, FILL], [shift, 0])
    assert g.ptr(0) % 16 == shift
    rc = P._L.pkt_ipv4_checksum_batch(P._ctx, g.ptr(0), stride, n, g.ptr(1), P._stream(None))
    (src, out), intact = g.read()
    assert rc == 0 and intact and np.array_equal(src, buf)
    same(out.view(np.uint16), want, (n, stride, shift))


# ------------------------------------------------------------------ j. broadcast
@pytest.mark.parametrize("n", R.BCAST_N)
@pytest.mark.parametrize("length,stride", R.BCAST)
def test_broadcast(P, length, stride, n):
    src, want = R.bcast_case(length, stride, n)
    g = Guarded([length, n * stride], [np.frombuffer(src, np.uint8), FILL])
    rc = P._L.pkt_broadcast(P._ctx, g.ptr(0), length, n, stride, g.ptr(1), P._stream(None))
    (s, out), intact = g.read()
    assert rc == 0 and intact and s.tobytes() == src
    same(out, want, (length, stride, n))


def test_broadcast_past_the_grid_cap(P):
    """More 16-byte chunks than the capped grid has threads: the grid-stride loop's second trip.  67 MB: the
    expectation is built and compared on the device."""
    import torch
    length, stride, n = R.BCAST_BIG
    src = dev(np.arange(1, length + 1, dtype=np.uint8))
    big = torch.full((GUARD + n * stride + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    out = big[GUARD:GUARD + n * stride]
    out.fill_(FILL)
    assert out.data_ptr() % 16 == 0
    rc = P._L.pkt_broadcast(P._ctx, src.data_ptr(), length, n, stride, out.data_ptr(), P._stream(None))
    torch.cuda.synchronize()
    assert rc == 0
    want = torch.zeros((n, stride), dtype=torch.uint8, device="cuda")
    want[:, :length] = src
    assert torch.equal(out.view(n, stride), want)
    assert bool((big[:GUARD] == 0xA5).all()) and bool((big[GUARD + n * stride:] == 0xA5).all())
