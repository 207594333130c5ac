"""Bounded-memory capture streams: pkt_pcap_stream_release / _room / _released / _batch (include/pktgpu.h).

The stream holds a WINDOW of the capture (the global header, then the bytes from the first unreleased
record on) in max_bytes of device memory; the consumer polls, uses the window's columns and packets and
releases the records it is done with.  Every capture here is many times its stream's max_bytes.

The reference is computed once per capture, on the WHOLE capture, and never changed: gen.pcap_index_py
for the records, oracle.parse_batch for the columns (reference src/parser/fast.rs:5-227).  A window that
has released R records and B bytes must report, for its m records, the slice [R, R + m) of both, with
offsets = the whole capture's minus B.  The driver (_Ring) also models the window's size from the
records alone, so room() and released() are checked against the model at every step, and which of the
release's move paths each cut takes (disjoint, overlapping chunks, temporary buffer) is known from the
model, not from the library."""
import functools
import struct

import numpy as np
import pytest

import oracle
from pktgpu import gen, schema

pytestmark = pytest.mark.gpu

SLOT = ("hdr_type", "hdr_off")
KiB = 1 << 10


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need an MI355X")


class _Capture:
    """A capture and its reference over the whole of it (read-only)."""

    def __init__(self, buf):
        self.a = np.frombuffer(bytes(buf), np.uint8)
        self.offs, self.lens = gen.pcap_index_py(bytes(buf))
        self.n = len(self.offs)
        self.ref = oracle.parse_batch(self.a, self.n, offsets=self.offs, lens=self.lens, nthreads=8)
        self.hdr = self.offs.astype(np.int64) - 16                 # record header starts
        self.end = self.offs.astype(np.int64) + self.lens.astype(np.int64)
        for v in (self.a, self.offs, self.lens, self.hdr, self.end, *self.ref.values()):
            v.setflags(write=False)


@functools.lru_cache(maxsize=None)
def _c4():
    buf, _, _ = gen.gen_c4(20_000, seed=4242)
    return _Capture(buf.tobytes())


def _awkward_payloads():
    """As tests/test_pcap_stream.py::test_long_records_and_fake_chains: 1 500 records of 1 B to 70 KB,
    zero-filled long ones, payloads that are chains of plausible record headers."""
    rng = np.random.default_rng(9)
    pays = []
    for _ in range(1500):
        r = rng.random()
        if r < 0.1:
            pays.append(bytes(int(rng.integers(4096, 70000))))
        elif r < 0.3:
            inner = bytearray()
            for _ in range(int(rng.integers(1, 6))):
                L = int(rng.integers(1, 40))
                inner += struct.pack("<IIII", 1, 2, L, L) + rng.integers(0, 256, L, dtype=np.uint8).tobytes()
            pays.append(bytes(inner))
        else:
            pays.append(rng.integers(0, 256, int(rng.integers(1, 400)), dtype=np.uint8).tobytes())
    return pays


def _records(payloads):
    out = bytearray(gen.PCAP_GLOBAL_HEADER)
    for i, p in enumerate(payloads):
        out += struct.pack("<IIII", i, 0, len(p), len(p)) + bytes(p)
    return bytes(out)


@functools.lru_cache(maxsize=None)
def _awkward():
    return _Capture(_records(_awkward_payloads()))


def _move_path(kept, freed):
    """The path pkt_pcap_stream_release's move takes for `kept` bytes moved down by `freed`."""
    if kept == 0:
        return "none"
    chunks = -(-kept // freed)
    return "disjoint" if chunks == 1 else ("chunks" if chunks <= 64 else "temp")


class _Ring:
    """One stream over a _Capture, with the model of its window beside it."""

    def __init__(self, cap_, max_bytes, cap, step_bytes=0, pinned=False, scan64=False, columns="all", total=None):
        from pktgpu.stream import PcapStream
        self.C = cap_
        self.total = self.C.a.size if total is None else total  # bytes of the capture that will be pushed
        self.max_bytes, self.cap = max_bytes, cap
        self.st = PcapStream(0, max_bytes=max_bytes, cap=cap, columns=columns, out="pinned" if pinned else None,
                             step_bytes=step_bytes)
        if scan64:
            assert self.st._L.pkt_ctx_set_pcap_scan64(self.st.ctx(), 1) == 0
        self.pos = 0          # capture bytes pushed
        self.rel_rec = 0      # the model's released totals
        self.rel_bytes = 0
        self.c = 0            # the last poll's count
        self.paths = []       # the move path of every release
        self.label = f"max_bytes={max_bytes} cap={cap} step={step_bytes} pinned={pinned} scan64={scan64}"

    def close(self):
        self.st.close()

    def room(self):
        r = self.st.room()
        assert r == self.max_bytes - (self.pos - self.rel_bytes), (self.label, self.pos, self.rel_bytes, r)
        return r

    def push(self, m):
        m = int(m)
        assert 0 <= m <= self.total - self.pos
        self.st.push(self.C.a[self.pos:self.pos + m])
        self.pos += m

    def whole(self):
        """Records of the capture wholly inside the bytes pushed."""
        return int(np.searchsorted(self.C.end, self.pos, side="right"))

    def column(self, k, m):
        g = self.st.out[k]
        g = g[:, :m] if k in SLOT else g[:m]
        return g.cpu().numpy() if hasattr(g, "cpu") else np.asarray(g)

    def check(self, c, idx, want_c):
        """The window's count, index and every column against the slice of the whole capture's."""
        C, R = self.C, self.rel_rec
        assert c == want_c, (self.label, "count", self.pos, R, c, want_c)
        m = min(c, self.cap)
        assert len(idx[0]) == m and len(idx[1]) == m
        assert np.array_equal(idx[0].astype(np.int64), C.offs[R:R + m].astype(np.int64) - self.rel_bytes), (self.label, "offsets", R)
        assert np.array_equal(idx[1], C.lens[R:R + m]), (self.label, "lens", R)
        nh = C.ref["n_hdrs"][R:R + m].astype(np.int64)
        for k in self.st.out:
            gv = self.column(k, m)
            ov = C.ref[k][:, R:R + m] if k in SLOT else C.ref[k][R:R + m]
            if k in SLOT:
                valid = np.arange(schema.MAX_HDRS)[:, None] < nh[None, :]
                assert not (valid & (gv != ov)).any(), (self.label, k, R, m)
            else:
                assert np.array_equal(gv, ov), (self.label, k, R, m)
        return m

    def poll(self):
        c, idx = self.st.poll(index=True)
        self.c = c
        return c, self.check(c, idx, self.whole() - self.rel_rec)

    def release(self, n=None):
        """release(n) (None: everything the columns hold), then released() and room() against the model."""
        k = min(self.c, self.cap) if n is None else int(n)
        self.st.release(n)
        if k:
            p = int(self.C.end[self.rel_rec + k - 1])          # the cut, as a capture offset
            freed = p - 24 - self.rel_bytes
            self.paths.append((_move_path(self.pos - p, freed), self.pos - p, freed))
            self.rel_rec += k
            self.rel_bytes = p - 24
            self.c = 0
        assert self.st.released() == (self.rel_rec, self.rel_bytes), self.label
        self.room()

    def finish(self, want_total=None):
        """finish, the last window checked, and the totals: released + final count = the capture's."""
        want_total = self.C.n if want_total is None else want_total
        c, idx = self.st.finish()
        self.check(c, idx, want_total - self.rel_rec)
        r, b = self.st.released()
        assert r + c == want_total
        assert (r, b) == (self.rel_rec, self.rel_bytes)
        assert b == (int(self.C.end[r - 1]) - 24 if r else 0)
        return c


def _push_sizes(rng):
    sizes = rng.integers(1, 60_000, 64)
    sizes[::5] = rng.integers(1, 40, len(sizes[::5]))
    return sizes


def _drive(R, rng, pick):
    """Push min(random size, room()); when room() falls below the next push, or every few pushes, poll
    with the index, check the window and release pick(c, m) records; finish at the end."""
    sizes = _push_sizes(rng)
    k = windows = 0
    while R.pos < R.total:
        want = min(int(sizes[k % len(sizes)]), R.total - R.pos)
        if R.room() < want or k % 9 == 8:
            c, m = R.poll()
            R.release(pick(c, m))
            windows += 1
            if R.room() == 0:  # the window is still full: hand back everything it holds
                c, m = R.poll()
                assert m > 0, "a record larger than the window"
                R.release(m)
        R.push(min(want, R.room()))
        k += 1
    R.finish()
    return windows


@pytest.mark.parametrize("step", [1, 4096, 0])
@pytest.mark.parametrize("pinned", [False, True])
def test_release_everything_many_windows(step, pinned):
    """A 3.7 MB C4 capture through a 256 KiB window, pushes of 1 B to 60 KB, everything polled released:
    at least 14 windows, each equal to its slice of the whole capture's index and columns."""
    C = _c4()
    R = _Ring(C, 256 * KiB, 4096, step_bytes=step, pinned=pinned)
    try:
        windows = _drive(R, np.random.default_rng(100 + step), lambda c, m: None)
        assert windows >= 14 and C.a.size > 14 * 256 * KiB
    finally:
        R.close()


def test_partial_releases():
    """n drawn uniformly from [0, min(c, cap)] (0 and min(c, cap) forced at least once each): the kept
    records, indexed and parsed again in the new window, must again equal the oracle's."""
    C = _c4()
    rng = np.random.default_rng(77)
    picked = []

    def pick(c, m):
        # forced: nothing, everything, one record under a full window (kept > 64 x freed: the temporary
        # buffer), a third (kept = 2 x freed: overlapping chunks)
        n = {2: 0, 4: m, 6: min(1, m), 8: m // 3}.get(len(picked), int(rng.integers(0, m + 1)))
        picked.append((n, m))
        return n

    R = _Ring(C, 256 * KiB, 4096, step_bytes=4096)
    try:
        _drive(R, rng, pick)
        assert any(n == 0 for n, m in picked) and any(n == m and m > 0 for n, m in picked)
        assert any(0 < n < m for n, m in picked)
        assert {"temp", "chunks"} <= {p[0] for p in R.paths}  # small releases with a large kept tail among them
    finally:
        R.close()


def test_cap_as_batch_size():
    """cap = 300 under windows of about 1 400 records: every poll counts more than the columns hold, and
    release(cap) walks the capture in batches of 300, the records past cap parsed in the next window —
    none skipped, none twice: the windows' columns concatenated are the oracle's."""
    C = _c4()
    cap = 300
    names = ("ipv4_identification", "payload_len", "status")
    got = {k: [] for k in names}
    rng = np.random.default_rng(5)
    sizes = _push_sizes(rng)
    R = _Ring(C, 256 * KiB, cap, step_bytes=4096)
    try:
        k = 0
        while R.pos < R.total:
            want = min(int(sizes[k % len(sizes)]), R.total - R.pos)
            if R.room() < want:
                c, m = R.poll()
                assert c > cap and m == cap, (c, cap)
                for kk in names:
                    got[kk].append(R.column(kk, cap).copy())
                R.release(cap)
            R.push(min(want, R.room()))
            k += 1
        while True:  # every byte is in: drain the last window by the batch
            c, m = R.poll()
            if c <= cap:
                break
            for kk in names:
                got[kk].append(R.column(kk, cap).copy())
            R.release(cap)
        c = R.finish()
        assert R.rel_rec % cap == 0 and R.rel_rec // cap >= 60
        for kk in names:
            got[kk].append(R.column(kk, c).copy())
            assert np.array_equal(np.concatenate(got[kk]), C.ref[kk]), kk
    finally:
        R.close()


def _awkward_schedule(C, max_bytes):
    """Poll positions (capture offsets) and the records to release at each (None: all) for the awkward
    capture: the window's tail at a poll is 1..15 bytes of a record header, a whole header with no
    payload byte, half a payload, all but the last byte of a long record that follows few small ones
    (the kept bytes exceed the freed ones), nothing (the cut at a record's end); and releases of one
    small record under a full window (kept > 64 x freed; "small" makes the window start with one: the
    record that crosses a window's end is mostly a long one).  Pure model: no stream involved."""
    total = C.a.size
    kinds = [("hdr", j) for j in range(1, 16)] + [("hdr", 16), ("mid", 0), ("bigtail", 0), ("end", 0), ("small", 16),
                                                  ("one", 0), ("bigtail", 0), ("small", 7), ("one", 0)]
    sched, w, i, pos, t = [], 24, 0, 0, 0  # w: the window's first record header (capture offset); i: its record
    while True:
        limit = w - 24 + max_bytes
        if limit >= total:
            break
        kind, j = kinds[t % len(kinds)]
        t += 1
        n_rel, cut = None, None
        if kind == "bigtail":
            for r in range(i + 1, min(i + 80, C.n)):
                kept = 16 + int(C.lens[r]) - 1
                if C.lens[r] >= 20000 and C.hdr[r] - w < kept and pos <= C.end[r] - 1 <= limit:
                    cut = int(C.end[r]) - 1
                    break
        if cut is None:
            # the furthest record r > i whose cut still fits the window
            def at(r):
                if kind in ("hdr", "small"):
                    return int(C.hdr[r]) + j
                if kind == "end":
                    return int(C.hdr[r])
                return int(C.hdr[r]) + 16 + int(C.lens[r]) // 2
            r = int(np.searchsorted(C.hdr, limit, side="right")) - 1
            while r > i and not (pos <= at(r) <= limit and (kind != "small" or C.lens[r] < 400)):
                r -= 1
            cut = at(r) if r > i else limit
            if kind == "one":
                n_rel = 1
        assert pos <= cut <= limit
        pos = cut
        whole = int(np.searchsorted(C.end, pos, side="right"))
        assert whole > i, "the schedule must free something at every poll"
        i = i + n_rel if n_rel else whole
        w = int(C.hdr[i]) if i < C.n else total
        sched.append((pos, n_rel))
    return sched


@pytest.mark.parametrize("scan64", [False, True])
def test_awkward_cuts(scan64):
    """Records of 1 B to 70 KB (fake record chains, zero payloads) through a 160 KiB window, polled where
    the cut hurts: see _awkward_schedule.  The tails and move paths the schedule must produce are
    asserted from the model; the windows against the whole capture's reference as everywhere."""
    C = _awkward()
    max_bytes = 160 * KiB
    sched = _awkward_schedule(C, max_bytes)
    R = _Ring(C, max_bytes, 2048, step_bytes=4096, scan64=scan64)
    tails = set()
    try:
        for pos, n_rel in sched:
            while R.pos < pos:
                R.push(min(pos - R.pos, 50_000, R.room()))
            whole = R.whole()
            tails.add(pos - int(C.hdr[whole]) if whole < C.n else 0)
            R.poll()
            R.release(n_rel)
        while R.pos < R.total:
            R.push(min(R.total - R.pos, 50_000, R.room()))
        R.finish()
        assert set(range(0, 17)) <= tails, sorted(tails)[:20]       # every header split, a bare header, a clean cut
        paths = {p[0] for p in R.paths}
        assert {"disjoint", "chunks", "temp", "none"} <= paths, paths
        assert any(p[0] == "chunks" and p[1] > p[2] for p in R.paths)   # overlapping: kept > freed
        assert any(p[0] == "temp" and p[1] > 64 * p[2] for p in R.paths)
    finally:
        R.close()


def test_tails_and_errors_after_releases():
    """After releases: a trailing partial record header is ignored at finish; a last record running past
    the end is an error at finish and not at the poll before it; release(c + 1), a release after finish
    and a push larger than room() are refused and the stream works on."""
    C = _c4()
    cut = int(C.end[5999])            # 6 000 records of the capture ...
    rng = np.random.default_rng(11)
    # ... then 11 bytes of a next header: ignored
    R = _Ring(C, 128 * KiB, 2048, step_bytes=4096, total=cut + 11)
    try:
        sizes = _push_sizes(rng)
        k = 0
        refused = 0
        while R.pos < R.total:
            want = min(int(sizes[k % len(sizes)]), R.total - R.pos)
            if R.room() < want:
                c, m = R.poll()
                with pytest.raises(RuntimeError):
                    R.st.release(m + 1)
                with pytest.raises(RuntimeError):
                    R.st.push(C.a[:R.room() + 1])
                refused += 1
                assert R.st.released() == (R.rel_rec, R.rel_bytes)
                R.room()
                R.release()
            R.push(min(want, R.room()))
            k += 1
        assert refused >= 5
        c = R.finish(want_total=6000)
        with pytest.raises(RuntimeError):
            R.st.release(0)
        with pytest.raises(RuntimeError):
            R.st.release(c)
        assert R.st.released() == (R.rel_rec, R.rel_bytes)
    finally:
        R.close()
    # the last record 3 bytes short
    R = _Ring(C, 128 * KiB, 2048, step_bytes=0, total=cut - 3)
    try:
        while R.pos < R.total:
            if R.room() < 30_000:
                R.poll()
                R.release()
            R.push(min(30_000, R.total - R.pos, R.room()))
        assert R.rel_rec > 0
        c, m = R.poll()
        assert R.rel_rec + c == 5999
        with pytest.raises(RuntimeError, match="past the end"):
            R.st.finish()
    finally:
        R.close()


def test_filter_a_live_capture_on_the_device():
    """End to end: at every poll the window's batch() and its hdr_mask column (the TCP bit) go through
    Parser.pcap_write on the device, the result minus its global header is appended on the host, and
    everything is released.  The concatenation is the host-built capture of the whole input's TCP
    packets; one window's slab[offsets[i] : offsets[i] + lens[i]] are the input's bytes."""
    import torch
    import pktgpu
    C = _c4()
    tcp = 1 << schema.HDR_ID["TCP"]
    sel_ref = (C.ref["hdr_mask"] & np.uint32(tcp)) != 0
    want, n_want, *_ = pktgpu.pcap_write(C.a, offsets=C.offs, lens=C.lens, select=sel_ref, ts=(0, 0))
    assert 0 < n_want < C.n
    P = pktgpu.Parser(0)
    R = _Ring(C, 256 * KiB, 4096, step_bytes=0, columns=["chain"])
    out = bytearray(want[:24].tobytes())
    rng = np.random.default_rng(3)
    sizes = _push_sizes(rng)
    bytes_checked = False

    def consume(m):
        nonlocal bytes_checked
        slab, offs, lens = R.st.batch()
        assert R.st.aliased, "this torch build copies a __cuda_array_interface__ holder instead of aliasing it"
        assert offs.numel() == m and lens.numel() == m and slab.numel() <= R.max_bytes
        if not bytes_checked and R.rel_rec > 0 and m > 100:
            h, o, l = slab.cpu().numpy(), offs.cpu().numpy().astype(np.int64), lens.cpu().numpy().astype(np.int64)
            assert np.array_equal(o, C.offs[R.rel_rec:R.rel_rec + m].astype(np.int64) - R.rel_bytes)
            for i in range(m):
                g0 = int(o[i]) + R.rel_bytes
                assert np.array_equal(h[o[i]:o[i] + l[i]], C.a[g0:g0 + l[i]]), i
            bytes_checked = True
        if m:
            select = (R.st.out["hdr_mask"][:m].view(torch.int32) & tcp) != 0
            capture, k, *_ = P.pcap_write(slab, offsets=offs, lens=lens, select=select, ts=(0, 0), index=False)
            assert k == int(sel_ref[R.rel_rec:R.rel_rec + m].sum())
            out.extend(capture[24:].cpu().numpy().tobytes())

    try:
        k = 0
        while R.pos < R.total:
            w = min(int(sizes[k % len(sizes)]), R.total - R.pos)
            if R.room() < w:
                c, m = R.poll()
                consume(m)
                R.release()
            R.push(min(w, R.room()))
            k += 1
        c = R.finish()
        consume(c)
        assert bytes_checked
        assert bytes(out) == want.tobytes()
    finally:
        R.close()
        P.close()
