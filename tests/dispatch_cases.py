"""The yardstick of pkt_dispatch_* and pkt_reorder_batch, shared by test_dispatch_host.py and
test_dispatch_device.py: the bucket rule, the stable partition and the reorder's layout written out with numpy
from include/pktgpu.h's text, never with the host twins or the device, and the case lists.  Each case asserts its
own premise.
"""
import numpy as np

import compare_cases as C
import l4_cases as L4
import match_cases as M
from pktgpu import schema

DROP = 0xFFFF
FILL = 0x77
MAXH = schema.MAX_HDRS


# ------------------------------------------------------------------ dispatch
def bprime(key, nb, table=None, select=None):
    """b' of every packet: its bucket, nb for a dropped one."""
    key = np.asarray(key, np.uint32).astype(np.int64)
    if table is None:
        b = np.where(key < nb, key, nb)
    else:
        t = np.asarray(table, np.int64)
        assert t.size >= 1 and t.size & (t.size - 1) == 0
        b = t[key & (t.size - 1)]
        b = np.where(b == DROP, nb, b)
    if select is not None:
        b = np.where(np.asarray(select) != 0, b, nb)
    return b


def expect_dispatch(key, nb, table=None, select=None):
    bp = bprime(key, nb, table, select)
    n = bp.size
    perm = np.argsort(bp, kind="stable").astype(np.uint32)
    rank = np.empty(n, np.uint32)
    rank[perm] = np.arange(n, dtype=np.uint32)
    cnt = np.bincount(bp, minlength=nb + 1)
    start = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64)
    assert start.size == nb + 2 and start[nb + 1] == n
    return dict(bucket=np.where(bp == nb, DROP, bp).astype(np.uint16), perm=perm, rank=rank, start=start)


def check_dispatch(got, want, label=""):
    for k, g in got.items():
        g, w = np.asarray(g), want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, (label, k, g.dtype, g.shape, w.shape)
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, (label, k, "first bad", bad[:8], g[bad[:8]], w[bad[:8]])


def dcase(name, key, nb, table=None, select=None, full=False, only=None):
    key = np.asarray(key, np.uint32)
    c = dict(name=name, key=key, nb=nb, table=None if table is None else np.asarray(table, np.uint16), select=select)
    cnt = np.bincount(bprime(key, nb, table, select), minlength=nb + 1)
    if full:  # every bucket and the drop tail are populated
        assert (cnt > 0).all(), name
    if only is not None:  # everything in one b'
        assert cnt[only] == key.size and key.size > 0, name
    return c


def dispatch_cases():
    rng = np.random.default_rng(20)
    out = []
    n = 1000
    for nb in (1, 2, 3, 64, 255, 256):
        key = rng.permutation(n) % (nb + 1)                      # the value nb drops (DIRECT: key >= nbuckets)
        out.append(dcase(f"direct_{nb}", key, nb, full=True))
        sel = (np.arange(n) % 5 != 0).astype(np.uint8)
        out.append(dcase(f"direct_{nb}_select", rng.permutation(n) % nb, nb, select=sel, full=nb <= 64))
        hi = key.astype(np.uint32) | (rng.integers(0, 2, n).astype(np.uint32) << 31)  # high bits: dropped, not wrapped
        out.append(dcase(f"direct_{nb}_high_bits", hi, nb))
    for tl in (1, 128, 4096):
        for nb in (1, 3, 256):
            tab = rng.integers(0, nb, tl).astype(np.uint16)
            key = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
            out.append(dcase(f"table_{tl}_{nb}", key, nb, tab))
            if tl > 1:
                tab = tab.copy()
                tab[::3] = DROP
                out.append(dcase(f"table_{tl}_{nb}_drops", key, nb, tab, select=(np.arange(n) % 7 != 3).astype(np.uint8)))
    tab = np.arange(128, dtype=np.uint16) % 4
    tab[5::16] = DROP
    out.append(dcase("table_128_4_full", rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32), 4, tab, full=True))
    out.append(dcase("one_bucket", np.full(n, 2), 3, only=2))
    out.append(dcase("one_bucket_table", rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32), 64,
                     np.full(128, 63, np.uint16), only=63))
    out.append(dcase("all_dropped_direct", np.full(n, 3), 3, only=3))
    out.append(dcase("all_dropped_select", rng.permutation(n) % 3, 3, select=np.zeros(n, np.uint8), only=3))
    out.append(dcase("all_dropped_table", np.arange(n), 256, np.full(1, DROP, np.uint16), only=256))
    for k in (0, 1, 2):
        out.append(dcase(f"n_{k}", np.arange(k) + 1, 3))
        out.append(dcase(f"n_{k}_table", np.arange(k), 2, np.array([1, DROP], np.uint16), select=np.ones(k, np.uint8)))
    return out


def edge_keys(kind, n, nb):
    """The device tests' skews: uniform keys, one bucket only, all dropped, two buckets alternating."""
    rng = np.random.default_rng(n * 7 + nb)
    if kind == "uniform":
        return rng.integers(0, nb + 1, n).astype(np.uint32)
    if kind == "one":
        return np.full(n, nb - 1, np.uint32)
    if kind == "dropped":
        return np.full(n, nb, np.uint32)
    assert kind == "alternate"
    return np.where(np.arange(n) % 2 == 0, 0, nb - 1).astype(np.uint32)  # (nb == 1: one bucket)


OUTPUT_SETS = [tuple(k for j, k in enumerate(("bucket", "perm", "rank", "start")) if m >> j & 1) for m in range(16)]


# ------------------------------------------------------------------ reorder
def filled(shape, dtype):
    a = np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, FILL, np.uint8).view(dtype)
    return a.reshape(shape)


def expect_reorder(b, perm, cols=None, seg=None, nseg=0, slot=None, m=None):
    """The reorder of batch dict `b` by `perm` from the header's text -> dict(dst, out_len, cols, check): every
    array starts as the 0x77 fill and holds the expected values wherever the call writes; check[c] is False
    where a slot row may be left unwritten (rows at or past the source packet's n_hdrs when n_hdrs is given)."""
    cols = cols or {}
    perm = np.asarray(perm, np.uint32)
    m = perm.size if m is None else m
    n = b["n"] if b is not None else 0
    ext = C.extents(b) if b is not None and slot else None
    sg = None
    if nseg:
        sg = np.minimum(np.asarray(seg, np.uint64)[:nseg + 1], m).astype(np.int64)
        assert sg[0] == 0 and (np.diff(sg) >= 0).all()   # the caller's promise
    dst = filled(m * slot, np.uint8) if slot else None
    out_len = filled(m, np.uint32) if slot else None
    oc, check = {}, {}
    for c, a in cols.items():
        shp = schema.column_shape(c, m)
        slots = len(shp) == 2 and shp[0] == MAXH and c in ("hdr_type", "hdr_off")
        oc[c] = filled((MAXH * m,) if slots and nseg else shp, a.dtype)
        check[c] = np.ones(oc[c].shape, bool)
    for k in range(m):
        if nseg:
            s = int(np.searchsorted(sg[1:], k, side="right"))
            if s >= nseg:
                continue                                   # at or past seg_start[nseg]: not written at all
            s0, ns = int(sg[s]), int(sg[s + 1] - sg[s])
            assert s0 <= k < s0 + ns
        else:
            s0, ns = 0, m
        p = int(perm[k])
        empty = p >= n
        if slot:
            ln = 0
            if not empty:
                off, ln = ext[p]
                ln = min(ln, slot)
                dst[k * slot:k * slot + ln] = b["slab"][off:off + ln]
            dst[k * slot + ln:k * slot + (ln + 15) // 16 * 16] = 0
            out_len[k] = ln
        rows = MAXH
        if "n_hdrs" in cols and not empty:
            rows = min(int(cols["n_hdrs"][p]), MAXH)
        for c, a in cols.items():
            if c in ("hdr_type", "hdr_off"):
                for j in range(MAXH):
                    e = MAXH * s0 + j * ns + (k - s0)
                    ix = e if nseg else (j, k)
                    if j < rows:
                        oc[c][ix] = 0 if empty else a[j, p]
                    else:
                        check[c][ix] = False
            else:
                oc[c][k] = 0 if empty else a[p]
    return dict(dst=dst, out_len=out_len, cols=oc, check=check)


def check_reorder(got_dst, got_len, got_cols, want, label=""):
    if want["dst"] is not None:
        bad = np.flatnonzero(np.asarray(got_dst) != want["dst"])
        assert bad.size == 0, (label, "dst: first bad bytes", bad[:8])
        bad = np.flatnonzero(np.asarray(got_len) != want["out_len"])
        assert bad.size == 0, (label, "out_len", bad[:8], np.asarray(got_len)[bad[:8]], want["out_len"][bad[:8]])
    for c, w in want["cols"].items():
        g = np.asarray(got_cols[c]).reshape(w.shape)
        bad = np.argwhere((g != w) & want["check"][c])
        assert bad.size == 0, (label, c, "first bad elements", bad[:8])


_SRC = None


def sources():
    """{name: (batch dict, parse columns)}: ref22.pcap's packets and a random mix, at indexed random alignments
    and in a fixed-stride slab; the columns are the chain (Python parser model) and a few made-up field columns
    of every element size, ipv6_src's 16 bytes included."""
    global _SRC
    if _SRC is not None:
        return _SRC
    rng = np.random.default_rng(77)
    pk22 = C.packets(M.ref22_batch())
    mix = M.random_mix(rng, 90)
    out = {}
    for name, pkts in (("ref22", pk22), ("mix", mix)):
        b = C.indexed(pkts, rng)
        out[name] = (b, columns_of(b, rng))
    stride = 128
    slab = rng.integers(0, 256, stride * len(mix), dtype=np.uint8)
    lens = np.array([min(len(p), stride) for p in mix], np.uint32)
    for i, p in enumerate(mix):
        slab[i * stride:i * stride + lens[i]] = np.frombuffer(p[:stride], np.uint8)
    b = C.batch(slab, lens=lens, stride=stride)
    out["mix_stride"] = (b, columns_of(b, rng))
    _SRC = out
    return out


def columns_of(b, rng):
    n = b["n"]
    cols = dict(L4.chain_of(b))
    for c in ("status", "payload_off", "hdr_mask", "eth_dst", "ipv6_src", "udp_checksum"):
        dt = schema.column_dtype(c)
        shp = schema.column_shape(c, n)
        cols[c] = rng.integers(1, 255, int(np.prod(shp)) * dt.itemsize, dtype=np.uint8).view(dt).reshape(shp)
    return cols


def aligned(b, al):
    """Batch b's packets again, every one at offset `al` mod 16."""
    return C.indexed(C.packets(b), np.random.default_rng(al), align=[al] * b["n"], pad=3)


COLSETS = [(), ("n_hdrs", "hdr_type", "hdr_off"), ("hdr_type",), ("hdr_off", "ipv6_src"),
           ("status", "payload_off", "hdr_mask", "eth_dst", "ipv6_src", "udp_checksum", "n_hdrs", "hdr_type", "hdr_off")]


def reorder_cases():
    """[dict(name, src, perm, seg, nseg, slot, cols)]: the layouts the issue lists."""
    rng = np.random.default_rng(5)
    out = []
    for src, (b, cols) in sources().items():
        n = b["n"]
        longest = max(ln for _, ln in C.extents(b))
        up = (longest + 15) // 16 * 16
        perm = rng.permutation(n).astype(np.uint32)
        wild = perm.copy()
        wild[::4] = np.array([n, n + 1, 0xFFFFFFFF, 1 << 31], np.uint32)[np.arange(wild[::4].size) % 4]  # empty positions
        # a dispatch's start: 5 buckets of which 1 and 3 are empty, and a dropped tail
        cuts = np.sort(rng.integers(0, n, 3))
        seg5 = np.array([0, cuts[0], cuts[0], cuts[1], cuts[1], cuts[2], n], np.uint64)
        assert seg5[5] < n and len(set(seg5.tolist())) >= 4
        for slot in sorted({16, max(16, up - 16), up, up + 32}):  # below, at and above the longest packet
            out.append(dict(name=f"{src}_slot{slot}", src=src, perm=perm, seg=None, nseg=0, slot=slot, cols=COLSETS[1]))
        assert 16 < longest  # the smallest slot cuts
        out.append(dict(name=f"{src}_wild", src=src, perm=wild, seg=None, nseg=0, slot=up, cols=COLSETS[4]))
        out.append(dict(name=f"{src}_one_seg", src=src, perm=wild, seg=np.array([0, n], np.uint64), nseg=1, slot=up, cols=COLSETS[4]))
        out.append(dict(name=f"{src}_segs", src=src, perm=perm, seg=seg5, nseg=5, slot=up, cols=COLSETS[4]))
        out.append(dict(name=f"{src}_segs_past_m", src=src, perm=wild, seg=np.array([0, 3, n + 9, 1 << 40], np.uint64), nseg=3,
                        slot=32, cols=COLSETS[1]))
        for k, cs in enumerate(COLSETS):
            out.append(dict(name=f"{src}_cols{k}", src=src, perm=wild, seg=seg5, nseg=5, slot=None if k % 2 else 48, cols=cs))
        out.append(dict(name=f"{src}_repeats", src=src, perm=rng.integers(0, n, 2 * n + 3).astype(np.uint32), seg=None, nseg=0,
                        slot=up, cols=COLSETS[3]))
    return out
