#!/usr/bin/env python3
"""pkt_lpm_lookup_batch at 2^20 C2 packets (64-byte slots), destination lookup, one JSON line per measurement (HIP
events over back-to-back launches on one stream after warm-up launches; the min of 3 rounds, as
scripts/dispatch_bench.py):

  lpm_v4_<routes>_<outputs>   routes = 1 (a /0), 2^10, 2^16 or about 2^20 synthetic IPv4 routes; outputs = route +
                              nexthop + plen + status, or nexthop alone.  Route lengths are drawn from V4_DIST (most
                              of a real table is /24), addresses uniformly, seed SEED; duplicates are dropped, so the
                              2^20 line holds a little under 2^20.
  lpm_v6_65536_<outputs>      2^16 IPv6 routes under 2000::/4, lengths from V6_DIST (none past /64, so that the torch
                              path below can work on the address's upper half), Ether / IPv6 / UDP in 64-byte slots.

Destination addresses: INSIDE of the packets lie in a random route with random host bits, the rest are uniform; the
hit share (status == OK, after the check below) must come out at 0.9 or more.  Per line: pkt_lpm_info's bytes and
depths and the create time (validate + compile on the host + upload, blocking).  Beside each line, from the same
process and run:
  (i)  a streaming copy of the call's own bytes (pkt_probe_stream_copy): per packet 13 chain bytes and the two
       aligned 16-byte slab chunks that hold the address read, the outputs written.  The table's entries are
       gathered on top of that and are not part of the copy.
  (ii) what a user can do without this call: pkt_extract_fields of the address, then one torch.searchsorted per
       distinct prefix length over per-length sorted prefix tensors, the lengths ascending so that the longest hit
       stays.  Its `route` is checked equal to the kernel's before it is timed.

  python scripts/lpm_bench.py [--n 1048576] [--iters 20] > profiles/lpm/lpm_bench.jsonl
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "packet-rs_amd"), os.path.join(REPO, "scripts"), REPO]
import pktgpu  # noqa: E402
from pktgpu import gen, pktgen, schema  # noqa: E402
from secondary_bench import copy_ceiling, event_ms  # noqa: E402

SEED = 20263
INSIDE = 0.95
V4_DIST = {8: 0.001, 12: 0.004, 16: 0.045, 20: 0.10, 22: 0.15, 24: 0.60, 28: 0.05, 32: 0.05}
V6_DIST = {32: 0.20, 40: 0.05, 48: 0.50, 56: 0.10, 64: 0.15}


def out(d):
    print(json.dumps(d), flush=True)


def min_ms(launch, it, rounds=3, warm=3):
    return min(event_ms(launch, it, warm=warm) for _ in range(rounds))


def rand_addr(rng, n, v6):
    """Uniform addresses as their upper 32 (IPv4) / 64 (IPv6, under 2000::/4) bits."""
    if not v6:
        return rng.integers(0, 1 << 32, n, dtype=np.uint64)
    return rng.integers(0, 1 << 60, n, dtype=np.uint64) | np.uint64(2 << 60)


def synth_routes(rng, count, dist, v6):
    """(plen uint8 [k], prefix uint64 [k]: the address's upper 32 (IPv4) / 64 (IPv6) bits, host bits zero), k <=
    count distinct routes."""
    if count == 1:
        return np.zeros(1, np.uint8), np.zeros(1, np.uint64)
    width = np.uint64(64 if v6 else 32)
    lens = np.array(sorted(dist))
    plen = rng.choice(lens, size=count, p=np.array([dist[int(k)] for k in lens]) / sum(dist.values())).astype(np.uint64)
    addr = rand_addr(rng, count, v6) >> (width - plen) << (width - plen)
    if v6:
        _, first = np.unique(np.stack([plen, addr], 1), axis=0, return_index=True)
    else:
        _, first = np.unique(plen << np.uint64(32) | addr, return_index=True)
    first.sort()
    return plen[first].astype(np.uint8), addr[first]


def route_array(plen, prefix, v6):
    arr = np.zeros(plen.size, schema.LPM_ROUTE_DTYPE)
    be = prefix.astype(">u8").view(np.uint8).reshape(-1, 8)
    if v6:
        arr["addr"][:, :8] = be
    else:
        arr["addr"][:, :4] = be[:, 4:]
    arr["ipver"], arr["plen"] = (6 if v6 else 4), plen
    arr["nexthop"] = np.arange(plen.size, dtype=np.uint32) % 64
    return arr


def draw_dst(rng, n, plen, prefix, v6):
    """n destination addresses (their upper 32 / 64 bits): INSIDE of them in a random route, random host bits."""
    width = np.uint64(64 if v6 else 32)
    uni = rand_addr(rng, n, v6)
    pick = rng.integers(0, plen.size, n)
    host = uni & ((np.uint64(1) << (width - plen[pick].astype(np.uint64))) - np.uint64(1))
    return np.where(rng.random(n) < INSIDE, prefix[pick] | host, uni)


def v6_slab(dst_hi, rng):
    """Ether / IPv6 / UDP packets in 64-byte slots with the given upper destination halves, random lower halves."""
    tpl = bytes(gen.create_udpv6_packet("00:01:02:03:04:05", "00:06:07:08:09:0a", False, 10, 3, 5, 6, 64, "2001:db8::1",
                                        "2001:db8::2", 1234, 9090, False, b"").to_vec())
    assert len(tpl) == 62
    n = dst_hi.size
    slab = np.zeros((n, 64), np.uint8)
    slab[:, :62] = np.frombuffer(tpl, np.uint8)
    slab[:, 38:46] = dst_hi.astype(">u8").view(np.uint8).reshape(-1, 8)
    slab[:, 46:54] = rng.integers(0, 256, (n, 8), dtype=np.uint8)
    return slab.reshape(-1)


class TorchLpm:
    """(ii): per distinct length the sorted prefixes (as the address's upper bits shifted down) and their route
    indices; a lookup is one searchsorted per length, ascending, the last hit staying."""

    def __init__(self, plen, prefix, v6, dev):
        self.width = 64 if v6 else 32
        self.tabs = []
        for L in np.unique(plen):
            sel = np.flatnonzero(plen == L)
            key = (prefix[sel] >> np.uint64(self.width - int(L))) if L else np.zeros(sel.size, np.uint64)
            order = np.argsort(key, kind="stable")
            self.tabs.append((int(L), torch.from_numpy(key[order].astype(np.int64)).to(dev),
                              torch.from_numpy(sel[order].astype(np.int64)).to(dev)))

    def lookup(self, addr):  # int64 [n]: the upper bits (non-negative: IPv4, or IPv6 under 2000::/4)
        route = torch.full_like(addr, -1)
        for L, keys, idx in self.tabs:
            k = addr >> (self.width - L) if L else torch.zeros_like(addr)
            at = torch.searchsorted(keys, k).clamp_(max=keys.numel() - 1)
            route = torch.where(keys[at] == k, idx[at], route)
        return route


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    n, it = a.n, a.iters
    dev = torch.device("cuda", 0)
    P = pktgpu.Parser(0)
    out({"box": torch.cuda.get_device_name(0), "packets": n, "iters": it, "seed": SEED, "inside_share_drawn": INSIDE,
         "v4_length_dist": V4_DIST, "v6_length_dist": V6_DIST,
         "measured": "HIP events around back-to-back launches on one stream, after 3 warm-up launches; min of 3 rounds"})
    rng = np.random.default_rng(SEED)
    s = P._stream(None)
    lines = [("v4", 1), ("v4", 1 << 10), ("v4", 1 << 16), ("v4", 1 << 20), ("v6", 1 << 16)]
    for ver, count in lines:
        v6 = ver == "v6"
        plen, prefix = synth_routes(rng, count, V6_DIST if v6 else V4_DIST, v6)
        arr = route_array(plen, prefix, v6)
        t0 = time.perf_counter()
        lpm = P.lpm(arr, default_nexthop=0xFFFF)
        create_ms = (time.perf_counter() - t0) * 1e3
        info = lpm.info()
        dst = draw_dst(rng, n, plen, prefix, v6)
        if v6:
            slab = torch.from_numpy(v6_slab(dst, rng)).to(dev)
            spec = [("IPv6", 0, 192, 255)]
        else:
            slab = pktgen.gen_udp(P, n, {"ipv4_dst": torch.from_numpy(dst.astype(np.int64)).to(dev).view(torch.uint64)})
            spec = [("IPv4", 0, 128, 159)]
        chain = P.parse(slab, stride=64, columns=["chain"])
        cols = {c: chain[c] for c in ("n_hdrs", "hdr_type", "hdr_off")}
        batch = dict(slab=slab, stride=64, n=n)
        full = lpm.lookup(batch, cols)
        tl = TorchLpm(plen, prefix, v6, dev)

        def torch_way(k):
            vals, found = P.extract_fields(slab, cols, spec, stride=64)
            return tl.lookup(vals[0].view(torch.int64))
        troute = torch_way(0)
        torch.cuda.synchronize()
        kroute = full["route"].view(torch.int32).to(torch.int64)  # PKT_LPM_NONE reads as -1
        same = bool(torch.equal(troute, kroute))
        hit = float((full["status"] == 0).float().mean())
        assert same, "the torch path and the kernel disagree"
        assert hit >= 0.9, hit
        tms = min_ms(torch_way, max(2, it // 4), rounds=3, warm=1)
        b = P._batch(slab, n, 64, None, None)
        ch = P._chain(cols)
        ptr = lambda k: full[k].data_ptr()  # noqa: E731
        for mode, args, wb in (("all_outputs", (ptr("route"), ptr("nexthop"), ptr("plen"), ptr("status")), 10),
                               ("nexthop_alone", (None, ptr("nexthop"), None, None), 4)):
            def launch(k):
                assert P._L.pkt_lpm_lookup_batch(lpm._t, ctypes.byref(b), ctypes.byref(ch), 0, 0, *args, s) == 0
            ms = min_ms(launch, it)
            ln = {"workload": f"lpm_{ver}_{count}_{mode}", "routes": int(plen.size), "table_bytes": info["bytes"],
                  "nodes": info["nodes_v6" if v6 else "nodes_v4"], "depth": info["depth_v6" if v6 else "depth_v4"],
                  "create_ms": round(create_ms, 2), "hit_share": round(hit, 4),
                  "kernel_us": round(ms * 1e3, 2), "Gpkt/s": round(n / (ms * 1e-3) / 1e9, 3),
                  "bytes_per_pkt": {"chain_read": 13, "slab_chunks_read": 32, "written": wb},
                  "torch_extract_searchsorted_us": round(tms * 1e3, 2), "torch_lengths": len(tl.tabs),
                  "lpm_frac_of_torch": round(ms / tms, 4), "route_equal_torch": same}
            c = copy_ceiling(n, 45, wb, dev, it, ms)
            if c is not None:
                ln["stream_copy"] = c
            out(ln)
        lpm.close()
        del slab, chain, cols, full, tl
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
