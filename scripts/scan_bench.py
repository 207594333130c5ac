#!/usr/bin/env python3
"""pkt_scan_batch, one JSON line per measurement.  Launches go back to back on one stream between two HIP events,
after 3 warm-up launches, over a RING of slab copies larger than the 256 MB MALL, so that no launch finds its packets
in a cache; the figure is the median of 5 such rounds, the minimum beside it.

  workloads   c2_payload / c2_packet: 2^20 C2 packets (64-byte Ether / IPv4 / UDP, fixed stride), the PAYLOAD region
              from the parse's chain, and the whole PACKET; rand1500: 2^17 packets of 1500 random bytes in 1504-byte
              slots, PACKET
  sets        1, 64, 1024 and 8192 random patterns of 4..16 random bytes, as they are ("none": what occurs, occurs
              by chance) and with pattern 0 planted in 1 % of the packets ("planted")
  adversarial 2^17 packets of 1500 bytes 'a' against one pattern of 64 bytes 'a': every start walks 64 deep
  create      pkt_scan_create at the limits (8192 patterns of 16 bytes), wall clock
  with_hits   the same launch with the per-pattern counters

Beside each line, from the same process and run: (i) a streaming copy of the call's own bytes
(pkt_probe_stream_copy): per packet its region's bytes (whole packets for PACKET), the chain's 13 bytes for PAYLOAD,
and the 24 bytes of the seven outputs; (ii) for the 1-pattern lines, what a user could do before: the torch
expression of m shifted compares over the fixed-stride slab, reduced to one bool per packet.

  python scripts/scan_bench.py [--iters 10] > profiles/scan/scan_bench.jsonl
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "packet-rs_amd"), os.path.join(REPO, "scripts"), REPO]
import pktgpu  # noqa: E402
from pktgpu import gen, schema  # noqa: E402
from secondary_bench import copy_ceiling, event_ms  # noqa: E402

MALL = 256 << 20
OUT = (("status", torch.uint8), ("pat", torch.uint32), ("off", torch.uint16), ("action", torch.uint32), ("sel", torch.uint8),
       ("count", torch.uint32), ("matched", torch.uint64))


def out(d):
    print(json.dumps(d), flush=True)


def rounds(launch, it, k=5):
    ms = [event_ms(launch, it) for _ in range(k)]
    return statistics.median(ms), min(ms)


def random_set(rng, k):
    return [rng.integers(0, 256, int(rng.integers(4, 17)), dtype=np.uint8).tobytes() for _ in range(k)]


def plant(slab2d, pat, at, share, rng):
    """pattern bytes at column `at` of share of the rows (a copy)."""
    s = slab2d.clone()
    rows = torch.from_numpy(rng.choice(s.shape[0], int(s.shape[0] * share), replace=False)).to(s.device)
    s[rows, at:at + len(pat)] = torch.frombuffer(bytearray(pat), dtype=torch.uint8).to(s.device)
    return s


def torch_prior_art(slab2d, pat, lo, hi):
    """One bool per packet: pattern `pat` starts somewhere in columns [lo, hi - len] — m shifted compares."""
    w = hi - lo - len(pat) + 1

    def run(_):
        acc = slab2d[:, lo:lo + w] == pat[0]
        for k in range(1, len(pat)):
            acc &= slab2d[:, lo + k:lo + k + w] == pat[k]
        return acc.any(dim=1)
    return run


def measure(P, sc, ring, n, stride, lens, chain, region, it, hits=None):
    """(median ms, min ms, the last call's outputs) of pkt_scan_batch over the ring."""
    L = P._L
    dev = ring[0].device
    res = {k: torch.empty(n, dtype=dt, device=dev) for k, dt in OUT}
    bs = [P._batch(s.reshape(-1), n, stride, None, lens) for s in ring]
    ch = None if chain is None else P._chain(chain)
    s = P._stream(None)
    ptrs = [res[k].data_ptr() for k, _ in OUT]
    hp = None if hits is None else hits.data_ptr()

    def launch(k):
        assert L.pkt_scan_batch(sc._t, ctypes.byref(bs[k % len(bs)]), None if ch is None else ctypes.byref(ch), region, None,
                                *ptrs, hp, s) == 0
    med, mn = rounds(launch, it)
    return med, mn, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--n", type=int, default=1 << 20)
    a = ap.parse_args()
    it = a.iters
    dev = torch.device("cuda", 0)
    P = pktgpu.Parser(0)
    rng = np.random.default_rng(11)
    out({"box": torch.cuda.get_device_name(0), "iters": it,
         "measured": "HIP events around back-to-back launches on one stream over a ring of slab copies above 256 MB, "
                     "after 3 warm-up launches; median and min of 5 rounds"})
    n2, n15 = a.n, a.n // 8
    c2 = torch.from_numpy(gen.gen_c2(n2, seed=7)).to(dev).reshape(n2, 64)
    chain = P.parse(c2.reshape(-1), stride=64, columns=["chain"])
    chain = {k: chain[k] for k in ("n_hdrs", "hdr_type", "hdr_off")}
    r15 = torch.randint(0, 256, (n15, 1504), dtype=torch.uint8, device=dev)
    l15 = torch.full((n15,), 1500, dtype=torch.int32, device=dev).view(torch.uint32)
    torch.cuda.synchronize()
    works = (("c2_payload", c2, n2, 64, None, chain, schema.SCAN_PAYLOAD, 42, 64, 22 + 13),
             ("c2_packet", c2, n2, 64, None, None, schema.SCAN_PACKET, 0, 64, 64),
             ("rand1500", r15, n15, 1504, l15, None, schema.SCAN_PACKET, 0, 1500, 1500 + 4))
    sets = {k: random_set(rng, k) for k in (1, 64, 1024, 8192)}
    for name, slab, n, stride, lens, ch, region, lo, hi, read_b in works:
        copies = MALL // slab.numel() + 2
        for k, pats in sets.items():
            sc = P.scanner(pats)
            for planted in (False, True):
                base = plant(slab, pats[0], lo + 3, 0.01, rng) if planted else slab
                ring = [base] + [base.clone() for _ in range(copies - 1)]
                med, mn, res = measure(P, sc, ring, n, stride, lens, ch, region, it)
                hits = torch.zeros(k + 1, dtype=torch.uint64, device=dev)
                medh, _, _ = measure(P, sc, ring, n, stride, lens, ch, region, it, hits)
                torch.cuda.synchronize()
                ln = {"workload": name, "patterns": k, "occurrences": "planted 1%" if planted else "none", "packets": n,
                      "info": sc.info, "hit_share": round(float((res["status"] == 1).float().mean().item()), 5),
                      "call_us": round(med * 1e3, 1), "call_us_min": round(mn * 1e3, 1), "with_hits_us": round(medh * 1e3, 1),
                      "ns_per_packet": round(med * 1e6 / n, 3), "region_GB/s": round(n * (hi - lo) / (med * 1e-3) / 1e9, 1),
                      "ring_bytes": int(base.numel()) * copies}
                c = copy_ceiling(n, read_b, 24, dev, it, med)
                if c is not None:
                    ln["stream_copy"] = c
                if k == 1:
                    fn = torch_prior_art(base, pats[0], lo, hi)
                    same = bool(torch.equal(fn(0), res["status"] == 1))
                    tms, _ = rounds(fn, max(2, it // 4), k=3)
                    ln["torch_shifted_compares"] = {"pattern_bytes": len(pats[0]), "us": round(tms * 1e3, 1), "same_answer": same,
                                                    "over_fused": round(tms / med, 2)}
                out(ln)
                del ring, base
                torch.cuda.empty_cache()
            sc.close()
    # ---- the worst case: every start walks the whole pattern
    rows = torch.full((n15, 1504), ord("a"), dtype=torch.uint8, device=dev)
    ring = [rows, rows.clone()]
    for m in (8, 64):
        sc = P.scanner([b"a" * m])
        med, mn, res = measure(P, sc, ring, n15, 1504, l15, None, schema.SCAN_PACKET, max(2, it // 2))
        torch.cuda.synchronize()
        assert int(res["count"][0].item()) == 1500 - m + 1
        out({"workload": "adversarial_repeated_byte", "pattern_bytes": m, "packets": n15, "info": sc.info, "call_us": round(med * 1e3, 1),
             "call_us_min": round(mn * 1e3, 1), "ns_per_start": round(med * 1e6 / (n15 * 1500), 4),
             "ns_per_step": round(med * 1e6 / (n15 * 1500 * m), 5)})
        sc.close()
    del ring, rows
    # ---- create at the limits
    raw = rng.integers(0, 256, (schema.SCAN_MAX_PATTERNS, 16), dtype=np.uint8)
    tab = np.zeros(schema.SCAN_MAX_PATTERNS, schema.SCAN_PATTERN_DTYPE)
    tab["off"], tab["len"], tab["action"] = np.arange(schema.SCAN_MAX_PATTERNS) * 16, 16, 1
    ts = []
    for _ in range(5):
        t0 = time.perf_counter()
        sc = pktgpu.Scanner(P, (raw.reshape(-1), tab))
        ts.append(time.perf_counter() - t0)
        info = sc.info
        sc.close()
    out({"what": "pkt_scan_create at the limits", "patterns": schema.SCAN_MAX_PATTERNS, "bytes": schema.SCAN_MAX_BYTES, "info": info,
         "create_ms": round(statistics.median(ts) * 1e3, 2), "create_ms_min": round(min(ts) * 1e3, 2)})


if __name__ == "__main__":
    main()
