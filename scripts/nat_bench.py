#!/usr/bin/env python3
"""pkt_nat_batch at 2^20 C2 packets (Ether / IPv4 / UDP in 64-byte slots), one JSON line per measurement.  A call
rewrites its batch, so every launch is timed on its own (a HIP event pair around the one call; the slab is put back
from a pristine copy, and for the creating cases the table cleared, between the pairs, outside the timed windows); a
line reports the mean of its launches, the min of 3 rounds.

  nat_out_hit            all OUT, every packet hits one of 2^16 established sessions
  nat_in_hit             all IN, every packet hits one of them
  nat_out_hit_no_write   / nat_in_hit_no_write: PKT_NAT_NO_WRITE: what the stores cost is the difference
  nat_new_65536          2^16 new flows in one call, from a cleared table (16 packets a flow)
  nat_new_all            every packet a flow of its own (17 pool addresses), from a cleared table
  nat_mix_50_50          OUT and IN hits alternating, `dir` given
  nat_expire_half        pkt_nat_expire of half of 2^20 sessions (blocking; host clock around the call)

Beside each pkt_nat_batch line, from the same process and run:
  (i)   a streaming copy of the call's own bytes (pkt_probe_stream_copy): per packet, read twice (the claim and the
        translate kernel each classify) 13 chain bytes and the 28 header bytes, the 4-byte scratch word written and
        read; written 6 output bytes and the 10 rewritten packet bytes.  The forward table's and the reverse map's
        entries are gathered on top of that and are not part of the copy.
  (ii)  Forwarder.run on the same batch (one adjacency), the neighbouring per-packet rewrite.
  (iii) for the hit cases, what a user had before: flow_keys + torch.searchsorted and gathers on a prepared mapping +
        pkt_set_fields_csum + l4_checksum(update=True).  Its addresses and ports are checked equal to the kernel's
        before it is timed.
One creating call's per-kernel times come from a kernel trace of this script with --trace-case (one warm call, one
traced call, nothing else), not from this script's own clocks.

  python scripts/nat_bench.py [--n 1048576] [--iters 10] > profiles/nat/nat_bench.jsonl
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "packet-rs_amd"), os.path.join(REPO, "scripts"), REPO]
import pktgpu  # noqa: E402
from pktgpu import pktgen, schema  # noqa: E402
from secondary_bench import copy_ceiling  # noqa: E402

INSIDE, REMOTE = 0x0A000000, 0xC6336407
POOL = ["192.0.2.%d" % (k + 1) for k in range(17)]
PORTS = (1024, 65535)
NPORTS = PORTS[1] - PORTS[0] + 1
SET_OUT = [("IPv4", 0, 96, 127), ("UDP", 0, 0, 15)]    # IPv4.src, UDP.src
SET_IN = [("IPv4", 0, 128, 159), ("UDP", 0, 16, 31)]   # IPv4.dst, UDP.dst


def out(d):
    print(json.dumps(d), flush=True)


def u64(t):
    return t.to(torch.int64).view(torch.uint64)


def each_ms(fn, iters, between):
    """The mean of `iters` launches, each between its own event pair; between() runs before each, untimed."""
    s = torch.cuda.current_stream()
    between()
    fn()
    total = 0.0
    for _ in range(iters):
        between()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        fn()
        b.record(s)
        torch.cuda.synchronize()
        total += a.elapsed_time(b)
    return total / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--trace-case", default=None, help="run only this case: one warm call and one more, for a kernel trace")
    a = ap.parse_args()
    n, it = a.n, a.iters
    dev = torch.device("cuda", 0)
    P = pktgpu.Parser(0)
    if not a.trace_case:
        out({"box": torch.cuda.get_device_name(0), "packets": n, "iters": it,
             "measured": "a HIP event pair around every single call; slab restored (and, creating cases, table cleared) "
                         "between the pairs; mean of the launches, min of 3 rounds"})
    idx = torch.arange(n, device=dev, dtype=torch.int64)
    nat = P.nat(POOL, PORTS, slots=1 << 22)
    pool = torch.tensor([int.from_bytes(bytes(int(x) for x in p.split(".")), "big") for p in POOL], dtype=torch.int64, device=dev)

    def outbound(flow):  # flow f: inside host 10.x.y.z, port 1024 + f % 60000
        return pktgen.gen_udp(P, n, {"ipv4_src": u64(INSIDE + 1 + flow // 60000), "udp_src": u64(1024 + flow % 60000),
                                     "ipv4_dst": u64(torch.full_like(flow, REMOTE)), "udp_dst": u64(torch.full_like(flow, 53))})

    def inbound(flow):  # to the outside endpoint of entry `flow` (the flows of a cleared table take entries 0, 1, 2, ...)
        return pktgen.gen_udp(P, n, {"ipv4_dst": u64(pool[flow // NPORTS]), "udp_dst": u64(PORTS[0] + flow % NPORTS),
                                     "ipv4_src": u64(torch.full_like(flow, REMOTE)), "udp_src": u64(torch.full_like(flow, 53))})

    F = 1 << 16
    hit_flow = idx % F
    fwd = P.forwarder([("02:00:00:00:00:01", "02:00:00:00:00:fe", 0)])
    zeros32 = torch.zeros(n, dtype=torch.uint32, device=dev)
    half = (idx & 1).to(torch.uint8)
    cases = [("nat_out_hit", "out", hit_flow, True, False), ("nat_in_hit", "in", hit_flow, True, False),
             ("nat_out_hit_no_write", "out", hit_flow, False, False), ("nat_in_hit_no_write", "in", hit_flow, False, False),
             ("nat_new_65536", "out", hit_flow, True, True), ("nat_new_all", "out", idx, True, True),
             ("nat_mix_50_50", "mix", hit_flow, True, False)]
    for name, kind, flow, write, creating in cases:
        if a.trace_case and a.trace_case != name:
            continue
        if kind == "mix":
            po, pi = outbound(flow), inbound(flow)
            pristine = torch.where((half == 1).repeat_interleave(64), pi, po)
            dirs = half
            del po, pi
        else:
            pristine = outbound(flow) if kind == "out" else inbound(flow)
            dirs = schema.NAT_OUT if kind == "out" else schema.NAT_IN
        slab = pristine.clone()
        chain = P.parse(slab, stride=64, columns=["chain"])
        cols = {c: chain[c] for c in ("n_hdrs", "hdr_type", "hdr_off")}
        batch = dict(slab=slab, stride=64, n=n)

        def establish():  # the 2^16 sessions of the hit cases: entries 0 .. F - 1 in flow order
            nat.clear()
            est = outbound(torch.arange(n, device=dev, dtype=torch.int64) % F)
            r = nat.run(dict(slab=est, stride=64, n=n), cols, dir=schema.NAT_OUT, now=1, write=False, outputs=("status",))
            assert bool((r.status == 0).all())
        if not creating:
            establish()

        def call():
            return nat.run(batch, cols, dir=dirs, now=2, write=write)

        def restore():
            slab.copy_(pristine)
            if creating:
                nat.clear()
        if a.trace_case:
            restore()
            call()
            restore()
            call()
            torch.cuda.synchronize()
            return
        restore()
        r = call()
        torch.cuda.synchronize()
        ok_share = float((r.status == 0).float().mean())
        assert ok_share == 1.0, (name, ok_share, torch.bincount(r.status.to(torch.int64), minlength=12).tolist())
        ms = min(each_ms(call, it, restore) for _ in range(3))
        fms = min(each_ms(lambda: fwd.run(batch, cols, nexthop=zeros32), it, lambda: slab.copy_(pristine)) for _ in range(3))
        rd, wr = 2 * (13 + 28) + 4, 6 + 4 + (10 if write else 0)
        ln = {"workload": name, "sessions_before": 0 if creating else F, "created": int(r.created.sum()), "ok_share": ok_share,
              "call_us": round(ms * 1e3, 2), "Gpkt/s": round(n / (ms * 1e-3) / 1e9, 3), "bytes_per_pkt": {"read": rd, "written": wr},
              "forwarder_run_us": round(fms * 1e3, 2), "nat_frac_of_forwarder": round(ms / fms, 3)}
        if not creating and kind in ("out", "in") and write:
            # (iii) the path a user had: the prepared mapping is the sorted hashes of the established flows' packets
            specs = SET_OUT if kind == "out" else SET_IN
            slab.copy_(pristine)
            h = P.flow_keys(slab, cols, stride=64)["hash"].view(torch.int64)[:F]
            order = torch.argsort(h)
            sorted_h = h[order]
            e = torch.arange(F, device=dev, dtype=torch.int64)
            if kind == "out":
                new_addr, new_port = pool[e // NPORTS], PORTS[0] + e % NPORTS
            else:
                new_addr, new_port = INSIDE + 1 + e // 60000, 1024 + e % 60000

            def before():
                hh = P.flow_keys(slab, cols, stride=64)["hash"].view(torch.int64)
                f = order[torch.searchsorted(sorted_h, hh).clamp(max=F - 1)]
                P.set_fields(slab, cols, specs, [u64(new_addr[f]), u64(new_port[f])], stride=64, ipv4_checksum=0)
                P.l4_checksum(slab, cols, update=True, keep_zero_udp=True, stride=64)
            slab.copy_(pristine)
            call()
            mine = slab.clone()
            slab.copy_(pristine)
            before()
            torch.cuda.synchronize()
            same = bool(torch.equal(mine, slab))  # valid checksums before: updating and recomputing agree
            bms = min(each_ms(before, max(2, it // 2), lambda: slab.copy_(pristine)) for _ in range(3))
            ln.update({"before_keys_search_gather_set_csum_us": round(bms * 1e3, 2), "nat_frac_of_before": round(ms / bms, 4),
                       "slab_equal_before": same})
        c = copy_ceiling(n, rd, wr, dev, it, ms)
        if c is not None:
            ln["stream_copy"] = c
        out(ln)
        del slab, pristine, chain, cols
        torch.cuda.empty_cache()
    if a.trace_case:
        return
    # expire: 2^20 sessions, the even flows last seen at 0, the odd ones at 100; idle 50 at now 100 removes the even ones
    best = None
    for _ in range(3):
        nat.clear()
        slab = outbound(idx)
        chain = P.parse(slab, stride=64, columns=["chain"])
        cols = {c: chain[c] for c in ("n_hdrs", "hdr_type", "hdr_off")}
        nat.run(dict(slab=slab, stride=64, n=n), cols, now=0, write=False, outputs=())
        nat.run(dict(slab=slab, stride=64, n=n), cols, now=100, write=False, outputs=(), select=half)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        gone = nat.expire(100, (0, 50, 0))
        dt = time.perf_counter() - t0
        assert gone == n // 2 and nat.count() == (0, n - n // 2, 0), (gone, nat.count())
        best = dt if best is None else min(best, dt)
    out({"workload": "nat_expire_half", "sessions": n, "expired": n // 2, "pool_entries_per_protocol": len(POOL) * NPORTS,
         "slots": 1 << 22, "call_ms_host_clock": round(best * 1e3, 3)})
    nat.close()


if __name__ == "__main__":
    main()
