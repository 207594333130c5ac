#!/usr/bin/env python3
"""pkt_meter_batch at 2^20 C2 packets (Ether / IPv4 / UDP in 64-byte slots), one JSON line per measurement.  A call
moves the meters' state on, so every launch is timed on its own (a HIP event pair around the one call; between the
pairs, outside the timed windows, the times move on by one batch so that every call sees the same traffic against the
same contract); a line reports the mean of its launches, the min of 3 rounds.

  meter_one_conforming     one meter, every packet green (rate and bursts far above the traffic)
  meter_one_overload_2x    one meter, twice the committed rate: green and red interleave
  meter_256                256 meters, uniformly
  meter_65536              2^16 meters, uniformly
  meter_distinct           2^20 meters, one packet each
  meter_256_now            256 meters, one `now` for the batch instead of per-packet times
  meter_256_mark           256 meters, every colour's action REMARK, PKT_METER_MARK

Beside each line, from the same process and run:
  (i)   a streaming copy of the call's own bytes (pkt_probe_stream_copy): per packet, the meter id read by the count
        and the place kernel of the first radix pass, 8 bytes of (meter, index) written and read per pass and read by
        the walk, the time, the colour byte written and read, 3 output bytes (and under MARK the 13 chain bytes, the
        IPv4 header's 12 bytes read and 3 written).  The gathers by index are part of the call and not of the copy.
  (ii)  the host twin (Meters(None, ...)) on one thread over the same arrays: what a user had before, after copying
        ids, times and lengths to the host (the copies are not counted).
The colours of the first call are checked equal to the host twin's before anything is timed.
One call's per-kernel times come from a kernel trace of this script with --trace-case (one warm call, one traced call,
nothing else), not from this script's own clocks.

  python scripts/meter_bench.py [--n 1048576] [--iters 10] > profiles/meter/meter_bench.jsonl
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
from pktgpu import pktgen  # noqa: E402
from secondary_bench import copy_ceiling  # noqa: E402

GAP = 50  # ns between packets: 64-byte packets (84 on the wire with adjust = 20) at 1.68 GB/s


def out(d):
    print(json.dumps(d), flush=True)


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
    ap.add_argument("--only", default=None, help="comma-separated case names")
    a = ap.parse_args()
    n, it = a.n, a.iters
    dev = torch.device("cuda", 0)
    P = pktgpu.Parser(0)
    if not a.trace_case:
        out({"box": torch.cuda.get_device_name(0), "packets": n, "iters": it, "lib": os.environ.get("PKTGPU_LIB", "libpktgpu.so"),
             "measured": "a HIP event pair around every single call; the times moved on by one batch between the pairs; "
                         "mean of the launches, min of 3 rounds"})
    idx = torch.arange(n, device=dev, dtype=torch.int64)
    slab = pktgen.gen_udp(P, n, {"udp_src": (1024 + idx % 60000).view(torch.uint64)})
    chain = P.parse(slab, stride=64, columns=["chain"])
    cols = {c: chain[c] for c in ("n_hdrs", "hdr_type", "hdr_off")}
    batch = dict(slab=slab, stride=64, n=n)
    span = n * GAP
    wire = 84  # bytes a packet costs with adjust = 20
    rate = wire * 10 ** 9 // GAP  # the traffic's bytes per second, all of it
    remark = (pktgpu.METER_REMARK,) * 3

    def contract(share, nm, action=(0, 0, 1)):  # a meter's cir = share of its own traffic
        per = rate // nm
        return dict(cir=int(per * share), cbs=3000, xbs=3000, action=action, dscp=(10, 12, 14))

    cases = [("meter_one_conforming", 1, [dict(cir=1 << 40, cbs=1 << 26, xbs=1 << 26)], "time", False),
             ("meter_one_overload_2x", 1, [dict(cir=rate // 2, cbs=wire, xbs=0)], "time", False),
             ("meter_256", 256, [contract(0.75, 256)], "time", False),
             ("meter_65536", 1 << 16, [contract(0.75, 1 << 16)], "time", False),
             ("meter_distinct", n, [contract(0.75, n)], "time", False),
             ("meter_256_now", 256, [contract(0.75, 256)], "now", False),
             ("meter_256_mark", 256, [contract(0.75, 256, remark)], "time", True)]
    only = a.only.split(",") if a.only else None
    for name, nm, cfg, clock, mark in cases:
        if (a.trace_case and a.trace_case != name) or (only and name not in only):
            continue
        cfgs = np.repeat(pktgpu.meter_cfgs(cfg), nm)
        m = P.meters(cfgs, adjust=20)
        ids = ((idx * 2654435761) % nm).to(torch.int32).view(torch.uint32) if 1 < nm < n else None
        if nm == n:
            ids = torch.randperm(n, device=dev).to(torch.int32).view(torch.uint32)
        t0 = (1000 + idx * GAP)
        tcur = t0.clone()
        calls = [0]

        def call():
            kw = dict(time=tcur.view(torch.uint64)) if clock == "time" else dict(now=1000 + calls[0] * span)
            return m.run(batch, cols if mark else None, meter=0 if ids is None else ids, mark=mark, **kw)

        def advance():
            calls[0] += 1
            tcur.copy_(t0 + calls[0] * span)
        if a.trace_case:
            call()
            advance()
            call()
            torch.cuda.synchronize()
            return
        r = call()
        torch.cuda.synchronize()
        # (ii) the host twin over the same arrays, from fresh state: the first call's colours agree
        hb = dict(slab=slab.cpu().numpy(), stride=64, n=n)
        hch = {c: v.cpu().numpy() for c, v in cols.items()} if mark else None
        hids = 0 if ids is None else ids.cpu().numpy()
        hm = pktgpu.Meters(None, cfgs, adjust=20)
        hkw = dict(time=t0.cpu().numpy().astype(np.uint64)) if clock == "time" else dict(now=1000)
        w0 = time.perf_counter()
        hr = hm.run(hb, hch, meter=hids, mark=mark, **hkw)
        host_ms = (time.perf_counter() - w0) * 1e3
        assert np.array_equal(hr.color, r.color.cpu().numpy()), name
        share = np.bincount(hr.color, minlength=4) / n
        ms = min(each_ms(call, it, advance) for _ in range(3))
        passes = 1 if nm <= 256 else 2 if nm <= 65536 else 3
        rd = 8 + 16 * (passes - 1) + 8 + (8 if clock == "time" else 0) + 5 + (25 if mark else 0)
        wr = 8 * passes + 1 + 3 + (3 if mark else 0)
        ln = {"workload": name, "meters": nm, "radix_passes": passes, "colour_share": [round(float(x), 4) for x in share],
              "call_us": round(ms * 1e3, 2), "Gpkt/s": round(n / (ms * 1e-3) / 1e9, 3), "bytes_per_pkt": {"read": rd, "written": wr},
              "host_twin_one_thread_ms": round(host_ms, 2), "host_over_device": round(host_ms / ms, 1)}
        c = copy_ceiling(n, rd, wr, dev, it, ms)
        if c is not None:
            ln["stream_copy"] = c
        out(ln)
        m.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
