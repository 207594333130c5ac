#!/usr/bin/env python3
"""pkt_icmp_err_batch at 2^20 source packets, one JSON line per measurement.  Every call is timed by its own pair of
HIP events on the call's stream (the call waits for its totals, so calls cannot be queued back to back); the figure is
the minimum over `iters` calls after 2 warm-up calls, the median beside it.

  icmp_c2_all          C2 packets (64-byte Ether / IPv4 / UDP), every one answered with time exceeded: 92-byte outputs,
                       nothing clipped
  icmp_1500_all        1500-byte packets in 1504-byte slots, every one answered with too big: 590-byte outputs, every
                       quote clipped to 548 bytes
  icmp_1500_fwd_1pct   the same packets with a pkt_fwd_batch status array as the code (through ICMP_MAP_FWD) in which
                       1 packet in 100 is refused (TTL / MTU / NO_ADJ in turn): what a router's batch looks like
  *_no_write           the same calls with PKT_ICMPE_NO_WRITE (decision, scan, out_index): what the build kernel's
                       walk costs is the difference

Beside each line, from the same process and run, a streaming copy of the call's own bytes (pkt_probe_stream_copy):
read per source packet 13 chain bytes, the code, for an indexed batch offset and length, the 32 header bytes the
decision loads and, per output, the prefix and the quote; written the outputs' rounded bytes, 16 bytes of out_off /
out_len / src_index and the out_chain rows per output, and status / out_index per source.

  python scripts/icmp_bench.py [--n 1048576] [--iters 10] > profiles/icmp/icmp_bench.jsonl
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "packet-rs_amd"), os.path.join(REPO, "scripts"), REPO]
import pktgpu  # noqa: E402
from pktgpu import _lib, gen, schema  # noqa: E402
from frag_bench import big_packets, out, per_call_ms  # noqa: E402
from secondary_bench import copy_ceiling  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    n, it = a.n, a.iters
    dev = torch.device("cuda", 0)
    P = pktgpu.Parser(0)
    L = P._L
    out({"box": torch.cuda.get_device_name(0), "packets": n, "iters": it,
         "measured": "one pair of HIP events around every call (each waits for its totals); min and median over the calls, after 2 warm-up calls"})
    # every packet answerable: a unicast destination MAC and unicast addresses (C2's are random)
    a2 = gen.gen_c2(n, seed=7)
    a2[:, 0] &= 0xFE
    a2[:, 26], a2[:, 30] = 10, 11
    c2 = torch.from_numpy(a2.reshape(-1)).to(dev)
    c2_chain = P.parse(c2, stride=64, columns=["chain"])
    torch.cuda.synchronize()
    big, big_chain = big_packets(n, dev)
    big["slab"].view(n, 1504)[:, 0] = 2
    fwd = torch.zeros(n, dtype=torch.uint8, device=dev)
    for k, s in enumerate((schema.FWD_TTL, schema.FWD_MTU, schema.FWD_NO_ADJ)):
        fwd[100 * k + 7::300] = s
    works = [("icmp_c2_all", dict(slab=c2, stride=64, n=n, lens=None), {k: c2_chain[k] for k in ("n_hdrs", "hdr_type", "hdr_off")},
              dict(reason=schema.ICMP_R_TIME_EXCEEDED), 64),
             ("icmp_1500_all", big, big_chain, dict(reason=schema.ICMP_R_TOO_BIG, mtu=1400), 1500),
             ("icmp_1500_fwd_1pct", big, big_chain, dict(fwd_status=fwd, mtu=1400), 1500)]
    s = P._stream(None)
    cfg = _lib.PktIcmpCfg()
    cfg.src4[:] = bytes([192, 0, 2, 1])
    cfg.src6[:] = bytes([0x20, 0x01, 0x0d, 0xb8] + [0] * 11 + [1])
    for name, batch, chain, kw, src_b in works:
        plan = P.icmp_errors(batch, chain, src4="192.0.2.1", src6="2001:db8::1", plan_only=True, **kw)
        n_out, nbytes = plan.n_out, plan.bytes_out
        r = P.icmp_errors(batch, chain, src4="192.0.2.1", src6="2001:db8::1", out_cap=max(1, n_out), dst_bytes=nbytes, **kw)
        assert (r.n_out, r.bytes_out) == (n_out, nbytes)
        rows = int(r.out_chain["n_hdrs"].sum().item())
        st = np.bincount(r.status.cpu().numpy(), minlength=schema.ICMPE_STATUS_COUNT)
        b = P._batch(batch["slab"], n, batch["stride"], None, batch["lens"])
        ch = P._chain(chain)
        oc = P._lib.PktChain(*[r.out_chain[k].data_ptr() for k in ("n_hdrs", "hdr_type", "hdr_off")])
        tot, cnt = ctypes.c_uint64(), ctypes.c_uint64()
        code = kw.get("fwd_status")
        cmap = schema.ICMP_MAP_FWD if code is not None else None
        head = (P._ctx, ctypes.byref(b), ctypes.byref(ch), 0)
        mid = (ctypes.byref(cfg), code.data_ptr() if code is not None else None, 0 if code is not None else kw["reason"],
               cmap.ctypes.data if cmap is not None else None, None, kw["mtu"] if "mtu" in kw else 0, None, r.status.data_ptr(),
               r.out_index.data_ptr())

        def full(k):
            assert L.pkt_icmp_err_batch(*head, 0, *mid, r.slab.data_ptr(), r.slab.numel(), max(1, n_out), r.offsets.data_ptr(),
                                        r.lens.data_ptr(), r.src_index.data_ptr(), ctypes.byref(oc), None, ctypes.byref(tot),
                                        ctypes.byref(cnt), s) == 0

        def sizing(k):
            assert L.pkt_icmp_err_batch(*head, schema.ICMPE_NO_WRITE, *mid, None, 0, 0, None, None, None, None, None,
                                        ctypes.byref(tot), ctypes.byref(cnt), s) == 0
        ms, med = per_call_ms(full, it)
        ms0, med0 = per_call_ms(sizing, it)
        quoted = int(r.lens[:n_out].sum().item()) - 8 * n_out
        rd = n * (13 + 32 + (1 if code is not None else 0) + (4 if batch["lens"] is not None else 0)) + quoted
        wr = nbytes + 16 * n_out + n_out + 3 * rows + 5 * n
        ln = {"workload": name, "outputs": n_out, "out_bytes": nbytes, "status": {schema.ICMPE_STATUS[k]: int(v) for k, v in enumerate(st) if v},
              "call_us": round(ms * 1e3, 1), "call_us_median": round(med * 1e3, 1), "no_write_us": round(ms0 * 1e3, 1),
              "no_write_us_median": round(med0 * 1e3, 1), "build_us": round((ms - ms0) * 1e3, 1), "source_packet_bytes": src_b,
              "bytes": {"read": rd, "written": wr}, "GB/s_read_plus_written": round((rd + wr) / (ms * 1e-3) / 1e9, 1)}
        c = copy_ceiling(n, rd / n, wr / n, dev, it, ms)
        if c is not None:
            ln["stream_copy"] = c
        out(ln)
        del r
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
