#!/usr/bin/env python3
"""pkt_frag_batch at 2^20 packets, one JSON line per measurement.  Every call is timed by its own pair of HIP events
on the call's stream (the call waits for its totals, so calls cannot be queued back to back); the figure is the minimum
over `iters` calls after 2 warm-up calls, the median beside it.

  frag_1500_mtu576    1500-byte Ether / IPv4 / UDP packets in 1504-byte slots, every one SPLIT into 3 fragments
  frag_1500_mtu1280   the same into 2 fragments
  frag_c2_fits        C2 packets (64-byte Ether / IPv4 / UDP) at mtu 1500: every one FITS, the pass-through cost
  *_no_write          the same calls with PKT_FRAG_NO_WRITE (decision, scan and first[]): what the emit and copy
                      kernels cost is the difference

Beside each line, from the same process and run:
  (i)  a streaming copy of the call's own bytes (pkt_probe_stream_copy): read per source packet its bytes, 13 chain
       bytes and, for an indexed batch, offset and length; written the outputs' rounded bytes, 18 bytes of out_off /
       out_len / src_index / frag_index and the out_chain rows per output, and status / nfrag / first per source;
  (ii) pkt_pcap_write of the same source batch (the nearest existing variable-length packed copy: one record per
       packet), with the streaming copy of ITS bytes, so that both calls' fractions of their copy stand side by side.

  python scripts/frag_bench.py [--n 1048576] [--iters 10] > profiles/frag/frag_bench.jsonl
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
from pktgpu import gen, schema  # noqa: E402
from secondary_bench import copy_ceiling  # noqa: E402


def out(d):
    print(json.dumps(d), flush=True)


def per_call_ms(fn, iters, warm=2):
    s = torch.cuda.current_stream()
    ms = []
    for k in range(warm + iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        fn(k)
        b.record(s)
        torch.cuda.synchronize()
        if k >= warm:
            ms.append(a.elapsed_time(b))
    return min(ms), float(np.median(ms))


def big_packets(n, dev):
    """n 1500-byte Ether / IPv4 / UDP packets in 1504-byte slots (the identification differs per packet), lens = 1500."""
    p = np.zeros(1504, np.uint8)
    p[0:12] = np.arange(1, 13)
    p[12:14] = (8, 0)
    L = 1500 - 14
    p[14:34] = (0x45, 0, L >> 8, L & 255, 0, 0, 0, 0, 64, 17, 0, 0, 10, 0, 0, 1, 10, 0, 0, 2)
    p[34:42] = (0x12, 0x34, 0x00, 0x50, (L - 20) >> 8, (L - 20) & 255, 0, 0)
    p[42:1500] = (np.arange(1458) * 7 + 3) % 251
    slab = torch.from_numpy(p).to(dev).repeat(n, 1)
    ident = torch.arange(n, device=dev)
    slab[:, 18] = (ident >> 8 & 255).to(torch.uint8)
    slab[:, 19] = (ident & 255).to(torch.uint8)
    slab = slab.reshape(-1)
    lens = torch.full((n,), 1500, dtype=torch.int32, device=dev).view(torch.uint32)
    ty = torch.zeros((schema.MAX_HDRS, n), dtype=torch.uint8, device=dev)
    of = torch.zeros((schema.MAX_HDRS, n), dtype=torch.int16, device=dev)
    for j, (t, o) in enumerate((("Ether", 0), ("IPv4", 14), ("UDP", 34))):
        ty[j], of[j] = schema.HDR_ID[t], o
    chain = dict(n_hdrs=torch.full((n,), 3, dtype=torch.uint8, device=dev), hdr_type=ty, hdr_off=of.view(torch.uint16))
    return dict(slab=slab, stride=1504, n=n, lens=lens), chain


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
    c2 = torch.from_numpy(gen.gen_c2(n, seed=7).reshape(-1)).to(dev)
    c2_chain = P.parse(c2, stride=64, columns=["chain"])
    torch.cuda.synchronize()
    big, big_chain = big_packets(n, dev)
    works = [("frag_1500_mtu576", big, big_chain, 576), ("frag_1500_mtu1280", big, big_chain, 1280),
             ("frag_c2_fits", dict(slab=c2, stride=64, n=n, lens=None), {k: c2_chain[k] for k in ("n_hdrs", "hdr_type", "hdr_off")}, 1500)]
    s = P._stream(None)
    for name, batch, chain, mtu in works:
        plan = P.fragment(batch, chain, mtu=mtu, plan_only=True)
        n_out, nbytes = plan.n_out, plan.bytes_out
        r = P.fragment(batch, chain, mtu=mtu, out_cap=n_out, dst_bytes=nbytes)
        assert (r.n_out, r.bytes_out) == (n_out, nbytes)
        rows = int(r.out_chain["n_hdrs"].sum().item())
        st = np.bincount(r.status.cpu().numpy(), minlength=schema.FRAG_STATUS_COUNT)
        b = P._batch(batch["slab"], n, batch["stride"], None, batch["lens"])
        ch = P._chain(chain)
        oc = P._lib.PktChain(*[r.out_chain[k].data_ptr() for k in ("n_hdrs", "hdr_type", "hdr_off")])
        tot, cnt = ctypes.c_uint64(), ctypes.c_uint64()
        head = (P._ctx, ctypes.byref(b), ctypes.byref(ch), 0)
        tail = (r.status.data_ptr(), r.nfrag.data_ptr(), r.first.data_ptr())

        def full(k):
            assert L.pkt_frag_batch(*head, 0, None, mtu, None, *tail, r.slab.data_ptr(), r.slab.numel(), n_out, r.offsets.data_ptr(),
                                    r.lens.data_ptr(), r.src_index.data_ptr(), r.frag_index.data_ptr(), ctypes.byref(oc), None,
                                    ctypes.byref(tot), ctypes.byref(cnt), s) == 0

        def sizing(k):
            assert L.pkt_frag_batch(*head, schema.FRAG_NO_WRITE, None, mtu, None, *tail, None, 0, 0, None, None, None, None, None, None,
                                    ctypes.byref(tot), ctypes.byref(cnt), s) == 0
        ms, med = per_call_ms(full, it)
        ms0, med0 = per_call_ms(sizing, it)
        src_b = 1500 if batch["stride"] == 1504 else 64
        rd = n * (src_b + 13 + (4 if batch["lens"] is not None else 0))
        wr = nbytes + 18 * n_out + n_out + 3 * rows + 9 * n
        ln = {"workload": name, "mtu": mtu, "outputs": n_out, "out_bytes": nbytes, "split": int(st[schema.FRAG_SPLIT]), "fits": int(st[schema.FRAG_FITS]),
              "call_us": round(ms * 1e3, 1), "call_us_median": round(med * 1e3, 1), "no_write_us": round(ms0 * 1e3, 1),
              "no_write_us_median": round(med0 * 1e3, 1), "emit_and_copy_us": round((ms - ms0) * 1e3, 1),
              "bytes": {"read": rd, "written": wr}, "GB/s_read_plus_written": round((rd + wr) / (ms * 1e-3) / 1e9, 1)}
        c = copy_ceiling(n, rd / n, wr / n, dev, it, ms)
        if c is not None:
            ln["stream_copy"] = c
        # pkt_pcap_write of the same source batch, with its own streaming copy
        pdst = torch.empty(24 + n * (16 + src_b), dtype=torch.uint8, device=dev)
        kw = dict(stride=batch["stride"], lens=batch["lens"], dst=pdst, n=n)

        def pw(k):
            P.pcap_write(batch["slab"], **kw)
        pms, pmed = per_call_ms(pw, it)
        prd, pwr = n * (src_b + (4 if batch["lens"] is not None else 0)), 24 + n * (16 + src_b) + 16 * n
        ln["pcap_write"] = {"call_us": round(pms * 1e3, 1), "call_us_median": round(pmed * 1e3, 1), "bytes": {"read": prd, "written": pwr},
                            "frag_call_over_pcap_write": round(ms / pms, 3)}
        pc = copy_ceiling(n, prd / n, pwr / n, dev, it, pms)
        if pc is not None:
            ln["pcap_write"]["stream_copy"] = pc
        out(ln)
        del r, pdst
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
