#!/usr/bin/env python3
"""pkt_dispatch_batch and pkt_reorder_batch at 2^20 packets, one JSON line per measurement (HIP events over
back-to-back launches on one stream after warm-up launches; the min of 3 rounds, as scripts/flow_bench.py):

  dispatch_<keys>_<outputs>   keys = 4 / 64 / 256 uniform buckets (DIRECT mode), one bucket only, or a 128-entry
                              indirection table over 4 queues on uniform 32-bit hashes; outputs = bucket + perm +
                              rank + start, or perm + start alone.  Beside each: a streaming copy of the line's
                              algorithmic bytes (pkt_probe_stream_copy) and what a user can do without the call:
                              torch.sort(bucket, stable=True) + bincount + cumsum on the ready bucket column.
  reorder_c2_chain            2^20 C2 packets (64-byte slots) and the three chain columns gathered by the
                              64-bucket dispatch's perm into per-bucket segments.  Beside it: the copy of its bytes,
                              and index_select on the [n, 64] slab view plus one per column (slot rows: one
                              index_select on the [16, n] view, which does not give the per-segment layout).

  python scripts/dispatch_bench.py [--n 1048576] [--iters 20] > profiles/dispatch/dispatch_bench.jsonl
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "packet-rs_amd"), os.path.join(REPO, "scripts"), REPO]
import pktgpu  # noqa: E402
from pktgpu import pktgen  # noqa: E402
from secondary_bench import copy_ceiling, event_ms  # noqa: E402


def out(d):
    print(json.dumps(d), flush=True)


def min_ms(launch, it, rounds=3, warm=3):
    return min(event_ms(launch, it, warm=warm) for _ in range(rounds))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    n, it = a.n, a.iters
    dev = torch.device("cuda", 0)
    P = pktgpu.Parser(0)
    out({"box": torch.cuda.get_device_name(0), "packets": n, "iters": it,
         "measured": "HIP events around back-to-back launches on one stream, after 3 warm-up launches; min of 3 rounds"})
    rng = np.random.default_rng(5)
    s = P._stream(None)
    table = [k % 4 for k in range(128)]
    uni = lambda hi: rng.integers(0, hi, n, dtype=np.uint64).astype(np.uint32)  # noqa: E731
    lines = [("4_buckets", 4, None, uni(4)), ("64_buckets", 64, None, uni(64)), ("256_buckets", 256, None, uni(256)),
             ("one_bucket_of_64", 64, None, np.full(n, 17, np.uint32)), ("table128_4_queues", 4, table, uni(1 << 32))]
    perm64 = start64 = None
    for name, nb, tab, key in lines:
        key = torch.from_numpy(key.view(np.int32)).to(dev).view(torch.uint32)
        d = P.dispatcher(nb, tab, max_n=n)
        full = d.run(key)
        # the torch path works on the ready bucket column (int64 for bincount; dropped packets do not occur here)
        bcol = full["bucket"].view(torch.int16).to(torch.int64)

        def torch_way(k):
            srt, perm = torch.sort(bcol, stable=True)
            start = torch.cumsum(torch.bincount(bcol, minlength=nb), 0)
            return perm, start
        tperm, tstart = torch_way(0)
        torch.cuda.synchronize()
        same = bool(torch.equal(tperm, full["perm"].view(torch.int32).to(torch.int64))) and \
            tstart.cpu().tolist() == full["start"].cpu().tolist()[1:nb + 1]
        tms = min_ms(torch_way, max(2, it // 4), rounds=3, warm=1)
        if name == "64_buckets":
            perm64, start64 = full["perm"], full["start"]
        ptr = lambda k: full[k].data_ptr()  # noqa: E731
        for mode, args, wb in (("all_outputs", (ptr("bucket"), ptr("perm"), ptr("rank"), ptr("start")), 10),
                               ("perm_start", (None, ptr("perm"), None, ptr("start")), 4)):
            def launch(k):
                assert P._L.pkt_dispatch_batch(d._d, key.data_ptr(), None, n, *args, s) == 0
            ms = min_ms(launch, it)
            # the keys are read twice (count, place); the [bucket][tile] counts are written, scanned and read
            scratch = 3 * 4 * (nb + 1) * ((n + 2047) // 2048) / n
            ln = {"workload": f"dispatch_{name}_{mode}", "nbuckets": nb, "table_len": len(tab) if tab else 0,
                  "kernel_us": round(ms * 1e3, 2), "Gpkt/s": round(n / (ms * 1e-3) / 1e9, 3),
                  "bytes_per_pkt": {"keys_read": 8, "written": wb, "scratch_counts": round(scratch, 2)},
                  "torch_sort_bincount_cumsum_us": round(tms * 1e3, 2), "dispatch_frac_of_torch": round(ms / tms, 4),
                  "perm_and_start_equal_torch": same}
            c = copy_ceiling(n, 8, wb, dev, it, ms)
            if c is not None:
                ln["stream_copy"] = c
            out(ln)
        d.close()
    # ---- reorder: C2 packets and their chain by the 64-bucket perm
    slab = pktgen.gen_udp(P, n, {"udp_src": (1000 + torch.arange(n, device=dev) % 30000).to(torch.uint64)})
    chain = P.parse(slab, stride=64, columns=["chain"])
    cols = {c: chain[c] for c in ("n_hdrs", "hdr_type", "hdr_off")}
    ro = P.reorder(perm64, slab, stride=64, columns=cols, start=start64, slot=64)
    idx = perm64.view(torch.int32).to(torch.int64)
    rows = slab.view(n, 64)

    def torch_way(k):
        return (rows.index_select(0, idx), cols["n_hdrs"].index_select(0, idx), cols["hdr_type"].index_select(1, idx),
                cols["hdr_off"].index_select(1, idx))
    tw = torch_way(0)
    torch.cuda.synchronize()
    same = bool(torch.equal(tw[0].reshape(-1), ro["slab"])) and bool(torch.equal(tw[1], ro["columns"]["n_hdrs"]))
    tms = min_ms(torch_way, max(2, it // 4), rounds=3, warm=1)

    def launch(k):
        P.reorder(perm64, slab, stride=64, columns=cols, start=start64, slot=64, out=ro)
    ms = min_ms(launch, it)
    # C2's chain is 3 headers: n_hdrs + 3 rows of hdr_type (1 B) and hdr_off (2 B), read and written
    rb, wb = 4 + 64 + 1 + 3 * 3, 64 + 4 + 1 + 3 * 3
    ln = {"workload": "reorder_c2_chain", "nseg": 64, "slot": 64, "kernel_us": round(ms * 1e3, 2),
          "Gpkt/s": round(n / (ms * 1e-3) / 1e9, 3), "launches": 2,
          "bytes_per_pkt": {"read": rb, "written": wb},
          "torch_index_select_x4_us": round(tms * 1e3, 2), "reorder_frac_of_torch": round(ms / tms, 4),
          "bytes_and_n_hdrs_equal_torch": same}
    c = copy_ceiling(n, rb, wb, dev, it, ms)
    if c is not None:
        ln["stream_copy"] = c
    out(ln)


if __name__ == "__main__":
    main()
