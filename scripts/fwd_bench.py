#!/usr/bin/env python3
"""pkt_fwd_batch at 2^20 C2 packets (Ether / IPv4 / UDP in 64-byte slots, ttl 255), one JSON line per measurement (HIP
events over back-to-back launches on one stream after warm-up launches; the min of 3 rounds, as scripts/lpm_bench.py;
the slab is put back from a pristine copy before every round, outside the timed window, so that the ttl never runs
out):

  fwd_nexthop_adj<k>          `nexthop` given (uniform over the table), k = 1 / 256 / 65,536 adjacencies, outputs
                              status + port + adj_index.  Of every 64 adjacencies one drops, one punts and one has an
                              mtu below the packets' L3 length; the rest forward.
  fwd_lpm_<routes>            `lpm` fused, with scripts/lpm_bench.py's 1,024- and 2^16-drawn (65,381 distinct) IPv4
                              route tables and its destination addresses (the same seed and draws), 256 adjacencies.
  fwd_nexthop_adj256_no_write PKT_FWD_NO_WRITE: what the stores into the slab cost is the difference to the line above.
  fwd_nexthop_adj256_counters the same with hits + bytes.

Beside each line, from the same process and run:
  (i)   a streaming copy of the call's own bytes (pkt_probe_stream_copy): per packet 13 chain bytes, the aligned
        16-byte slab chunks read (two for the IP header's first 12 bytes; with lpm two more for the address), the next
        hop (4), and written the outputs (9) and the 15 rewritten packet bytes.  The adjacency entry and the trie's
        entries are gathered on top of that and are not part of the copy.
  (ii)  what a user could do before this call: [Lpm.lookup, with lpm] + pkt_extract_fields of ttl / total_len / the
        two MACs + torch gathers from per-field adjacency tensors + torch masks for expiry, action and mtu +
        pkt_set_fields_csum with three per-packet value arrays (a refused packet gets its own values back).  Its
        status and port are checked equal to the kernel's before it is timed.  (It recomputes the checksum where the
        kernel updates it, so the slabs are not compared.)
  (iii) for the lpm lines, Lpm.lookup followed by the unfused run.

  python scripts/fwd_bench.py [--n 1048576] [--iters 20] > profiles/fwd/fwd_bench.jsonl
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
from pktgpu import pktgen, schema  # noqa: E402
from secondary_bench import copy_ceiling, event_ms  # noqa: E402
import lpm_bench  # noqa: E402

SPECS = [("IPv4", 0, 64, 71), ("IPv4", 0, 16, 31), ("Ether", 0, 0, 47), ("Ether", 0, 48, 95)]  # ttl, total_len, dst, src
SET = [("Ether", 0, 0, 47), ("Ether", 0, 48, 95), ("IPv4", 0, 64, 71)]


def out(d):
    print(json.dumps(d), flush=True)


def adjacencies(k, rng):
    arr = np.zeros(k, schema.FWD_ADJ_DTYPE)
    arr["dmac"], arr["smac"] = rng.integers(0, 256, (k, 6), dtype=np.uint8), rng.integers(0, 256, (k, 6), dtype=np.uint8)
    idx = np.arange(k)
    arr["port"] = idx % 16
    arr["mtu"] = np.where(idx % 64 == 45, 40, 1500)
    arr["action"] = np.where(idx % 64 == 13, 1, np.where(idx % 64 == 29, 2, 0))
    return arr


def mac48(m):
    return (m.astype(np.int64) << (8 * np.arange(5, -1, -1))).sum(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    n, it = a.n, a.iters
    assert it + 3 < 250, "the ttl starts at 255 and every launch takes one off"
    dev = torch.device("cuda", 0)
    P = pktgpu.Parser(0)
    out({"box": torch.cuda.get_device_name(0), "packets": n, "iters": it, "seed": lpm_bench.SEED,
         "measured": "HIP events around back-to-back launches on one stream, after 3 warm-up launches; min of 3 rounds; "
                     "the slab restored before each round"})
    rng = np.random.default_rng(lpm_bench.SEED)
    arng = np.random.default_rng(lpm_bench.SEED + 1)
    s = P._stream(None)
    # lpm_bench's tables and destinations, drawn in its order: (1 route), 2^10, 2^16
    tables = {}
    for count in (1, 1 << 10, 1 << 16):
        plen, prefix = lpm_bench.synth_routes(rng, count, lpm_bench.V4_DIST, False)
        tables[count] = (plen, prefix, lpm_bench.draw_dst(rng, n, plen, prefix, False))
    ttl = torch.full((n,), 255, dtype=torch.int64, device=dev).view(torch.uint64)
    configs = [("nexthop", 1, None, 0, False), ("nexthop", 256, None, 0, False), ("nexthop", 65536, None, 0, False),
               ("lpm", 256, 1 << 10, 0, False), ("lpm", 256, 1 << 16, 0, False),
               ("nexthop", 256, None, schema.FWD_NO_WRITE, False), ("nexthop", 256, None, 0, True)]
    for mode, nadj, count, flags, counters in configs:
        fused = mode == "lpm"
        plen, prefix, dst = tables[count if fused else 1 << 10]
        pristine = pktgen.gen_udp(P, n, {"ipv4_dst": torch.from_numpy(dst.astype(np.int64)).to(dev).view(torch.uint64), "ipv4_ttl": ttl})
        slab = pristine.clone()
        chain = P.parse(slab, stride=64, columns=["chain"])
        cols = {c: chain[c] for c in ("n_hdrs", "hdr_type", "hdr_off")}
        batch = dict(slab=slab, stride=64, n=n)
        arr = adjacencies(nadj, arng)
        fwd = P.forwarder(arr)
        lpm = None
        if fused:
            routes = lpm_bench.route_array(plen, prefix, False)
            routes["nexthop"] = np.arange(plen.size, dtype=np.uint32) % nadj
            lpm = P.lpm(routes, default_nexthop=0xFFFF)
            nexthop = None
        else:
            nexthop = torch.from_numpy(arng.integers(0, nadj, n).astype(np.int32)).to(dev).view(torch.uint32)
        t_act, t_mtu, t_port = (torch.from_numpy(arr[k].astype(np.int64)).to(dev) for k in ("action", "mtu", "port"))
        t_dmac, t_smac = torch.from_numpy(mac48(arr["dmac"])).to(dev), torch.from_numpy(mac48(arr["smac"])).to(dev)
        none = torch.tensor(schema.FWD_NONE, dtype=torch.int64, device=dev)

        def before(k, write=True):
            nh = lpm.lookup(batch, cols, outputs=("nexthop",))["nexthop"] if fused else nexthop
            vals, found = P.extract_fields(slab, cols, SPECS, stride=64)
            tt, tl, dm, sm = (v.view(torch.int64) for v in vals)
            ai = nh.view(torch.int32).to(torch.int64)
            inr = (ai >= 0) & (ai < nadj)
            ac = ai.clamp(0, nadj - 1)
            act, mtu = t_act[ac], t_mtu[ac]
            big = (mtu != 0) & (tl > mtu)
            st = torch.where(found[0] == 0, 2, torch.where(tt <= 1, 5, torch.where(~inr, 6, torch.where(
                act == 1, 7, torch.where(act == 2, 8, torch.where(big, 9, 0))))))
            ok = st == 0
            port = torch.where(ok, t_port[ac], none)
            if write:
                P.set_fields(slab, cols, SET, [torch.where(ok, t_dmac[ac], dm).view(torch.uint64), torch.where(ok, t_smac[ac], sm).view(torch.uint64),
                                               torch.where(ok, tt - 1, tt).view(torch.uint64)], stride=64, ipv4_checksum=0)
            return st, port

        res = fwd.run(batch, cols, nexthop=nexthop, lpm=lpm, write=False)
        bst, bport = before(0, write=False)
        torch.cuda.synchronize()
        same = bool(torch.equal(bst, res["status"].to(torch.int64))) and bool(torch.equal(bport, res["port"].view(torch.int32).to(torch.int64) & 0xFFFFFFFF))
        assert same, "the torch path and the kernel disagree"
        ok_share = float((res["status"] == 0).float().mean())
        hits = torch.zeros(10, dtype=torch.uint64, device=dev)
        byts = torch.zeros(10, dtype=torch.uint64, device=dev)
        b = P._batch(slab, n, 64, None, None)
        ch = P._chain(cols)
        args = (ctypes.byref(b), ctypes.byref(ch), 0, flags, None if lpm is None else lpm._t, None if fused else nexthop.data_ptr(), None,
                res["status"].data_ptr(), res["port"].data_ptr(), res["adj_index"].data_ptr(),
                hits.data_ptr() if counters else None, byts.data_ptr() if counters else None, s)

        def launch(k):
            assert P._L.pkt_fwd_batch(fwd._f, *args) == 0

        def timed(fn, iters, warm):
            best = None
            for _ in range(3):
                slab.copy_(pristine)
                ms = event_ms(fn, iters, warm=warm)
                best = ms if best is None else min(best, ms)
            return best
        ms = timed(launch, it, 3)
        bms = timed(before, max(2, it // 4), 1)
        name = f"fwd_{mode}_" + (f"{plen.size}" if fused else f"adj{nadj}") + ("_no_write" if flags else "") + ("_counters" if counters else "")
        rd, wr = 13 + 32 + (32 if fused else 4), 9 + (0 if flags else 15)
        ln = {"workload": name, "adjacencies": nadj, "ok_share": round(ok_share, 4), "kernel_us": round(ms * 1e3, 2),
              "Gpkt/s": round(n / (ms * 1e-3) / 1e9, 3), "bytes_per_pkt": {"read": rd, "written": wr},
              "before_extract_gather_mask_set_us": round(bms * 1e3, 2), "fwd_frac_of_before": round(ms / bms, 4),
              "status_and_port_equal_before": same}
        if fused:
            ln["routes"] = int(plen.size)
            nh_buf = torch.empty(n, dtype=torch.uint32, device=dev)
            uargs = args[:4] + (None, nh_buf.data_ptr()) + args[6:]

            def pair(k):
                assert P._L.pkt_lpm_lookup_batch(lpm._t, ctypes.byref(b), ctypes.byref(ch), 0, 0, None, nh_buf.data_ptr(), None, None, s) == 0
                assert P._L.pkt_fwd_batch(fwd._f, *uargs) == 0
            pms = timed(pair, it, 3)
            ln["lookup_then_unfused_run_us"] = round(pms * 1e3, 2)
            ln["fwd_frac_of_unfused_pair"] = round(ms / pms, 4)
        c = copy_ceiling(n, rd, wr, dev, it, ms)
        if c is not None:
            ln["stream_copy"] = c
        out(ln)
        fwd.close()
        if lpm is not None:
            lpm.close()
        del slab, pristine, chain, cols, res
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
