#!/usr/bin/env python3
"""Flow keys and the flow table on C2 (2^20 x 64 B Ether/IPv4/UDP packets from pkt_gen_run), one JSON line per
measurement (HIP events over back-to-back launches on one stream, scripts/secondary_bench.py's idiom):

  flow_keys / flow_keys_rss   pkt_flow_key_batch without and with the Toeplitz hash, beside a streaming copy of
                              the bytes it must move (pkt_probe_stream_copy: 64 B in, 40 + 8 + 1 + 4 + 1 B out,
                              + 4 with rss) and its fraction of that copy;
  flow_update_<population>    pkt_flow_table_update (its three launches) for 1 flow, 2^16 flows drawn uniformly
                              and 2^20 distinct flows, beside the same box's torch expression for the same
                              answer: torch.unique(keys, dim=0, return_inverse=True) + bincount + index_add_.

If the 1-flow shape takes longer than the 2^20-flow shape, the wave aggregation is not doing its job: the
last line says which way it came out.

  python scripts/flow_bench.py [--n 1048576] [--iters 20] > profiles/flow/flow_bench.jsonl
"""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "packet-rs_amd"), os.path.join(REPO, "scripts"), REPO]
import pktgpu  # noqa: E402
from pktgpu import pktgen  # noqa: E402
from secondary_bench import copy_ceiling, event_ms  # noqa: E402

RSS_KEY = bytes.fromhex("6d5a56da255b0ec24167253d43a38fb0d0ca2bcbae7b30b477cb2da38030f20c6a42b73bbeac01fa")


def out(d):
    print(json.dumps(d), flush=True)


def population(n, flows, dev, seed):
    """Per packet: ipv4_src, ipv4_dst, udp_src, udp_dst (uint64 device tensors) of `flows` distinct flows."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    f = torch.zeros(n, dtype=torch.int64) if flows == 1 else \
        torch.arange(n, dtype=torch.int64) if flows == n else torch.randint(0, flows, (n,), generator=g)
    f = f.to(dev)
    u = lambda t: t.to(torch.uint64)  # noqa: E731
    return {"ipv4_src": u(0x0A000000 + f), "ipv4_dst": u(0x0B000000 + (f * 7919) % (1 << 24)),
            "udp_src": u(1024 + f % 60000), "udp_dst": u(53 + (f >> 16))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    n, it = a.n, a.iters
    dev = torch.device("cuda", 0)
    P = pktgpu.Parser(0)
    out({"box": torch.cuda.get_device_name(0), "packets": n, "iters": it,
         "measured": "HIP events around back-to-back launches on one stream, after 3 warm-up launches"})
    slab = pktgen.gen_udp(P, n, population(n, 1 << 16, dev, 1))
    chain = P.parse(slab, stride=64, columns=["chain"])
    torch.cuda.synchronize()
    # ---- the key kernel
    for name, rk in (("flow_keys", None), ("flow_keys_rss", RSS_KEY)):
        args, outs, keep = P._flow_args(slab, chain, symmetric=True, seed=1, rss_key=rk, stride=64)
        s = P._stream(None)

        def launch(k):
            assert P._L.pkt_flow_key_batch(P._ctx, *args, s) == 0
        ms = min(event_ms(launch, it) for _ in range(3))
        rb, wb = 64, 40 + 8 + 1 + 4 + 1 + (4 if rk else 0)
        d = {"workload": name, "kernel_us": round(ms * 1e3, 2), "Gpkt/s": round(n / (ms * 1e-3) / 1e9, 3),
             "bytes_per_pkt": {"read_slab": rb, "written": wb, "chain_columns_read": 1 + 4 * 3},
             "GB/s_slab_plus_outputs": round((rb + wb) * n / (ms * 1e-3) / 1e9, 1)}
        c = copy_ceiling(n, rb, wb, dev, it, ms)
        if c is not None:
            d["stream_copy"] = c
        out(d)
    # ---- the table
    res = {}
    for label, flows in (("1_flow", 1), ("65536_flows_uniform", 1 << 16), ("1048576_distinct_flows", n)):
        slab = pktgen.gen_udp(P, n, population(n, flows, dev, 2))
        keys = P.flow_keys(slab, chain, symmetric=True, seed=1, stride=64)
        slots = max(64, 1 << (2 * min(flows, n) - 1).bit_length())       # load factor <= 1/2
        t = pktgpu.FlowTable(P, slots)
        uargs, uouts, ukeep = t._update_args(keys, "plen", 0)
        s = P._stream(None)
        base = [0]

        def update(k):
            a_ = list(uargs)
            a_[6] = base[0]                                                 # a rising base, as a stream gives it
            base[0] += n
            assert P._L.pkt_flow_table_update(t._t, *a_, s) == 0
        warm = event_ms(update, 1, warm=0)                                  # the first update inserts every flow
        ms = min(event_ms(update, it) for _ in range(3))
        assert t.count() == flows and int(t.flows()["pkts"].sum()) == base[0]

        def torch_way(k):
            uniq, inv = torch.unique(keys["keys"], dim=0, return_inverse=True)
            pk = torch.bincount(inv, minlength=uniq.shape[0])
            by = torch.zeros(uniq.shape[0], dtype=torch.int64, device=dev).index_add_(0, inv, keys["plen"].to(torch.int64))
            return pk, by
        tms = min(event_ms(torch_way, max(2, it // 5), warm=1) for _ in range(2))
        res[label] = ms
        out({"workload": f"flow_update_{label}", "flows": flows, "slots": slots, "update_us": round(ms * 1e3, 2),
             "first_update_us_with_inserts": round(warm * 1e3, 2), "Gpkt/s": round(n / (ms * 1e-3) / 1e9, 3),
             "launches": 3, "torch_unique_bincount_index_add_us": round(tms * 1e3, 2),
             "update_frac_of_torch": round(ms / tms, 4)})
        t.close()
    one, many = res["1_flow"], res["1048576_distinct_flows"]
    out({"wave_aggregation": "1 flow is faster than 2^20 distinct flows" if one <= many else
         "1 flow is SLOWER than 2^20 distinct flows: the wave aggregation is not doing its job",
         "one_flow_us": round(one * 1e3, 2), "distinct_flows_us": round(many * 1e3, 2)})


if __name__ == "__main__":
    main()
