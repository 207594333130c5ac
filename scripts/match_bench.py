#!/usr/bin/env python3
"""pkt_match_batch on C2 (2^20 x 64 B Ether/IPv4/UDP packets from pkt_gen_run), one JSON line per measurement
(HIP events over back-to-back launches on one stream after warm-up launches; the median of 5 rounds):

  match_<program>_<outputs>   program a = one rule of one term (UDP dst port), b = a 16-rule 5-tuple ACL (src and
                              dst prefix by mask, protocol, source- and destination-port range), c = 64 rules of
                              4 terms; outputs = `select` alone, or rule + action + select + matched + hits +
                              bytes.  Beside each: a streaming copy of the same bytes in and out
                              (pkt_probe_stream_copy) and the call's fraction of it, and what a user could do
                              before pkt_match_batch: pkt_extract_fields of the program's distinct fields plus
                              the torch expression that yields the same `select` (the two masks are compared, and
                              the first call's hits / bytes with the histogram of its own `rule` column).

  python scripts/match_bench.py [--n 1048576] [--iters 20] > profiles/match/match_bench.jsonl
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "packet-rs_amd"), os.path.join(REPO, "scripts"), REPO]
import pktgpu  # noqa: E402
from pktgpu import fields, pktgen, schema  # noqa: E402
from secondary_bench import copy_ceiling, event_ms  # noqa: E402

FIELD = {"src": ("IPv4", "src"), "dst": ("IPv4", "dst"), "proto": ("IPv4", "protocol"), "sport": ("UDP", "src"),
         "dport": ("UDP", "dst")}
DPORTS = [53, 80, 443, 8080]


def out(d):
    print(json.dumps(d), flush=True)


def population(n, dev, seed):
    """Per packet: 16 source /24s x 16 destination /24s, source ports 1000..33767, four destination ports."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    r = lambda hi: torch.randint(0, hi, (n,), generator=g).to(dev)  # noqa: E731
    u = lambda t: t.to(torch.uint64)  # noqa: E731
    dp = torch.tensor(DPORTS, dtype=torch.int64, device=dev)[r(4)]
    return {"ipv4_src": u(0x0A000000 + (r(16) << 8) + r(256)), "ipv4_dst": u(0xAC100000 + (r(16) << 8) + r(256)),
            "udp_src": u(1000 + r(32768)), "udp_dst": u(dp)}


def programs():
    """name -> (rules, default); a rule is (action, [(field key, "==" | "in", a, b)]), b the mask or the upper end."""
    a = [(1, [("dport", "==", 53, 0xFFFF)])]
    b = []
    for r in range(16):
        b.append((0 if r % 3 == 0 else 100 + r,
                  [("src", "==", 0x0A000000 + ((r % 4) << 8), 0xFFFFFC00 if r % 2 else 0xFFFFFF00),
                   ("dst", "==", 0xAC100000 + ((r // 4) << 10), 0xFFFFFC00), ("proto", "==", 17, 0xFF),
                   ("sport", "in", 1000 + 1000 * r, 20000 + 1000 * r), ("dport", "in", 0, 1023 if r % 2 else 100)]))
    c = []
    for r in range(64):
        c.append((r % 2, [("src", "==", 0x0A000000 + ((r % 16) << 8), 0xFFFFFF00), ("dst", "==", 0, 0) if r % 4 == 0 else
                          ("dst", "==", 0xAC100000 + ((r // 4) << 8), 0xFFFFFF00),
                          ("sport", "in", 1000 + 400 * r, 9000 + 400 * r), ("dport", "in", 53, 443 if r % 8 else 53)]))
    return {"a_1rule_1term": (a, 0), "b_acl_16x5": (b, 7), "c_64x4": (c, 0)}


def to_rules(prog):
    return [(act, [(FIELD[k][0], 0, FIELD[k][1], op, x, y) for k, op, x, y in tl]) for act, tl in prog]


def torch_select(P, slab, chain, prog, default):
    """(launch(k) -> select, the distinct field keys): extract_fields + the first-match expression."""
    keys = sorted({k for _, tl in prog for k, _, _, _ in tl})
    specs = [(FIELD[k][0], 0) + fields.FIELDS[schema.HDR_ID[FIELD[k][0]]][FIELD[k][1]] for k in keys]

    def launch(k):
        vals, found = P.extract_fields(slab, chain, specs, stride=64)
        v = {key: (x.view(torch.int64), f != 0) for key, x, f in zip(keys, vals, found)}
        n = slab.numel() // 64
        done = torch.zeros(n, dtype=torch.bool, device=slab.device)
        sel = torch.full((n,), default != 0, dtype=torch.bool, device=slab.device)
        for act, tl in prog:
            m = torch.ones(n, dtype=torch.bool, device=slab.device)
            for key, op, x, y in tl:
                val, f = v[key]
                m &= f & ((((val ^ x) & y) == 0) if op == "==" else ((val >= x) & (val <= y)))
            new = m & ~done
            sel = torch.where(new, act != 0, sel)
            done |= m
        return sel.view(torch.uint8)
    return launch, keys


def median_ms(launch, it, rounds=5, warm=3):
    return statistics.median(event_ms(launch, it, warm=warm) for _ in range(rounds))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    n, it = a.n, a.iters
    dev = torch.device("cuda", 0)
    P = pktgpu.Parser(0)
    out({"box": torch.cuda.get_device_name(0), "packets": n, "iters": it,
         "measured": "HIP events around back-to-back launches on one stream, after 3 warm-up launches; median of 5 rounds"})
    slab = pktgen.gen_udp(P, n, population(n, dev, 1))
    chain = P.parse(slab, stride=64, columns=["chain"])
    torch.cuda.synchronize()
    s = P._stream(None)
    for name, (prog, default) in programs().items():
        mp = P.match_program(to_rules(prog), default)
        full = P.match(slab, chain, mp, stride=64, hits=True, bytes=True)
        tl, keys = torch_select(P, slab, chain, prog, default)
        same = bool(torch.equal(tl(0), full["select"]))
        torch.cuda.synchronize()
        hits = full["hits"].cpu().tolist()
        # the counters of that one call against the call's own per-packet rules (every packet is 64 bytes)
        slot = torch.where(full["rule"] == pktgpu.MATCH_NONE, mp.nrules, full["rule"].to(torch.int64))
        exact = hits == torch.bincount(slot, minlength=mp.nrules + 1).cpu().tolist() and \
            full["bytes"].cpu().tolist() == [64 * h for h in hits] and sum(hits) == n
        tms = median_ms(tl, max(2, it // 4), rounds=3, warm=1)
        b, ch = P._batch(slab, None, 64, None, None), P._chain(chain)
        ptr = lambda k: full[k].data_ptr()  # noqa: E731
        for mode, args, wb in (("select", (None, None, ptr("select"), None, None, None), 1),
                               ("all_outputs", tuple(ptr(k) for k in ("rule", "action", "select", "matched", "hits", "bytes")), 14)):
            def launch(k):
                assert P._L.pkt_match_batch(mp._m, ctypes.byref(b), ctypes.byref(ch), *args, s) == 0
            ms = median_ms(launch, it)
            d = {"workload": f"match_{name}_{mode}", "rules": mp.nrules, "terms": mp.nterms, "kernel_us": round(ms * 1e3, 2),
                 "Gpkt/s": round(n / (ms * 1e-3) / 1e9, 3),
                 "bytes_per_pkt": {"read_slab": 64, "written": wb, "chain_columns_read": 1 + 4 * 3},
                 "first_match_histogram": {"rules_hit": sum(1 for h in hits[:-1] if h), "none": hits[-1]},
                 "extract_fields_plus_torch_us": round(tms * 1e3, 2), "distinct_fields_extracted": len(keys),
                 "match_frac_of_extract_plus_torch": round(ms / tms, 4), "select_equals_torch_expression": same,
                 "counters_equal_histogram_of_rule": exact}
            c = copy_ceiling(n, 64, wb, dev, it, ms)
            if c is not None:
                d["stream_copy"] = c
            out(d)
        mp.close()


if __name__ == "__main__":
    main()
