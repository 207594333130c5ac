#!/usr/bin/env python3
"""pkt_reasm_batch at 2^20 fragments, one JSON line per measurement.  Every call is timed by its own pair of HIP events
on the call's stream (the call waits for its totals, so calls cannot be queued back to back); the figure is the median
over `iters` calls after 2 warm-up calls, the minimum beside it.

  reasm_1500_mtu576       the fragments Parser.fragment makes of 1500-byte packets at mtu 576 (3 each), in order
  reasm_1500_mtu1280      the same at mtu 1280 (2 each)
  *_shuffled64            the same fragments, shuffled within windows of 64
  reasm_c2_whole          C2 packets (64-byte Ether / IPv4 / UDP): every one WHOLE, the pass-through cost
  reasm_one_key           2^20 8-byte fragments that all share one key (every one PENDING: the starts repeat)
  reasm_64k_datagrams     128 datagrams of 8189 8-byte fragments each (65512 payload bytes), in order and shuffled64
  no_write_us             each workload's sizing pass alone (PKT_REASM_NO_WRITE)

Beside each line, from the same process and run:
  (i)  a streaming copy of the call's own bytes (pkt_probe_stream_copy): read per source packet its bytes, 13 chain
       bytes and, for an indexed batch, offset and length; written the outputs' rounded bytes, 20 bytes of out_off /
       out_len / src_index / nfrag and the out_chain rows per output, and status / out_index per source (the call's
       scratch traffic is its own cost and is not in the copy);
  (ii) for the fragments of 1500-byte packets, pkt_frag_batch producing them: the inverse call on the same bytes.

  python scripts/reasm_bench.py [--n 1048576] [--iters 10] > profiles/reasm/reasm_bench.jsonl
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
from frag_bench import big_packets, per_call_ms  # noqa: E402
from secondary_bench import copy_ceiling  # noqa: E402


def out(d):
    print(json.dumps(d), flush=True)


def chain_rows(n, rows, dev):
    ty = torch.zeros((schema.MAX_HDRS, n), dtype=torch.uint8, device=dev)
    of = torch.zeros((schema.MAX_HDRS, n), dtype=torch.int16, device=dev)
    for j, (t, o) in enumerate(rows):
        ty[j], of[j] = schema.HDR_ID[t], o
    return dict(n_hdrs=torch.full((n,), len(rows), dtype=torch.uint8, device=dev), hdr_type=ty, hdr_off=of.view(torch.uint16))


def tiny_fragments(n, per, dev):
    """n Ether / IPv4 fragments of 8 payload bytes in 48-byte slots: fragment k is piece k % per of datagram k // per
    (the identification; the last piece of a datagram has MF clear)."""
    p = np.zeros(48, np.uint8)
    p[0:12] = np.arange(1, 13)
    p[12:14] = (8, 0)
    p[14:34] = (0x45, 0, 0, 28, 0, 0, 0, 0, 64, 17, 0, 0, 10, 0, 0, 1, 10, 0, 0, 2)
    p[34:42] = np.arange(8) + 1
    slab = torch.from_numpy(p).to(dev).repeat(n, 1)
    k = torch.arange(n, device=dev)
    d, j = k // per, k % per
    w = j % 8191 | torch.where(j + 1 < per, 0x2000, 0)  # (with per above 8191 the starts repeat)
    slab[:, 18], slab[:, 19] = (d >> 8 & 255).to(torch.uint8), (d & 255).to(torch.uint8)
    slab[:, 20], slab[:, 21] = (w >> 8).to(torch.uint8), (w & 255).to(torch.uint8)
    lens = torch.full((n,), 42, dtype=torch.int32, device=dev).view(torch.uint32)
    return dict(slab=slab.reshape(-1), stride=48, n=n, lens=lens), chain_rows(n, (("Ether", 0), ("IPv4", 14)), dev)


def shuffled64(batch, chain, n, dev, seed=1):
    """The same packets as an indexed batch, permuted within windows of 64."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    m = n // 64 * 64
    perm = torch.arange(n, device=dev)
    perm[:m] = (torch.rand((m // 64, 64), device=dev, generator=g).argsort(dim=1) + torch.arange(0, m, 64, device=dev)[:, None]).reshape(-1)
    signed = {torch.uint64: torch.int64, torch.uint32: torch.int32, torch.uint16: torch.int16}

    def take(t, dim=0):  # (indexing is defined for the signed types)
        return t.view(signed.get(t.dtype, t.dtype)).index_select(dim, perm).contiguous().view(t.dtype)
    if batch.get("offsets") is not None:
        offs, lens = take(batch["offsets"][:n]), take(batch["lens"][:n])
    else:
        offs = (perm * batch["stride"]).to(torch.int64).view(torch.uint64)
        lens = take(batch["lens"]) if batch.get("lens") is not None else torch.full((n,), batch["stride"], dtype=torch.int32, device=dev).view(torch.uint32)
    ch = dict(n_hdrs=take(chain["n_hdrs"][:n]), hdr_type=take(chain["hdr_type"][:, :n], 1), hdr_off=take(chain["hdr_off"][:, :n], 1))
    return dict(slab=batch["slab"], offsets=offs, lens=lens, n=n), ch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    n, it = a.n, a.iters
    dev = torch.device("cuda", 0)
    P = pktgpu.Parser(0)
    L = P._L
    s = P._stream(None)
    out({"box": torch.cuda.get_device_name(0), "fragments": n, "iters": it,
         "measured": "one pair of HIP events around every call (each waits for its totals); median and min over the calls, after 2 warm-up calls"})
    works = []  # (name, batch, chain, frag_us or None)
    for mtu, k in ((576, 3), (1280, 2)):
        big, big_chain = big_packets(n // k, dev)
        ident = torch.arange(n // k, device=dev)
        sl = big["slab"].view(-1, 1504)
        sl[:, 28], sl[:, 29] = (ident >> 16 & 255).to(torch.uint8), (ident >> 24).to(torch.uint8)  # the source address: one key per packet
        f = P.fragment(big, big_chain, mtu=mtu)
        tot, cnt = ctypes.c_uint64(), ctypes.c_uint64()
        b = P._batch(big["slab"], n // k, 1504, None, big["lens"])
        ch = P._chain(big_chain)
        oc = P._lib.PktChain(*[f.out_chain[c].data_ptr() for c in ("n_hdrs", "hdr_type", "hdr_off")])

        def frag(_):
            assert L.pkt_frag_batch(P._ctx, ctypes.byref(b), ctypes.byref(ch), 0, 0, None, mtu, None, f.status.data_ptr(),
                                    f.nfrag.data_ptr(), f.first.data_ptr(), f.slab.data_ptr(), f.slab.numel(), f.n_out,
                                    f.offsets.data_ptr(), f.lens.data_ptr(), f.src_index.data_ptr(), f.frag_index.data_ptr(),
                                    ctypes.byref(oc), None, ctypes.byref(tot), ctypes.byref(cnt), s) == 0
        fmin, fmed = per_call_ms(frag, it)
        fb = dict(slab=f.slab, offsets=f.offsets, lens=f.lens, n=f.n_out)
        works.append((f"reasm_1500_mtu{mtu}", fb, f.out_chain, fmed))
        works.append((f"reasm_1500_mtu{mtu}_shuffled64", *shuffled64(fb, f.out_chain, f.n_out, dev), fmed))
        del big, sl
    c2 = torch.from_numpy(gen.gen_c2(n, seed=7).reshape(-1)).to(dev)
    c2_chain = P.parse(c2, stride=64, columns=["chain"])
    torch.cuda.synchronize()
    works.append(("reasm_c2_whole", dict(slab=c2, stride=64, n=n, lens=None), {k: c2_chain[k] for k in ("n_hdrs", "hdr_type", "hdr_off")}, None))
    works.append(("reasm_one_key", *tiny_fragments(n, 1 << 30, dev), None))
    nk = n // 8189 * 8189
    t64 = tiny_fragments(nk, 8189, dev)
    works.append(("reasm_64k_datagrams", *t64, None))
    works.append(("reasm_64k_datagrams_shuffled64", *shuffled64(*t64, nk, dev), None))
    for name, batch, chain, frag_ms in works:
        nn = batch["n"]
        r = P.reassemble(batch, chain)
        n_out, nbytes = r.n_out, r.bytes_out
        st = np.bincount(r.status.cpu().numpy(), minlength=schema.REASM_STATUS_COUNT)
        rows = int(r.out_chain["n_hdrs"].sum().item())
        b = P._batch(batch["slab"], nn, batch.get("stride"), batch.get("offsets"), batch.get("lens"))
        ch = P._chain(chain)
        oc = P._lib.PktChain(*[r.out_chain[c].data_ptr() for c in ("n_hdrs", "hdr_type", "hdr_off")])
        tot, cnt = ctypes.c_uint64(), ctypes.c_uint64()
        head = (P._ctx, ctypes.byref(b), ctypes.byref(ch), 0)
        cap = r.offsets.numel()

        def full(_):
            assert L.pkt_reasm_batch(*head, 0, None, r.status.data_ptr(), r.out_index.data_ptr(), r.slab.data_ptr(), r.slab.numel(), cap,
                                     r.offsets.data_ptr(), r.lens.data_ptr(), r.src_index.data_ptr(), r.nfrag.data_ptr(), ctypes.byref(oc),
                                     None, ctypes.byref(tot), ctypes.byref(cnt), s) == 0

        def sizing(_):
            assert L.pkt_reasm_batch(*head, schema.REASM_NO_WRITE, None, r.status.data_ptr(), r.out_index.data_ptr(), None, 0, 0, None, None,
                                     None, None, None, None, ctypes.byref(tot), ctypes.byref(cnt), s) == 0
        mn, med = per_call_ms(full, it)
        mn0, med0 = per_call_ms(sizing, it)
        assert (tot.value, cnt.value) == (nbytes, n_out)
        if batch.get("offsets") is not None:
            src_bytes = int(batch["lens"][:nn].to(torch.int64).sum().item()) + 12 * nn
        else:
            src_bytes = nn * (42 + 4 if batch["stride"] == 48 else 64)
        rd = src_bytes + 13 * nn
        wr = nbytes + 21 * n_out + 3 * rows + 5 * nn
        ln = {"workload": name, "sources": nn, "outputs": n_out, "out_bytes": nbytes, "joined": int(st[schema.REASM_JOINED]),
              "whole": int(st[schema.REASM_WHOLE]), "pending": int(st[schema.REASM_PENDING]),
              "call_us": round(med * 1e3, 1), "call_us_min": round(mn * 1e3, 1), "no_write_us": round(med0 * 1e3, 1),
              "no_write_us_min": round(mn0 * 1e3, 1), "ns_per_source": round(med * 1e6 / nn, 2),
              "bytes": {"read": rd, "written": wr}, "GB/s_read_plus_written": round((rd + wr) / (med * 1e-3) / 1e9, 1)}
        c = copy_ceiling(nn, rd / nn, wr / nn, dev, it, med)
        if c is not None:
            ln["stream_copy"] = c
        if frag_ms is not None:
            ln["pkt_frag_batch_us"] = round(frag_ms * 1e3, 1)
            ln["reasm_over_frag"] = round(med / frag_ms, 3)
        out(ln)
        del r
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
