#!/usr/bin/env python3
"""pkt_tunnel_encap_batch / pkt_tunnel_decap_batch at 2^20 packets, one JSON line per measurement.  Every call is timed
on its own: a HIP event pair around the queued (_async) call with caller-sized outputs marshalled once, the totals taken
after the second event; a line reports the mean of its launches, the min of 3 rounds.

  encap_vxlan4_c2            C2 (Ether / IPv4 / UDP, 64 bytes in 64-byte slots) into one VXLAN / IPv4 tunnel, 64 -> 114 bytes
  encap_vxlan4_c2_csum       the same with PKT_TUN_F_UDP_CSUM
  encap_vxlan4_c2_65536      the same (no checksum) into 65536 tunnels drawn uniformly
  encap_vxlan4_c2_65536_csum ... with PKT_TUN_F_UDP_CSUM
  encap_gre6_1500            1500-byte packets into GRE / IPv6
  decap_*                    the decap of each of those outputs through its out_chain

Beside each line, from the same process and run:
  (i)   a streaming copy of the call's own bytes (pkt_probe_stream_copy): per packet the source bytes, the chain rows
        and the per-packet inputs read, the 32-byte plan written and read, the rounded output, its per-output row and
        chain rows and the per-packet outputs written;
  (ii)  for the C2 encaps, Parser.edit's constant-header VXLAN insert on the same batch (what a user had: the outer
        lengths and checksum are whatever the constant bytes hold), and for the decaps edit's remove(0) x 4;
  (iii) for UDP_CSUM, the two-call alternative: encap without it, then l4_checksum(which=0, update=True) on the output.
A call's per-kernel times come from a kernel trace of this script with --trace-case (one warm call, one traced call).

  python scripts/tunnel_bench.py [--n 1048576] [--iters 10] > profiles/tunnel/tunnel_bench.jsonl
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

MAXH = schema.MAX_HDRS


def out(d):
    print(json.dumps(d), flush=True)


def each_ms(fn, iters, after=None):
    """The mean of `iters` launches, each between its own event pair; after() runs behind the second event, untimed."""
    s = torch.cuda.current_stream()
    fn()
    if after:
        after()
    total = 0.0
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        fn()
        b.record(s)
        if after:
            after()
        torch.cuda.synchronize()
        total += a.elapsed_time(b)
    return total / iters


class Call:
    """One tunnel call with its outputs allocated and its arguments marshalled once."""

    def __init__(self, P, tun, op, batch, chain, n, cap, dst_bytes, tunnel=0, entropy=None):
        dev = P.torch_device
        self.P, self.op, self.n, self.cap = P, op, n, cap
        L = P._L
        self.fa, self.fr = getattr(L, f"pkt_tunnel_{op}_batch_async"), getattr(L, f"pkt_tunnel_{op}_result")
        self.b = P._batch(batch["slab"], batch.get("n"), batch.get("stride"), batch.get("offsets"), batch.get("lens"))
        self.ch = P._chain(chain)
        z = lambda k, dt: torch.zeros(k, dtype=dt, device=dev)  # noqa: E731
        self.status, self.out_index, self.tunnel_out = z(n, torch.uint8), z(n, torch.uint32), z(n, torch.uint32)
        self.dst, self.offsets, self.lens, self.src_index = z(dst_bytes, torch.uint8), z(cap, torch.uint64), z(cap, torch.uint32), z(cap, torch.uint32)
        self.out_chain = dict(n_hdrs=z(cap, torch.uint8), hdr_type=z((MAXH, cap), torch.uint8), hdr_off=z((MAXH, cap), torch.uint16))
        self.oc = P._chain(self.out_chain)
        self.keep = (batch, chain, tunnel, entropy)
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        head = [P._ctx, ctypes.byref(self.b), ctypes.byref(self.ch), 0, 0, tun._t]
        if op == "encap":
            per = torch.is_tensor(tunnel)
            mid = [ptr(tunnel) if per else None, 0 if per else int(tunnel), ptr(entropy), 0, None, ptr(self.status), ptr(self.out_index)]
        else:
            mid = [None, ptr(self.status), ptr(self.out_index), ptr(self.tunnel_out)]
        self.args = head + mid + [ptr(self.dst), dst_bytes, cap, ptr(self.offsets), ptr(self.lens), ptr(self.src_index),
                                  ctypes.byref(self.oc), None]
        self.tot, self.cnt = ctypes.c_uint64(0), ctypes.c_uint64(0)

    def queue(self):
        rc = self.fa(*self.args, self.P._stream(None))
        assert rc == 0, self.P._L.pkt_ctx_last_error(self.P._ctx)

    def take(self):
        rc = self.fr(self.P._ctx, ctypes.byref(self.tot), ctypes.byref(self.cnt))
        assert rc == 0, self.P._L.pkt_ctx_last_error(self.P._ctx)

    def batch(self):
        return dict(slab=self.dst, offsets=self.offsets, lens=self.lens)


def entries(count, csum, kind="vxlan", v6=False):
    e = np.zeros(count, schema.TUNNEL_ENTRY_DTYPE)
    e["kind"], e["ipver"] = schema.TUN_KIND[kind], 6 if v6 else 4
    e["flags"] = schema.TUN_F_UDP_CSUM if csum else 0
    e["id"] = np.arange(count) % (1 << 24)
    e["sport_lo"], e["sport_hi"] = 49152, 65535
    k = 16 if v6 else 4
    e["src"][:, :k] = np.arange(1, k + 1)
    e["dst"][:, :k] = 200
    e["dst"][:, k - 2] = np.arange(count) >> 8
    e["dst"][:, k - 1] = np.arange(count) & 255
    e["eth_dst"][:], e["eth_src"][:] = 2, 4
    return e


def mirrored(e):
    r = e.copy()
    r["src"], r["dst"] = e["dst"], e["src"]
    return r


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
             "measured": "a HIP event pair around every single queued call, outputs caller-sized and marshalled once, the "
                         "totals taken behind the second event; mean of the launches, min of 3 rounds"})
    c2 = torch.from_numpy(gen.gen_c2(n, seed=1).reshape(-1)).to(dev)
    big = np.zeros((n, 1504), np.uint8)
    pay = 1500 - 14 - 20 - 8
    hd = bytearray(bytes(range(1, 13)) + b"\x08\x00" + bytes([0x45, 0]) + (1500 - 14).to_bytes(2, "big") + bytes(4) + bytes([64, 17, 0, 0]) +
                   bytes([10, 0, 0, 1, 10, 0, 0, 2]) + (1000).to_bytes(2, "big") + (53).to_bytes(2, "big") + (8 + pay).to_bytes(2, "big") + b"\0\0")
    big[:, :len(hd)] = np.frombuffer(bytes(hd), np.uint8)
    big[:, len(hd):1500] = (np.arange(pay) * 7 % 251).astype(np.uint8)
    big[:, 30:34] = np.arange(n, dtype=np.uint32).view(np.uint8).reshape(n, 4)  # distinct destinations
    b1500 = torch.from_numpy(big.reshape(-1)).to(dev)
    del big
    ent = (torch.arange(n, device=dev, dtype=torch.int64) * 2654435761 % (1 << 32)).to(torch.uint32)
    draw = torch.randint(0, 65536, (n,), device=dev, dtype=torch.int64).to(torch.uint32)
    sources = {"c2": (dict(slab=c2, stride=64, n=n), 64, 64), "1500": (dict(slab=b1500, stride=1504, n=n, lens=torch.full((n,), 1500, dtype=torch.uint32, device=dev)), 1500, 1504)}
    chains, parsed = {}, {}
    for k, (b, _, stride) in sources.items():
        r = parsed[k] = P.parse(b["slab"], stride=stride, n=n, lens=b.get("lens"), columns=["chain"])
        chains[k] = {c: r[c] for c in ("n_hdrs", "hdr_type", "hdr_off")}
    cases = [("vxlan4_c2", "c2", entries(1, False), 0, 50, 4), ("vxlan4_c2_csum", "c2", entries(1, True), 0, 50, 4),
             ("vxlan4_c2_65536", "c2", entries(65536, False), draw, 50, 4), ("vxlan4_c2_65536_csum", "c2", entries(65536, True), draw, 50, 4),
             ("gre6_1500", "1500", entries(1, False, "gre", True), 0, 44, 2)]
    o50 = bytes(gen.reference_22_packets()[8].to_vec())[:50]
    enc_ops = [("insert", "Vxlan", o50[42:50]), ("insert", "UDP", o50[34:42]), ("insert", "IPv4", o50[14:34]), ("insert", "Ether", o50[0:14])]
    plain = {}
    for name, src, ents, tunnel, hl, add in cases:
        if a.trace_case and a.trace_case not in ("encap_" + name, "decap_" + name):
            continue
        batch, plen, stride = sources[src]
        chain = chains[src]
        rows = 3  # Ether / IPv4 / UDP
        tun, tun_back = P.tunnels(ents), P.tunnels(mirrored(ents))  # the other end's table takes the packets out again
        ol = plen + hl
        r16 = (ol + 15) // 16 * 16
        enc = Call(P, tun, "encap", batch, chain, n, n, n * r16, tunnel, ent)
        enc.queue()
        enc.take()
        assert enc.cnt.value == n and bool((enc.status == 0).all()), (name, enc.cnt.value)
        dec = Call(P, tun_back, "decap", enc.batch(), enc.out_chain, n, n, n * ((plen + 15) // 16 * 16))
        dec.queue()
        dec.take()
        assert dec.cnt.value == n and bool((dec.status == 0).all()), (name, dec.cnt.value, torch.bincount(dec.status.to(torch.int64)).tolist())
        back = dec.dst.view(n, -1)[:, :plen]
        assert torch.equal(back, batch["slab"].view(n, stride)[:, :plen]), (name, "decap(encap(x)) != x")
        for op, call, pin, pout, rin, rout in (("encap", enc, plen, r16, rows, rows + add), ("decap", dec, ol, (plen + 15) // 16 * 16, rows + add, rows)):
            if a.trace_case:
                if a.trace_case == op + "_" + name:
                    call.queue()
                    call.take()
                    call.queue()
                    call.take()
                    torch.cuda.synchronize()
                    return
                continue
            ms = min(each_ms(call.queue, it, call.take) for _ in range(3))
            rd = pin + 1 + 3 * max(4, rin) + (8 if op == "encap" else 0) + 32 + 3 * rin
            wr = 32 + pout + 17 + 3 * rout + (5 if op == "encap" else 9)
            ln = {"workload": f"{op}_{name}", "tunnels": len(ents), "in_bytes": pin, "out_bytes": pout if op == "decap" else ol,
                  "call_us": round(ms * 1e3, 2), "Gpkt/s": round(n / (ms * 1e-3) / 1e9, 3), "bytes_per_pkt": {"read": rd, "written": wr}}
            if src == "c2":
                if op == "encap":
                    dst = torch.zeros(n * 128, dtype=torch.uint8, device=dev)
                    eargs, _, ekeep = P._edit_args(batch["slab"], parsed[src], enc_ops, stride=64, dst=dst, slot=128)  # marshalled once, too
                    ems = min(each_ms(lambda: P._L.pkt_edit_batch(P._ctx, *eargs, P._stream(None)), it) for _ in range(3))
                    ln.update({"edit_insert_50_bytes_us": round(ems * 1e3, 2), "frac_of_edit": round(ms / ems, 3)})
                    if name == "vxlan4_c2":
                        e_dst, e_len, e_st, e_ch = P.edit(batch["slab"], parsed[src], enc_ops, stride=64, dst=dst, slot=128)
                        torch.cuda.synchronize()
                        plain["edit"] = (dst, e_ch)
                        mine = enc.dst.view(n, 128)[:4, :114].cpu().numpy()
                        theirs = dst.view(n, 128)[:4, :114].cpu().numpy()
                        ln["edit_output_differs_in_bytes"] = sorted(set(np.flatnonzero((mine != theirs).any(axis=0)).tolist()))[:24]
                    else:
                        del dst
                elif "edit" in plain:
                    e_dst, e_ch = plain["edit"]
                    ddst = torch.zeros(n * 64, dtype=torch.uint8, device=dev)
                    dargs, _, dkeep = P._edit_args(e_dst, e_ch, [("remove", 0)] * 4, stride=128, dst=ddst, slot=64)
                    ems = min(each_ms(lambda: P._L.pkt_edit_batch(P._ctx, *dargs, P._stream(None)), it) for _ in range(3))
                    ln.update({"edit_remove_x4_us": round(ems * 1e3, 2), "frac_of_edit": round(ms / ems, 3)})
                    del ddst
            if op == "encap" and name.endswith("_csum"):
                nocs = ents.copy()
                nocs["flags"] = 0
                tun2 = P.tunnels(nocs)
                two = Call(P, tun2, "encap", batch, chain, n, n, n * r16, tunnel, ent)
                ob = two.batch()

                def two_calls():
                    two.queue()
                    P.l4_checksum(two.dst, two.out_chain, which=0, update=True, offsets=ob["offsets"], lens=ob["lens"], n=n)
                two_calls()
                two.take()
                torch.cuda.synchronize()
                same = bool(torch.equal(two.dst, enc.dst))
                tms = min(each_ms(two_calls, it, two.take) for _ in range(3))
                ln.update({"encap_then_l4_checksum_update_us": round(tms * 1e3, 2), "frac_of_two_calls": round(ms / tms, 3),
                           "two_calls_output_equal": same})
                del two, tun2
            c = copy_ceiling(n, rd, wr, dev, it, ms)
            if c is not None:
                ln["stream_copy"] = c
            out(ln)
        del enc, dec, tun, tun_back
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
