#!/usr/bin/env python3
"""Measurements of the §8(f) kernels beside the hot path: one JSON line per workload.

  pktgen_clone   tests/lib.rs:770-776  pkt.clone().to_vec() of test_tcp_packet (154 B), n times
  pktgen_update  tests/lib.rs:778-787  set_etype(i % 0xFFFF), clone, to_vec
  pktgen_new     tests/lib.rs:762-768  every builder argument of test_tcp_packet varied per packet
                 (MACs, IPs, tos, ttl, id, ports, seq, ack: splitmix64) + the IPv4 checksum refresh
  pktgen_values  the same fields from per-packet value arrays (8 B read per field per packet)
  to_vec_c2 / to_vec_c4   PacketSlice::to_vec of every parsed packet (tests/lib.rs:790-817), C2 slab
                 and C4 pcap replay, into the input's layout; to_vec_c4_packed: the C4 outputs
                 packed back to back (dst_offsets = prefix of the lengths)
  pcap_write     pkt_pcap_write (tests/pcap.rs:7-37 as a batch operation), two lines: pcap_write_c2, the
                 C2 slab at fixed stride with every packet selected, and pcap_write_c4, an indexed batch
                 over a C4 capture with every record selected (the capture again); timed per call
  compare        pkt_compare_batch (Packet::compare, packet.rs:326-358, as a batch operation), five lines:
                 compare_c2, the C2 slab at fixed stride against an identical copy, and compare_pcap, the same
                 packets against their own pkt_pcap_write capture (an indexed b, misaligned by the 16-byte
                 record headers), each with no ignores and (_ign4) with 4 IPv4 fields ignored, and
                 compare_c2_rewritten_ign4, a copy that differs in those 4 fields in every packet; timed
                 per call; compare_c2 also beside the torch expression a user can write today
  edit           pkt_edit_batch (Packet::push / insert / pop / remove, packet.rs:117-164, then to_vec), five lines:
                 edit_identity_c2 (nops = 0 on C2, beside pkt_to_vec_batch on the same batch in the same run; and
                 _bytes_only, with the status, length and chain outputs NULL), edit_encap_c2 (VXLAN encap, 64 ->
                 114 bytes in 128-byte slots), edit_decap_c2 (the decap of that output through its out chain) and
                 edit_vlan_strip_c3 (the first tag of C3 removed, 128-byte slots to 128-byte slots)
  l4             pkt_l4_checksum_batch (the TCP / UDP / ICMP checksum with its pseudo-header, RFC 1071), four lines:
                 l4_verify_c2 / l4_update_c2 (the C2 slab at fixed stride, which = 0) and l4_verify_c4 / l4_update_c4
                 (an indexed batch over a C4 capture in place, which = PKT_L4_LAST), read-only and with PKT_L4_UPDATE
  extract_c2     every field of Ether/IPv4/UDP (19 specs, one launch) over C2 (headers.rs:195-201)
  setfields_c2   4 setters + the IPv4 checksum refresh, in place over C2 (headers.rs:315-324)

Each line: kernel time per launch (HIP events over back-to-back launches on one stream, outputs
from a >= 1 GiB ring), Gpkt/s, algorithmic bytes per packet (what the kernel must read + write),
roofline frac vs 8 TB/s, and the CPU restatement (oracle/) on a bounded sample with every core this
process may use.  Parity of each workload's output is checked against the oracle on a sample.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "packet-rs_amd"), os.path.join(REPO, "oracle"), REPO]
import pktgpu  # noqa: E402
from pktgpu import gen, pktgen, schema  # noqa: E402

PEAK = 8000.0  # GB/s, MI355X HBM3E spec


def host_cores():
    aff = len(os.sched_getaffinity(0))
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            return min(aff, max(1, int(int(q) / int(per))))
    except (OSError, ValueError):
        pass
    return aff


def timed(fn, budget):
    reps, t0 = 0, time.perf_counter()
    while reps < 1 or time.perf_counter() - t0 < budget:
        fn()
        reps += 1
    return reps, time.perf_counter() - t0


def prepared_extract(P, slab, chain, specs):
    """pkt_extract_fields over a fixed-stride (64 B) slab with its arguments built once."""
    import ctypes
    b = P._batch(slab, None, 64, None, None)
    ch = P._chain(chain)
    k = len(specs)
    sp = (P._lib.PktFieldSpec * k)()
    for j, (t, occ, s0, e0) in enumerate(specs):
        sp[j] = P._lib.PktFieldSpec(schema.HDR_ID[t] if isinstance(t, str) else int(t), occ, s0, e0, 0)
    vals = [torch.empty(b.n, dtype=torch.uint64, device=slab.device) for _ in range(k)]
    found = [torch.empty(b.n, dtype=torch.uint8, device=slab.device) for _ in range(k)]
    vp = (ctypes.c_void_p * k)(*[v.data_ptr() for v in vals])
    fp = (ctypes.c_void_p * k)(*[f.data_ptr() for f in found])
    args = (P._ctx, ctypes.byref(b), ctypes.byref(ch), sp, k, vp, fp, P._stream(None))
    keep = (b, ch, sp, vals, found, vp, fp)

    def launch():
        assert P._L.pkt_extract_fields(*args) == 0 and keep
    return launch


def event_ms(launch, iters, warm=3):
    s = torch.cuda.current_stream()
    for k in range(warm):
        launch(k)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(s)
    for k in range(iters):
        launch(k)
    b.record(s)
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


_PROBE = []


def copy_ceiling(n, read_b, write_b, dev, it, kernel_ms):
    """The no-work ceiling of a workload's byte shape (as the C2 line's
    roofline.ceiling.stream_copy): libpktprobe's hand-written streaming copy reading read_b and writing
    write_b bytes per packet (16-byte global_load/store_dwordx4 by consecutive lanes, 1 KiB contiguous
    per wave instruction, 4 loads in flight per lane), one launch per batch over a >= 1 GiB ring, HIP
    events on one stream.  `kernel_frac_of_copy` = copy time / the workload's kernel time."""
    import ctypes
    from bench import load_probe
    if not _PROBE:
        _PROBE.append(load_probe())
    L = _PROBE[0]
    if L is None:
        return None
    rb, wb = (int(read_b * n) + 15) // 16 * 16, (int(write_b * n) + 15) // 16 * 16
    per = max(rb, wb, 16)
    ring = max(2, (1 << 30) // per + 1)
    srcs = [torch.empty(max(rb, 16), dtype=torch.uint8, device=dev) for _ in range(min(ring, 8))]
    dsts = [torch.empty(max(wb, 16), dtype=torch.uint8, device=dev) for _ in range(ring)]
    P8 = ctypes.POINTER(ctypes.c_uint8)
    sp = [(P8 * 1)(ctypes.cast(ctypes.c_void_p(t.data_ptr()), P8)) for t in srcs]
    dp = [(P8 * 1)(ctypes.cast(ctypes.c_void_p(t.data_ptr()), P8)) for t in dsts]
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def launch(k):
        assert L.pkt_probe_stream_copy(sp[k % len(sp)], dp[k % ring], 1, rb, wb, st) == 0
    ms = min(event_ms(launch, it) for _ in range(3))
    del srcs, dsts
    torch.cuda.empty_cache()
    gbs = (rb + wb) / (ms * 1e-3) / 1e9
    return {"kernel": "pkt_probe_stream_copy (libpktprobe.so): the workload's read and written bytes, contiguous, "
                      "no work", "read_bytes": rb, "written_bytes": wb, "copy_us": round(ms * 1e3, 2),
            "copy_frac_of_peak": round(gbs / PEAK, 4), "kernel_frac_of_copy": round(ms / kernel_ms, 4),
            "measured": "min of 3 rounds of HIP events over back-to-back one-batch launches, same stream"}


def line(name, n, ms, read_b, write_b, cpu, extra=None):
    gbs = (read_b + write_b) * n / (ms * 1e-3) / 1e9
    d = {"workload": name, "packets": n, "kernel_us": round(ms * 1e3, 2), "Gpkt/s": round(n / (ms * 1e-3) / 1e9, 3),
         "algorithmic_bytes_per_pkt": {"read": read_b, "written": write_b},
         "roofline": {"bound": "hbm", "achieved": round(gbs, 1), "peak": PEAK, "unit": "GB/s",
                      "frac": round(gbs / PEAK, 4)},
         "cpu_baseline": cpu}
    if extra:
        d.update(extra)
    if CEILING[0]:
        c = copy_ceiling(n, read_b, write_b, torch.device("cuda", 0), 20, ms)
        if c is not None:
            d["roofline"]["ceiling"] = c
    print(json.dumps(d), flush=True)


CEILING = [True]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--cpu-budget", type=float, default=3.0)
    ap.add_argument("--only", default="")
    ap.add_argument("--no-ceiling", action="store_true", help="skip the streaming-copy ceiling of each line")
    args = ap.parse_args()
    CEILING[0] = not args.no_ceiling
    import oracle
    oracle.build()
    n, it = args.n, args.iters
    cores = host_cores()
    P = pktgpu.Parser(0)
    dev = P.torch_device
    only = set(args.only.split(",")) if args.only else None

    def want(name):
        return only is None or name in only

    # ---------------------------------------------------------------- pktgen
    tpl = pktgen.test_tcp_template()
    stride = 160
    ring = max(2, (1 << 30) // (n * stride) + 1)
    outs = [torch.empty(n * stride, dtype=torch.uint8, device=dev) for _ in range(ring)]
    cpu_n = 1 << 18
    cpu_out = np.zeros((cpu_n, stride), np.uint8)

    def cpu_loop(mode):
        r, t = timed(lambda: oracle.pktgen_loop(tpl, cpu_n, stride, mode, nthreads=cores, out=cpu_out), args.cpu_budget)
        return {"value": round(r * cpu_n / t / 1e9, 6), "unit": "Gpkt/s", "cores": cores, "kind": "port",
                "sample": f"{r} x {cpu_n} packets of oracle.pktgen_loop({mode}) (owned Packet: Box per header, "
                          f"Arc<Mutex> header bytes, Vec-grown to_vec), {cores} threads"}

    if want("pktgen_clone"):
        G = pktgen.Generator(P, tpl)
        ms = event_ms(lambda k: G.run(n, stride, dst=outs[k % ring]), it)
        got = G.run(4096, stride).cpu().numpy().reshape(4096, stride)
        ok = np.array_equal(got, oracle.pktgen_loop(tpl, 4096, stride, "clone"))
        line("pktgen_clone", n, ms, 0, stride, cpu_loop("clone"), {"parity_vs_oracle": bool(ok), "stride": stride})
    if want("pktgen_update"):
        G = pktgen.Generator(P, tpl, [pktgen.Field("Ether", "etype", kind="inc", count=0xFFFF)])
        ms = event_ms(lambda k: G.run(n, stride, dst=outs[k % ring]), it)
        got = G.run(70000, stride).cpu().numpy().reshape(70000, stride)
        ok = np.array_equal(got, oracle.pktgen_loop(tpl, 70000, stride, "update"))
        line("pktgen_update", n, ms, 0, stride, cpu_loop("update"), {"parity_vs_oracle": bool(ok), "stride": stride})
    names = [("Ether", "dst"), ("Ether", "src"), ("IPv4", "src"), ("IPv4", "dst"), ("IPv4", "diffserv"),
             ("IPv4", "ttl"), ("IPv4", "identification"), ("TCP", "src"), ("TCP", "dst"), ("TCP", "seq_no"),
             ("TCP", "ack_no")]
    for kind in ("random", "values"):
        name = "pktgen_new" if kind == "random" else "pktgen_values"
        if not want(name):
            continue
        fs = [pktgen.Field(h, f, kind=kind, base=1000 + j) for j, (h, f) in enumerate(names)]
        G = pktgen.Generator(P, tpl, fs, csum=[0])
        vals = {}
        if kind == "values":
            g = torch.Generator(device="cpu").manual_seed(5)
            vals = {j: torch.randint(0, 2**62, (n,), generator=g, dtype=torch.int64).to(torch.uint64).to(dev)
                    for j in range(len(fs))}
        ms = event_ms(lambda k: G.run(n, stride, values=vals, dst=outs[k % ring]), it)
        m = 8192
        got = G.run(m, stride, values=vals).cpu().numpy().reshape(m, stride)
        gi = np.arange(m, dtype=np.uint64)
        hv = [f.value(gi, vals[j][:m].cpu().numpy() if kind == "values" else None) for j, f in enumerate(fs)]
        slab = np.zeros((m, stride), np.uint8)
        slab[:, :len(tpl)] = np.frombuffer(tpl, np.uint8)
        slab = slab.reshape(-1)
        lens = np.full(m, len(tpl), np.uint32)
        chain = oracle.parse_batch(slab, m, stride=stride, lens=lens, columns=["status", "n_hdrs", "hdr_type", "hdr_off"])
        oracle.set_fields(slab, m, chain, [(f.hdr, 0, f.start, f.end) for f in fs], hv, stride=stride, lens=lens)
        oracle.ipv4_update_checksum(slab, m, chain, 0, stride=stride, lens=lens)
        ok = np.array_equal(got.reshape(-1), slab)
        line(name, n, ms, 8 * len(fs) if kind == "values" else 0, stride, None,
             {"parity_vs_oracle": bool(ok), "stride": stride, "fields": len(fs),
              "cpu_note": "the reference's 'new packet' loop runs the utils.rs builders (string parsing, "
                          "per-header allocation); no C restatement of the builders is timed"})
    del outs

    # ---------------------------------------------------------------- to_vec / extract / set_fields
    c2 = gen.gen_c2(n).reshape(-1)
    ring2 = max(2, (1 << 30) // c2.size + 1)
    slabs = [torch.from_numpy(c2).to(dev) for _ in range(min(ring2, 4))]
    chains = [P.parse(s, stride=64, columns=["chain"]) for s in slabs]
    torch.cuda.synchronize()
    if want("to_vec_c2"):
        dsts = [torch.empty_like(slabs[0]) for _ in range(ring2)]
        ms = event_ms(lambda k: P.to_vec(slabs[k % len(slabs)], chains[k % len(slabs)], stride=64,
                                         dst=dsts[k % ring2]), it)
        out, _ = P.to_vec(slabs[0], chains[0], stride=64)
        ok = np.array_equal(out.cpu().numpy(), c2)
        cpu_m = 1 << 18
        r, t = timed(lambda: oracle.round_trip_batch(c2[:cpu_m * 64], cpu_m, stride=64, slow=True, nthreads=cores),
                     args.cpu_budget)
        # read: the packet bytes + status/n_hdrs/3 slots (type+off)/payload_off/len; written: bytes + out_len
        line("to_vec_c2", n, ms, 64 + 1 + 1 + 3 * 3 + 4, 64 + 4,
             {"value": round(r * cpu_m / t / 1e9, 6), "unit": "Gpkt/s", "cores": cores, "kind": "port",
              "sample": f"{r} x {cpu_m} packets of oracle slow::parse(..).to_vec()"},
             {"parity_vs_oracle": bool(ok)})
        del dsts
    if want("to_vec_c4"):
        s4, o4, l4 = gen.gen_c4(n)
        d4, do4, dl4 = torch.from_numpy(s4).to(dev), torch.from_numpy(o4).to(dev), torch.from_numpy(l4).to(dev)
        ch4 = P.parse(d4, offsets=do4, lens=dl4, columns=["chain"])
        dsts = [torch.empty_like(d4) for _ in range(max(2, (1 << 30) // s4.size + 1))]
        ms = event_ms(lambda k: P.to_vec(d4, ch4, offsets=do4, lens=dl4, dst=dsts[k % len(dsts)]), it)
        out, ln = P.to_vec(d4, ch4, offsets=do4, lens=dl4)
        want_b, wl = oracle.round_trip_batch(s4, n, offsets=o4, lens=l4, slow=True, nthreads=cores)
        o = out.cpu().numpy()
        mask = np.zeros(s4.size, bool)
        for t_, L_ in zip(o4[:20000], wl[:20000]):
            mask[int(t_):int(t_) + int(L_)] = True
        ok = np.array_equal(ln.cpu().numpy(), wl) and np.array_equal(o[mask], want_b[mask])
        avg = float(l4.mean())
        nh = int(np.asarray(ch4["n_hdrs"].cpu().numpy(), np.int64).mean() + 0.5)
        cpu_m = 1 << 17
        r, t = timed(lambda: oracle.round_trip_batch(s4, cpu_m, offsets=o4[:cpu_m], lens=l4[:cpu_m], slow=True,
                                                     nthreads=cores), args.cpu_budget)
        line("to_vec_c4", n, ms, round(avg + 8 + 4 + 1 + 1 + 3 * nh + 4, 1), round(avg + 4, 1),
             {"value": round(r * cpu_m / t / 1e9, 6), "unit": "Gpkt/s", "cores": cores, "kind": "port",
              "sample": f"{r} x {cpu_m} records of oracle slow::parse(..).to_vec()"},
             {"parity_vs_oracle_first_20000": bool(ok), "avg_record_bytes": round(avg, 1)})
        # the same records packed back to back (dst_offsets = prefix of the lengths: each to_vec
        # output Vec in a contiguous packet buffer, no pcap record headers between them)
        po = np.zeros(n, np.uint64)
        po[1:] = np.cumsum(l4[:-1].astype(np.uint64))
        tot = int(po[-1]) + int(l4[-1])
        dpo = torch.from_numpy(po).to(dev)
        dstp = [torch.empty(((tot + 15) // 16) * 16, dtype=torch.uint8, device=dev)
                for _ in range(max(2, (1 << 30) // tot + 1))]
        ms = event_ms(lambda k: P.to_vec(d4, ch4, offsets=do4, lens=dl4, dst=dstp[k % len(dstp)], dst_offsets=dpo), it)
        outp, lnp = P.to_vec(d4, ch4, offsets=do4, lens=dl4, dst=dstp[0], dst_offsets=dpo)
        op = outp.cpu().numpy()
        okp = np.array_equal(lnp.cpu().numpy(), wl) and all(
            np.array_equal(op[int(po[j]):int(po[j]) + int(wl[j])], want_b[int(o4[j]):int(o4[j]) + int(wl[j])])
            for j in range(0, n, max(1, n // 20000)))
        line("to_vec_c4_packed", n, ms, round(avg + 8 + 8 + 4 + 1 + 1 + 3 * nh + 4, 1), round(avg + 4, 1),
             {"value": round(r * cpu_m / t / 1e9, 6), "unit": "Gpkt/s", "cores": cores, "kind": "port",
              "sample": f"{r} x {cpu_m} records of oracle slow::parse(..).to_vec()"},
             {"parity_vs_oracle_sampled": bool(okp), "avg_record_bytes": round(avg, 1),
              "dst": "packed: dst_offsets = prefix of the lengths"})
        del dstp
        del dsts, d4
    if want("pcap_write"):
        import ctypes

        def write_ms(slab, total, **kw):
            """GPU time of one pkt_pcap_write_async call (its four kernels), HIP events around each
            call, the result taken (one write in flight per ctx) before the next; the arguments are
            marshalled before the first event.  Destinations from a >= 1 GiB ring."""
            ring_w = max(2, (1 << 30) // total + 1)
            dsts = [torch.empty(total, dtype=torch.uint8, device=dev) for _ in range(ring_w)]
            nn = kw["offsets"].numel() if kw.get("offsets") is not None else slab.numel() // kw["stride"]
            rec = (torch.empty(nn, dtype=torch.uint64, device=dev), torch.empty(nn, dtype=torch.uint32, device=dev),
                   torch.empty(nn, dtype=torch.uint32, device=dev))
            b = P._batch(slab, None, kw.get("stride"), kw.get("offsets"), kw.get("lens"))
            s, tb, tn = P._stream(None), ctypes.c_uint64(), ctypes.c_uint64()
            evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(it)]
            cur = torch.cuda.current_stream()
            for k in range(-3, it):
                if k >= 0:
                    evs[k][0].record(cur)
                rc = P._L.pkt_pcap_write_async(P._ctx, ctypes.byref(b), None, 0, 0, 0, None, None,
                                               dsts[k % ring_w].data_ptr(), total, rec[0].data_ptr(), rec[1].data_ptr(),
                                               rec[2].data_ptr(), s)
                if k >= 0:
                    evs[k][1].record(cur)
                assert rc == 0 and P._L.pkt_pcap_write_result(P._ctx, ctypes.byref(tb), ctypes.byref(tn)) == 0
                assert tb.value == total and tn.value == nn
            torch.cuda.synchronize()
            t = sorted(a.elapsed_time(z) for a, z in evs)
            return sum(t) / len(t), t[len(t) // 2], t[0]

        def write_cpu(slab_h, m, **kw):
            r, t = timed(lambda: pktgpu.pcap_write(slab_h, **kw), args.cpu_budget)
            return {"value": round(r * m / t / 1e9, 6), "unit": "Gpkt/s", "cores": 1, "kind": "port",
                    "sample": f"{r} x {m} packets of pkt_pcap_write_host (the CPU model: a header and a memcpy per "
                              "record, tests/pcap.rs:26-36), 1 thread"}

        how = {"measured": "mean over the iterations of HIP events around ONE call's four kernels (reduce, scan, "
                           "emit, copy), the write's result taken between calls; dst from a >= 1 GiB ring"}
        # (a) the C2 slab, fixed stride, every packet: 64 B read; 16 + 64 B of file and the record table written
        tot2 = 24 + n * 80
        ms, med, best = write_ms(slabs[0], tot2, stride=64)
        cap, m_, o_, l_, s_ = P.pcap_write(slabs[0], stride=64)
        ok = cap[:24 + 4096 * 80].cpu().numpy().tobytes() == gen.pcap_bytes([c2[64 * i:64 * i + 64].tobytes() for i in range(4096)])
        ok = ok and m_ == n and cap.numel() == tot2 and bool((s_.cpu().numpy() == np.arange(n)).all())
        cpu_m = 1 << 18
        line("pcap_write_c2", n, ms, 64, 80 + 16, write_cpu(c2[:cpu_m * 64], cpu_m, stride=64),
             dict(how, parity_vs_struct_pack_first_4096=bool(ok), capture_bytes=tot2,
                  median_us=round(med * 1e3, 2), min_us=round(best * 1e3, 2)))
        del cap
        # (b) an indexed batch over a C4 capture, every record: the capture again
        s4, o4, l4 = gen.gen_c4(n)
        d4, do4, dl4 = torch.from_numpy(s4).to(dev), torch.from_numpy(o4).to(dev), torch.from_numpy(l4).to(dev)
        ms, med, best = write_ms(d4, s4.size, offsets=do4, lens=dl4)
        cap, m_, o_, l_, s_ = P.pcap_write(d4, offsets=do4, lens=dl4)
        ok = m_ == n and bool(torch.equal(cap, d4)) and np.array_equal(o_.cpu().numpy(), o4)
        avg = float(l4.mean())
        cpu_m = 1 << 17
        line("pcap_write_c4", n, ms, round(avg + 8 + 4, 1), round(avg + 16 + 16, 1),
             write_cpu(s4, cpu_m, offsets=o4[:cpu_m], lens=l4[:cpu_m]),
             dict(how, parity_reproduces_the_capture=bool(ok), capture_bytes=int(s4.size), avg_record_bytes=round(avg, 1),
                  median_us=round(med * 1e3, 2), min_us=round(best * 1e3, 2)))
        del cap, d4
    if want("compare"):
        import ctypes
        from pktgpu import fields as F
        ign4 = [("IPv4", 0) + tuple(F.FIELDS[schema.HDR_ID["IPv4"]][f])
                for f in ("identification", "ttl", "header_checksum", "diffserv")]
        # a ring of 4 (a, b) pairs: 512 MiB or more read before a pair comes round again
        caps = [P.pcap_write(s_, stride=64) for s_ in slabs]
        copies = [s_.clone() for s_ in slabs]
        outs3 = (torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint32, device=dev),
                 torch.empty(n, dtype=torch.uint32, device=dev))

        def compare_ms(bs, ignore):
            """GPU time of one pkt_compare_batch_async call (the compare kernel and the summary's
            copy-out), HIP events around each call, the result taken (one compare in flight per ctx)
            before the next; the arguments are marshalled before the first event."""
            sp, k = pktgpu._cmp_specs(P._lib, ignore)
            pa = [P._batch(s_, None, 64, None, None) for s_ in slabs]
            pb = [P._batch(*x) for x in bs]
            chs = [P._chain(c_) for c_ in chains]
            s, sm = P._stream(None), P._lib.PktCmpSummary()
            evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(it)]
            cur = torch.cuda.current_stream()
            for j in range(-3, it):
                r = j % len(slabs)
                if j >= 0:
                    evs[j][0].record(cur)
                rc = P._L.pkt_compare_batch_async(P._ctx, ctypes.byref(pa[r]), ctypes.byref(pb[r]),
                                                  ctypes.byref(chs[r]) if k else None, sp, k, outs3[0].data_ptr(),
                                                  outs3[1].data_ptr(), outs3[2].data_ptr(), s)
                if j >= 0:
                    evs[j][1].record(cur)
                assert rc == 0 and P._L.pkt_compare_result(P._ctx, ctypes.byref(sm)) == 0
                assert (sm.n_equal, sm.n_len, sm.n_bytes, sm.first_bad) == (n, 0, 0, n)
            torch.cuda.synchronize()
            ok = bool((outs3[0] == 0).all()) and bool((outs3[1] == 64).all()) and bool((outs3[2] == 64).all())
            t = sorted(a.elapsed_time(z) for a, z in evs)
            return sum(t) / len(t), t[len(t) // 2], t[0], ok

        cpu_m = 1 << 18
        ha = dict(slab=c2[:cpu_m * 64], stride=64)
        r, t = timed(lambda: pktgpu.compare(ha, ha), args.cpu_budget)
        cpu = {"value": round(r * cpu_m / t / 1e9, 6), "unit": "Gpkt/s", "cores": 1, "kind": "port",
               "sample": f"{r} x {cpu_m} pairs of pkt_compare_host (the CPU model: the reference's zip/filter/count, "
                         "packet.rs:347), 1 thread"}
        how = {"measured": "mean over the iterations of HIP events around ONE call's two kernels (compare, summary "
                           "copy-out), the result taken between calls; a ring of 4 (a, b) pairs",
               "all_equal": "every pair EQUAL, matching = first_diff = 64, checked on the device"}
        # the torch expression for the fixed-stride, same-length case, same ring, same run
        tms = event_ms(lambda k_: (slabs[k_ % len(slabs)].view(n, 64) == copies[k_ % len(slabs)].view(n, 64)).sum(1), it)
        # the ignores at work: copies whose 6 bytes of the 4 ignored fields differ in every packet (a device
        # under test that rewrites them), still EQUAL under the ignores; masks are built only for chunks
        # that hold a difference, so the identical copies above do not pay for them
        rewritten = [c_.clone() for c_ in copies]
        for c_ in rewritten:
            c_.view(n, 64)[:, [15, 18, 19, 22, 24, 25]] ^= 0x55
        shapes = (("c2", [(c_, None, 64, None, None) for c_ in copies], 0, (("", []), ("_ign4", ign4))),
                  ("pcap", [(c_[0], None, None, c_[2], c_[3]) for c_ in caps], 8 + 4, (("", []), ("_ign4", ign4))),
                  ("c2_rewritten", [(c_, None, 64, None, None) for c_ in rewritten], 0, (("_ign4", ign4),)))
        for tag, bs, idx_b, runs in shapes:
            for sfx, ignore in runs:
                ms, med, best, ok = compare_ms(bs, ignore)
                extra = dict(how, parity_all_equal=ok, median_us=round(med * 1e3, 2), min_us=round(best * 1e3, 2),
                             ignores=len(ignore))
                if tag == "c2":
                    extra["torch_baseline"] = {"expr": "(A.view(n, 64) == B.view(n, 64)).sum(1)", "us": round(tms * 1e3, 2),
                                               "kernel_speedup_vs_torch": round(tms / ms, 3)}
                # read: la + lb, b's offsets / lens when indexed, with ignores n_hdrs and 3 slots of the chain;
                # written: result, matching, first_diff
                line(f"compare_{tag}{sfx}", n, ms, 128 + idx_b + (1 + 3 * 3 if ignore else 0), 9, cpu, extra)
        del caps, copies, rewritten
    if want("l4"):
        T4, T6 = schema.HDR_ID["IPv4"], schema.HDR_ID["IPv6"]
        L4T = [schema.HDR_ID[k] for k in ("ICMP", "TCP", "UDP")]

        def l4_lines(tag, bufs, dkw, hslab, hkw, which, chs, idx_b):
            """l4_verify_<tag> and l4_update_<tag>: kernel time of pkt_l4_checksum_batch over a ring of copies of
            the batch, its arguments marshalled once per copy; parity of the three outputs and of the updated
            slab against pkt_l4_checksum_host over the whole batch."""
            hch = {k: chs[0][k].cpu().numpy() for k in ("n_hdrs", "hdr_type", "hdr_off")}
            twin = pktgpu.l4_checksum(hslab, hch, which, **hkw)
            summed = twin["status"] <= schema.L4_UNCHECKED
            # the bytes a summed packet's checksum needs: its segment, the IP header's length, fragment and
            # address bytes, the chain (n_hdrs and its slots), the index when there is one
            isl4 = np.isin(hch["hdr_type"], L4T) & (np.arange(schema.MAX_HDRS)[:, None] < hch["n_hdrs"][None, :])
            pick = np.where(isl4.any(0), schema.MAX_HDRS - 1 - np.argmax(isl4[::-1], axis=0), 0) if which == schema.L4_LAST \
                else np.argmax(isl4, axis=0)
            cols = np.arange(hch["n_hdrs"].size)
            s_off = hch["hdr_off"][pick, cols].astype(np.int64)
            ipt = hch["hdr_type"][np.maximum(pick, 1) - 1, cols]
            plen = hkw["lens"].astype(np.int64) if hkw.get("lens") is not None else np.full(cols.size, hkw["stride"], np.int64)
            # (the segment's end taken as the packet's end, as it is for all but a few C4 templates)
            seg = np.where(summed, plen - s_off + np.where(ipt == T4, 12, np.where(ipt == T6, 34, 0)), 0)
            read_b = round(float(seg.mean()) + 1 + 3 * float(np.minimum(hch["n_hdrs"], schema.MAX_HDRS).mean()) + idx_b, 1)
            sample = min(n, 1 << 18)
            if hkw.get("offsets") is not None:
                ckw = dict(offsets=hkw["offsets"][:sample], lens=hkw["lens"][:sample])
            else:
                ckw = dict(stride=hkw["stride"], n=sample)
            cch = {k: np.ascontiguousarray(v[..., :sample]) for k, v in hch.items()}
            r, t = timed(lambda: pktgpu.l4_checksum(hslab, cch, which, **ckw), args.cpu_budget)
            cpu = {"value": round(r * sample / t / 1e9, 6), "unit": "Gpkt/s", "cores": 1, "kind": "port",
                   "sample": f"{r} x {sample} packets of pkt_l4_checksum_host (the CPU model: a big-endian word loop "
                             "over pseudo-header and segment), 1 thread"}
            for upd in (False, True):
                work = [b_.clone() for b_ in bufs] if upd else bufs
                prep = [P._l4_args(w_, c_, which, upd, **bkw)
                        for w_, c_, bkw in zip(work, chs, dkw)]
                s = P._stream(None)

                def launch(k_):
                    assert P._L.pkt_l4_checksum_batch(P._ctx, *prep[k_ % len(prep)][0], s) == 0
                ms = min(event_ms(launch, it) for _ in range(3))
                got = {k: v.cpu().numpy() for k, v in zip(("calc", "stored", "status"), prep[0][1])}
                if upd:  # after the first update the field holds calc: the outputs of the later launches
                    ok = np.array_equal(got["calc"], twin["calc"]) and np.array_equal(got["stored"][summed], twin["calc"][summed])
                    hs = hslab.copy()
                    pktgpu.l4_checksum(hs, hch, which, True, **hkw)
                    ok = ok and np.array_equal(work[0].cpu().numpy().reshape(-1), hs.reshape(-1))
                else:
                    ok = all(np.array_equal(got[k], twin[k]) for k in got)
                hist = {schema.L4_STATUS[k]: int((twin["status"] == k).sum()) for k in range(7) if (twin["status"] == k).any()}
                line(f"l4_{'update' if upd else 'verify'}_{tag}", n, ms, read_b, 5 + (2 * float(summed.mean()) if upd else 0), cpu,
                     {"parity_vs_host_twin": bool(ok), "which": which, "status_counts": hist,
                      "measured": "min of 3 rounds of HIP events over back-to-back launches, one stream, a ring of "
                                  f"{len(work)} copies of the batch, arguments marshalled once"})
                del work, prep

        l4_lines("c2", slabs, [dict(stride=64) for _ in slabs], c2, dict(stride=64), 0, chains, 0)
        s4, o4, l4 = gen.gen_c4(n)
        d4 = [torch.from_numpy(s4).to(dev) for _ in range(min(4, max(2, (1 << 30) // s4.size + 1)))]
        do4, dl4 = torch.from_numpy(o4).to(dev), torch.from_numpy(l4).to(dev)
        ch4 = [P.parse(d_, offsets=do4, lens=dl4, columns=["chain"]) for d_ in d4]
        torch.cuda.synchronize()
        l4_lines("c4", d4, [dict(offsets=do4, lens=dl4) for _ in d4], s4, dict(offsets=o4, lens=l4), schema.L4_LAST, ch4, 8 + 4)
        del d4, ch4
    if want("edit"):
        import ctypes
        CH = ("status", "n_hdrs", "hdr_type", "hdr_off", "payload_off", "payload_len")

        def edit_line(name, srcs, parsed, ops, stride, slot, what, outputs=(True, True, True), beside=None):
            """One pkt_edit_batch line: srcs / parsed = a ring of source slabs (fixed `stride`) and their chain
            columns, the destinations a >= 1 GiB ring of n * slot bytes; the arguments marshalled once per
            ring slot.  Returns the last ring slot's outputs (dst, out_len, status, chain)."""
            ringd = max(2, (1 << 30) // (n * slot) + 1)
            dsts = [torch.empty(n * slot, dtype=torch.uint8, device=dev) for _ in range(ringd)]
            prep = [P._edit_args(srcs[r % len(srcs)], parsed[r % len(srcs)], ops, stride=stride, dst=dsts[r], slot=slot,
                                 outputs=outputs) for r in range(ringd)]
            s = P._stream(None)

            def launch(k):
                assert P._L.pkt_edit_batch(P._ctx, *prep[k % ringd][0], s) == 0
            ms = event_ms(launch, it)
            # parity with the host model (pkt_edit_host) on a sample, and the bytes the line moves
            m = 1 << 14
            dst, ln, st, ch = prep[0][1]
            hp = {c_: np.ascontiguousarray(parsed[0][c_].cpu().numpy()[..., :m]) for c_ in CH}
            hsrc = srcs[0][:m * stride].cpu().numpy()
            hd, hl, hs, hc = pktgpu.edit(hsrc, hp, ops, stride=stride, slot=slot)
            ok = np.array_equal(dst[:m * slot].cpu().numpy().reshape(m, slot)[np.arange(slot)[None, :] < hl[:, None]],
                                hd.reshape(m, slot)[np.arange(slot)[None, :] < hl[:, None]])
            if ln is not None:
                ok = ok and np.array_equal(ln.cpu().numpy()[:m], hl) and np.array_equal(st.cpu().numpy()[:m], hs)
                ok = ok and all(np.array_equal(ch[c_].cpu().numpy()[:m], hc[c_]) for c_ in ("n_hdrs", "payload_off", "hdr_mask"))
            nh_in = float(parsed[0]["n_hdrs"].float().mean())
            out_b = float(hl.mean())
            nh_out = float(hc["n_hdrs"].mean())
            src_b = float(np.minimum(hl, stride).mean()) if name != "edit_encap_c2" else 64.0
            # read: the source bytes that reach the output + status, n_hdrs, payload_off / len and the used slot rows;
            # written: the output bytes + (with outputs) out_len, edit_status and the seven chain columns' used rows
            read_b = src_b + 6 + 3 * nh_in
            write_b = out_b + ((4 + 1 + 10 + 3 * nh_out) if outputs[0] else 0)
            r_, t_ = timed(lambda: pktgpu.edit(hsrc, hp, ops, stride=stride, slot=slot), args.cpu_budget / 2)
            cpu = {"value": round(r_ * m / t_ / 1e9, 6), "unit": "Gpkt/s", "cores": 1, "kind": "port",
                   "sample": f"{r_} x {m} packets of pkt_edit_host (the CPU model), 1 thread"}
            extra = {"parity_vs_host_model": bool(ok), "what": what, "ops": len(ops), "slot": slot,
                     "mean_out_len": round(out_b, 2), "outputs": "out_len, edit_status, out_chain" if outputs[0] else "bytes only"}
            if beside:
                extra["beside"] = dict(beside, edit_over_it=round(ms * 1e3 / beside["us"], 3))
            line(name, n, ms, round(read_b, 2), round(write_b, 2), cpu, extra)
            res = prep[ringd - 1][1]
            del dsts, prep
            return res

        # (a) nops = 0 on C2, beside pkt_to_vec_batch on the same batch in the same run
        tvd = [torch.empty_like(slabs[0]) for _ in range(ring2)]
        tv_ms = event_ms(lambda k: P.to_vec(slabs[k % len(slabs)], chains[k % len(slabs)], stride=64, dst=tvd[k % ring2]), it)
        del tvd
        tv = {"kernel": "pkt_to_vec_batch, same slabs and chains, same run (its Python wrapper marshals per call)",
              "us": round(tv_ms * 1e3, 2)}
        edit_line("edit_identity_c2", slabs, chains, [], 64, 64, "nops = 0: to_vec of C2 into 64-byte slots", beside=tv)
        edit_line("edit_identity_c2_bytes_only", slabs, chains, [], 64, 64, "the same with out_len, edit_status and out_chain NULL",
                  outputs=(False, False, False), beside=tv)
        # (c) VXLAN encap of C2: 64 bytes -> 114 in 128-byte slots; (d) decap of its output with its out chain
        o50 = bytes(gen.reference_22_packets()[8].to_vec())[:50]
        enc = [("insert", "Vxlan", o50[42:50]), ("insert", "UDP", o50[34:42]), ("insert", "IPv4", o50[14:34]),
               ("insert", "Ether", o50[0:14])]
        e_dst, e_len, e_st, e_ch = edit_line("edit_encap_c2", slabs, chains, enc, 64, 128,
                                             "VXLAN encap of C2: Vxlan, UDP, IPv4, Ether inserted at index 0, 64 -> 114 bytes")
        edit_line("edit_decap_c2", [e_dst], [e_ch], [("remove", 0)] * 4, 128, 128,
                  "decap of edit_encap_c2's output through its out chain (no second parse): remove(0) x 4, 114 -> 64 bytes")
        del e_dst, e_len, e_st, e_ch
        # (b) strip the first VLAN tag of C3, 128-byte slots to 128-byte slots
        c3 = torch.from_numpy(gen.gen_c3(n).reshape(-1)).to(dev)
        ch3 = P.parse(c3, stride=128, columns=["chain"])
        edit_line("edit_vlan_strip_c3", [c3], [ch3], [("remove_hdr", "Vlan", 0)], 128, 128,
                  "remove_hdr Vlan 0 on C3 (0-2 tags, a third each): untagged packets copied whole")
        del c3, ch3
    if want("extract_c2"):
        from pktgpu import fields as F
        specs = [(h, 0, s0, e0) for h in ("Ether", "IPv4", "UDP") for (s0, e0) in F.FIELDS[schema.HDR_ID[h]].values()]
        # ctypes arguments and output columns built once per ring slot: the Python wrapper's per-call
        # argument marshalling and 38 output allocations take longer than the kernel
        prep = [prepared_extract(P, slabs[r], chains[r], specs) for r in range(len(slabs))]
        ms = event_ms(lambda k: prep[k % len(prep)](), it)
        vals, found = P.extract_fields(slabs[0], chains[0], specs, stride=64)
        m = 1 << 16
        ch_h = {k: np.ascontiguousarray(v.cpu().numpy()[..., :m]) for k, v in chains[0].items()}
        spec_ids = [(schema.HDR_ID[h], o, s0, e0) for h, o, s0, e0 in specs]
        wv, _ = oracle.extract_fields(c2[:m * 64], m, ch_h, spec_ids, stride=64)
        ok = all(np.array_equal(vals[j].cpu().numpy()[:m], wv[j]) for j in range(len(specs)))
        r, t = timed(lambda: oracle.extract_fields(c2[:m * 64], m, ch_h, spec_ids, stride=64), args.cpu_budget)
        # read: 64 B window (the headers) + n_hdrs + 3 slots; written: 8 B value + 1 B found per spec
        line("extract_c2", n, ms, 64 + 1 + 9, 9 * len(specs),
             {"value": round(r * m / t / 1e9, 6), "unit": "Gpkt/s", "cores": 1, "kind": "port",
              "sample": f"{r} x {m} packets x {len(specs)} getters, oracle per-bit bit_range, 1 thread"},
             {"parity_vs_oracle": bool(ok), "specs": len(specs)})
    if want("setfields_c2"):
        fs = [("Ether", 0, 0, 47), ("IPv4", 0, 64, 71), ("IPv4", 0, 96, 127), ("UDP", 0, 0, 15)]
        g = torch.Generator(device="cpu").manual_seed(9)
        vals = [torch.randint(0, 2**62, (n,), generator=g, dtype=torch.int64).to(torch.uint64).to(dev) for _ in fs]

        def launch(k):
            s = slabs[k % len(slabs)]
            # setters + checksum refresh in one launch (pkt_set_fields_csum)
            P.set_fields(s, chains[k % len(slabs)], fs, vals, stride=64, ipv4_checksum=0)
        ms = event_ms(launch, it)
        m = 1 << 16
        s_cpu = c2[:m * 64].copy()
        ch_h = {k: np.ascontiguousarray(v.cpu().numpy()[..., :m]) for k, v in chains[0].items()}
        spec_ids = [(schema.HDR_ID[h], o, s0, e0) for h, o, s0, e0 in fs]
        vh = [v.cpu().numpy()[:m] for v in vals]
        oracle.set_fields(s_cpu, m, ch_h, spec_ids, vh, stride=64)
        oracle.ipv4_update_checksum(s_cpu, m, ch_h, 0, stride=64)
        ok = np.array_equal(slabs[0].cpu().numpy()[:m * 64], s_cpu)

        def cpu():
            s2 = c2[:m * 64].copy()
            oracle.set_fields(s2, m, ch_h, spec_ids, vh, stride=64)
            oracle.ipv4_update_checksum(s2, m, ch_h, 0, stride=64)
        r, t = timed(cpu, args.cpu_budget)
        # read: the 4 values + chain (n_hdrs + 3 slots) + the header lines touched; written: the fields
        line("setfields_c2 (+ipv4 checksum)", n, ms, 32 + 1 + 9 + 64, 64,
             {"value": round(r * m / t / 1e9, 6), "unit": "Gpkt/s", "cores": 1, "kind": "port",
              "sample": f"{r} x {m} packets x 4 setters + checksum, oracle per-bit set_bit_range, 1 thread"},
             {"parity_vs_oracle": bool(ok), "launches_per_step": 1})


if __name__ == "__main__":
    main()
