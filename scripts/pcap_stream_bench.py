#!/usr/bin/env python3
"""pkt_pcap_stream_* (a capture that arrives as it is produced: north_star's NIC ring / growing file) by
push size: a C4 capture in pinned host memory pushed in pieces of `push` bytes (each push returns once
its bytes have landed on the device, so the caller can reuse its ring slot), a step per `step_bytes` of
new bytes (0 = the 4 MiB default), finish; wall clock from the first push to finish's return, median
of reps.  Columns on the device (`dev`) or in pinned host memory (`pinned`: each step's columns
exported over the link).  One JSON line per row; the record count is checked against the generator's.

--ring: the same capture through a WINDOW smaller than the file (pkt_pcap_stream_release): max_bytes of
--windows (32 and 128 MiB), pushes of --ring-pushes (1 and 16 MiB); when room() is short of the next push
the consumer polls and releases everything polled.  Each row carries the number of releases and the
mean poll and release times, and `vs_whole`: its time over that of the unchanged whole-capture stream
(max_bytes >= the file, no release) with the same pushes, timed in the same run."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "packet-rs_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pushes", default="65536,1048576,16777216")
    ap.add_argument("--step-bytes", type=int, default=0)
    ap.add_argument("--ring", action="store_true")
    ap.add_argument("--windows", default=f"{32 << 20},{128 << 20}")
    ap.add_argument("--ring-pushes", default=f"{1 << 20},{16 << 20}")
    a = ap.parse_args()
    import torch  # noqa: F401  (the device columns are torch tensors)
    import pktgpu
    from pktgpu import gen
    from pktgpu.stream import PcapStream
    buf, offs, lens = gen.gen_c4(a.records, seed=0x5EED0007)
    n = a.records
    P = pktgpu.Parser(0)
    hb = P.host_empty((buf.size,), np.uint8)
    hb[:] = buf
    if a.ring:
        ring(a, hb, n)
        P.close()
        return
    for out in ("dev", "pinned"):
        st = PcapStream(0, max_bytes=buf.size + 64, cap=n, columns="all", out=None if out == "dev" else "pinned",
                        step_bytes=a.step_bytes)
        st.close()  # the buffers are allocated; each rep opens its own stream (a fresh capture)
        for push in (int(x) for x in a.pushes.split(",")):
            ts = []
            for _ in range(a.reps):
                st = PcapStream(0, max_bytes=buf.size + 64, cap=n, columns="all",
                                out=None if out == "dev" else "pinned", step_bytes=a.step_bytes)
                try:
                    t0 = time.perf_counter()
                    for p0 in range(0, buf.size, push):
                        st.push(hb[p0:p0 + push])
                    c, _ = st.finish(index=False)
                    ts.append(time.perf_counter() - t0)
                    assert c == n, (c, n)
                finally:
                    st.close()
            t = float(np.median(ts))
            print(json.dumps({"what": "pkt_pcap_stream", "columns": out, "push_bytes": push,
                              "step_bytes": a.step_bytes or (4 << 20), "records": n, "file_bytes": int(buf.size),
                              "ms": round(t * 1e3, 3), "Grecords_s": round(n / t / 1e9, 4),
                              "in_GBps": round(buf.size / t / 1e9, 2)}), flush=True)
    P.close()


def ring_once(hb, n, out, push, max_bytes, step_bytes):
    """One capture through a window of max_bytes (None: the whole file, no release) -> (seconds,
    releases, mean poll seconds, mean release seconds)."""
    from pktgpu.stream import PcapStream
    st = PcapStream(0, max_bytes=max_bytes or hb.size + 64, cap=n, columns="all",
                    out=None if out == "dev" else "pinned", step_bytes=step_bytes)
    try:
        tp, tr = [], []
        t0 = time.perf_counter()
        for p0 in range(0, hb.size, push):
            piece = hb[p0:p0 + push]
            while piece.size:
                if max_bytes and st.room() < piece.size:
                    t1 = time.perf_counter()
                    st.poll()
                    t2 = time.perf_counter()
                    st.release()
                    tr.append(time.perf_counter() - t2)
                    tp.append(t2 - t1)
                m = min(piece.size, st.room())  # (a push larger than the window goes in by the windowful)
                st.push(piece[:m])
                piece = piece[m:]
        c, _ = st.finish(index=False)
        t = time.perf_counter() - t0
        assert st.released()[0] + c == n, (st.released(), c, n)
        return t, len(tr), float(np.mean(tp)) if tp else 0.0, float(np.mean(tr)) if tr else 0.0
    finally:
        st.close()


def ring(a, hb, n):
    for out in ("dev", "pinned"):
        ring_once(hb, n, out, 16 << 20, None, a.step_bytes)  # the buffers are allocated
        for push in (int(x) for x in a.ring_pushes.split(",")):
            rows = []
            for mb in [None] + [int(x) for x in a.windows.split(",")]:
                runs = sorted(ring_once(hb, n, out, push, mb, a.step_bytes) for _ in range(a.reps))
                rows.append((mb,) + runs[len(runs) // 2])  # the median run by time
            whole = rows[0][1]
            for mb, t, nrel, tpoll, trel in rows:
                print(json.dumps({"what": "pkt_pcap_stream_ring" if mb else "pkt_pcap_stream_whole", "columns": out,
                                  "max_bytes": mb or int(hb.size + 64), "push_bytes": push,
                                  "step_bytes": a.step_bytes or (4 << 20), "records": n, "file_bytes": int(hb.size),
                                  "releases": nrel, "poll_ms_mean": round(tpoll * 1e3, 3),
                                  "release_ms_mean": round(trel * 1e3, 3), "ms": round(t * 1e3, 3),
                                  "in_GBps": round(hb.size / t / 1e9, 2), "vs_whole": round(t / whole, 3)}), flush=True)


if __name__ == "__main__":
    main()
