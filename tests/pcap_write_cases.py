"""Batches and expected captures shared by test_pcap_write_host.py and test_pcap_write_device.py.

A case is a dict of pkt_pcap_write's inputs over numpy arrays (slab, offsets / lens or stride, n,
select, snaplen, ts) and `expect(case)` builds the capture it must give with struct.pack, record by
record (tests/pcap.rs:7-37), never with the code under test: (bytes, rec_offsets, rec_lens, src_index).
"""
import os
import struct

import numpy as np

from pktgpu import gen

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def case(slab, offsets=None, lens=None, stride=None, n=None, select=None, snaplen=0, ts=(0, 0)):
    slab = np.ascontiguousarray(slab, np.uint8).reshape(-1)
    if n is None:
        n = len(offsets) if offsets is not None else slab.size // stride
    return dict(slab=slab, offsets=None if offsets is None else np.asarray(offsets, np.uint64),
                lens=None if lens is None else np.asarray(lens, np.uint32), stride=stride, n=int(n),
                select=None if select is None else np.asarray(select, np.uint8), snaplen=int(snaplen), ts=ts)


def expect(c):
    slab, n = c["slab"], c["n"]
    out = bytearray(gen.PCAP_GLOBAL_HEADER)
    offs, lens, src = [], [], []
    for i in range(n):
        if c["select"] is not None and not c["select"][i]:
            continue
        off = int(c["offsets"][i]) if c["offsets"] is not None else i * c["stride"]
        ln = int(c["lens"][i]) if c["lens"] is not None else c["stride"]
        ln = min(ln, max(0, slab.size - off), 65535)  # pkt_batch_t: clamped to the slab end and 65535
        incl = min(ln, c["snaplen"]) if c["snaplen"] else ln
        sec, usec = (t if isinstance(t, int) else int(t[i]) for t in c["ts"])
        out += struct.pack("<IIII", sec, usec, incl, ln)
        offs.append(len(out))
        lens.append(incl)
        src.append(i)
        out += slab[off:off + incl].tobytes()
    return bytes(out), np.array(offs, np.uint64), np.array(lens, np.uint32), np.array(src, np.uint32)


def golden():
    """ref22.pcap as an indexed batch over itself, with each record's own time."""
    buf = open(os.path.join(GOLD, "ref22.pcap"), "rb").read()
    offs, lens = gen.pcap_index_py(buf)
    sec = np.array([struct.unpack_from("<I", buf, int(o) - 16)[0] for o in offs], np.uint32)
    usec = np.array([struct.unpack_from("<I", buf, int(o) - 12)[0] for o in offs], np.uint32)
    return buf, case(np.frombuffer(buf, np.uint8), offs, lens, ts=(sec, usec))


EDGE_LENS = [0, 1, 2, 15, 16, 17, 31, 32, 33] + list(range(4055, 4101)) + [65535]


def edges(per_packet_ts=False, snaplen=0):
    """The length edges in one indexed batch: sources at odd offsets, out of order, the 4055..4100
    ones overlapping each other (1002 bytes apart) and the 65535 one, in a slab of random bytes."""
    rng = np.random.default_rng(11)
    slab = rng.integers(0, 256, 140000, dtype=np.uint8)
    offs = []
    for j, ln in enumerate(EDGE_LENS):
        if ln == 65535:
            offs.append(3)
        elif ln >= 4055:
            offs.append(70001 + 1002 * (4100 - ln))  # descending: unordered, overlapping
        else:
            offs.append(131073 + 202 * (9 - j))
    assert all(o % 2 == 1 for o in offs) and max(o + ln for o, ln in zip(offs, EDGE_LENS)) <= slab.size
    n = len(offs)
    ts = (1700000000, 999999)
    if per_packet_ts:
        ts = (rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32),
              rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32))
    return case(slab, offs, EDGE_LENS, ts=ts, snaplen=snaplen)


SELECT_N = 5000


def select_masks():
    n = SELECT_N
    every3 = (np.arange(n) % 3 == 0)
    first = np.zeros(n, bool)
    first[0] = True
    last = np.zeros(n, bool)
    last[-1] = True
    gap = np.ones(n, bool)
    gap[1000:4000] = False
    return {"all": np.ones(n, bool), "none": np.zeros(n, bool), "every_third": every3, "first": first,
            "last": last, "gap_3000": gap}


def select_case(name):
    slab = gen.gen_c2(SELECT_N, seed=5)
    return case(slab, stride=64, select=select_masks()[name], ts=(7, 8))


def clamped():
    """Packets running past slab_len (written with the clamped length) and slots starting at or past
    the end (empty records), indexed; and the same in a fixed-stride batch whose n passes the slab."""
    rng = np.random.default_rng(13)
    slab = rng.integers(0, 256, 1000, dtype=np.uint8)
    indexed = case(slab, [10, 900, 1000, 5000, 999, 0], [50, 200, 50, 10, 70000, 70000], ts=(1, 2))
    fixed = case(slab, stride=64, n=18, ts=(3, 4))  # packet 15 = 40 bytes, 16 and 17 empty
    return indexed, fixed


def host_cases():
    """name -> case: every case of the host suite (the device suite runs the same ones)."""
    cs = {"golden": golden()[1], "edges_const_ts": edges(), "edges_packet_ts": edges(per_packet_ts=True)}
    for name in select_masks():
        cs["select_" + name] = select_case(name)
    for s in (1, 16, 60, 65535):
        cs[f"snaplen_{s}"] = edges(per_packet_ts=True, snaplen=s)
    cs["clamped_indexed"], cs["clamped_fixed"] = clamped()
    cs["empty_batch"] = case(np.zeros(0, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint32))
    return cs
