"""A capture that arrives in pieces: pkt_pcap_stream_* of the C ABI (include/pktgpu.h).

The capture path of tests/pcap.rs:7-37 (reference) fed as bytes arrive — a NIC ring drained into host
memory, a file read while it grows.  Each push appends bytes on the device; the device indexes only the
new bytes (from the first record the previous step could not count, kept in device words) and parses
the records they complete into the stream's columns, while later bytes are still copying in.

The stream holds a WINDOW of the capture in max_bytes of device memory: the global header, then the bytes
from the first unreleased record on.  Counts, offsets and columns are the window's; release(n) hands the
first n records back, so an open-ended capture runs in bounded memory:

    >>> st = PcapStream(0, max_bytes=64 << 20, cap=1 << 18, columns="all")         # device columns
    >>> for chunk in ring:                                                           # bytes / numpy u8
    ...     if len(chunk) > st.room():                                               # the window is full
    ...         c, _ = st.poll()
    ...         m = min(c, st.cap)
    ...         slab, offs, lens = st.batch()                                        # the packets, on the device
    ...         consume(st.out["ipv4_src"][:m], slab, offs, lens)                    # e.g. Parser.pcap_write(slab, offsets=offs, lens=lens)
    ...         st.release()                                                         # every record just polled
    ...     st.push(chunk)
    >>> n, (offs, lens) = st.finish()                                                # the last window
    >>> st.released()                                                                # (records, bytes) handed back before it

A stream that never releases is one capture of at most max_bytes held whole.
"""
import ctypes

import numpy as np

from . import ENTRY_ID, Parser, _torch, resolve_columns, schema


class PcapStream:
    """pkt_pcap_stream_open(device, max_bytes, cap, entry, out, step_bytes).  `out`: None = device
    columns allocated here (torch tensors), "pinned" = pinned host columns (numpy arrays from
    pkt_host_alloc: each step's columns are exported over the link), or a dict of either kind."""

    def __init__(self, device=0, max_bytes=1 << 28, cap=1 << 20, columns="all", entry="parse", out=None,
                 step_bytes=0):
        from . import _lib
        self._lib = _lib
        self._L = _lib.load()
        self.cap = int(cap)
        self._keep = None
        cols = resolve_columns(columns)
        if out is None:
            torch = _torch()
            dev = torch.device("cuda", device)
            out = {c: torch.zeros(schema.column_shape(c, self.cap), dtype=_tdtype_of(c), device=dev) for c in cols}
        elif isinstance(out, str) and out == "pinned":
            self._keep = Parser(device)  # owns the pinned allocations
            out = {c: self._keep.host_empty(schema.column_shape(c, self.cap), schema.column_dtype(c)) for c in cols}
        self.out = out
        o = _lib.PktOut()
        for c, v in out.items():
            ptr = v.data_ptr() if hasattr(v, "data_ptr") else v.ctypes.data
            setattr(o, c, ptr if _size(v) else None)
        e = ENTRY_ID[entry] if isinstance(entry, str) else int(entry)
        h = ctypes.c_void_p()
        rc = self._L.pkt_pcap_stream_open(int(device), int(max_bytes), self.cap, e, ctypes.byref(o), int(step_bytes),
                                          ctypes.byref(h))
        if rc != 0:
            raise RuntimeError(f"pkt_pcap_stream_open failed ({rc})")
        self._st = h
        self._dev = int(device)
        self._polled = 0
        self.aliased = None  # set by batch()

    def _check(self, rc, what):
        if rc != 0:
            msg = self._L.pkt_pcap_stream_last_error(self._st)
            raise RuntimeError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")

    def ctx(self):
        return self._L.pkt_pcap_stream_ctx(self._st)

    def push(self, data):
        a = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else \
            np.ascontiguousarray(data, np.uint8).reshape(-1)
        self._check(self._L.pkt_pcap_stream_push(self._st, a.ctypes.data if a.size else None, a.size),
                    "pkt_pcap_stream_push")

    def _counted(self, fn, what, index):
        n = ctypes.c_uint64()
        offs = np.zeros(self.cap, np.uint64) if index else None
        lens = np.zeros(self.cap, np.uint32) if index else None
        self._check(fn(self._st, ctypes.byref(n), offs.ctypes.data if index else None,
                       lens.ctypes.data if index else None), what)
        m = min(n.value, self.cap)
        self._polled = m
        return n.value, ((offs[:m], lens[:m]) if index else None)

    def poll(self, index=False):
        """Records wholly inside the bytes pushed so far (their columns written) -> (n, (offsets, lens))."""
        return self._counted(self._L.pkt_pcap_stream_poll, "pkt_pcap_stream_poll", index)

    def finish(self, index=True):
        """End of capture: the tail as pkt_pcap_index takes it -> (n, (offsets, lens))."""
        return self._counted(self._L.pkt_pcap_stream_finish, "pkt_pcap_stream_finish", index)

    def release(self, n=None):
        """pkt_pcap_stream_release: the consumer is done with window records [0, n) (None: every record of
        the last poll that the columns hold).  The columns, the index and batch()'s tensors restart at
        the next poll: what they held is stale after this call.  Blocking."""
        n = self._polled if n is None else int(n)
        self._check(self._L.pkt_pcap_stream_release(self._st, n), "pkt_pcap_stream_release")
        if n:
            self._polled = 0

    def room(self):
        """Bytes a push can take now (max_bytes minus the window's bytes)."""
        b = ctypes.c_uint64()
        self._check(self._L.pkt_pcap_stream_room(self._st, ctypes.byref(b)), "pkt_pcap_stream_room")
        return b.value

    def released(self):
        """(records, bytes) released so far: window record i is capture record i + records, window offset
        w is capture offset w + bytes."""
        r, b = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self._L.pkt_pcap_stream_released(self._st, ctypes.byref(r), ctypes.byref(b)),
                    "pkt_pcap_stream_released")
        return r.value, b.value

    def batch(self):
        """pkt_pcap_stream_batch: the window as of the last poll / finish as an indexed device batch ->
        (slab uint8, offsets uint64, lens uint32), torch tensors that ALIAS the stream's device memory (no
        copy; `aliased` is set True once that has been checked against the ABI's pointers), so
        Parser.pcap_write(slab, offsets=offsets, lens=lens) and its siblings take them directly.  They stay
        valid, and their contents stable, until the next push that starts a step, poll, release, finish
        or close.  Should a torch build copy instead of aliasing, the tensors are device copies of the same
        bytes (`aliased` False): still correct, at the price of the copy."""
        torch = _torch()
        b = self._lib.PktBatch()
        self._check(self._L.pkt_pcap_stream_batch(self._st, ctypes.byref(b)), "pkt_pcap_stream_batch")
        dev = torch.device("cuda", self._dev)
        n = int(b.n)

        def alias(ptr, nbytes, dtype):
            if not nbytes:
                return torch.empty(0, dtype=dtype, device=dev)
            t = torch.as_tensor(_DeviceBytes(self, ptr, nbytes), device=dev)
            self.aliased = t.data_ptr() == ptr
            return t.view(dtype)

        return (alias(b.slab, int(b.slab_len), torch.uint8), alias(b.offsets, n * 8, torch.uint64),
                alias(b.lens, n * 4, torch.uint32))

    def close(self):
        if getattr(self, "_st", None):
            self._L.pkt_pcap_stream_close(self._st)
            self._st = None
        if self._keep is not None:
            self._keep.close()
            self._keep = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _DeviceBytes:
    """`nbytes` of device memory at `ptr` for torch.as_tensor (the CUDA array interface); keeps the
    stream that owns the memory referenced while a tensor made from it lives."""

    def __init__(self, owner, ptr, nbytes):
        self._owner = owner
        self.__cuda_array_interface__ = {"shape": (int(nbytes),), "typestr": "|u1", "data": (int(ptr), False),
                                         "version": 2, "strides": None}


def _size(v):
    return v.numel() if hasattr(v, "numel") else v.size


def _tdtype_of(c):
    from . import _tdtype
    return _tdtype(schema.column_dtype(c))
