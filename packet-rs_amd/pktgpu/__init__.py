"""pktgpu — MI355X batched packet-header parser (Python host side).

Mirrors packet_rs's decode API for whole batches:

    fast::parse(&[u8]) -> PacketSlice            (src/parser/fast.rs:5)
    fast::parse_<hdr>(&[u8]) -> PacketSlice       (the 17 sub-entries, fast.rs:13-222)
    <Hdr>Slice::<field>() -> u64                  (make_header! getters, headers.rs:195-201)
    Packet::ipv4_checksum(&[u8]) -> u16           (src/packet.rs:93-107)

    >>> import torch, pktgpu
    >>> p = pktgpu.Parser(0)
    >>> res = p.parse(slab_u8_cuda, stride=64)              # every column
    >>> res = p.parse(slab, stride=64, columns=["chain", "ipv4", "udp"])
    >>> sl = pktgpu.packet_slice(res_host, i, packet_bytes) # PacketSlice-style view
    >>> sl.payload(), sl.to_vec(), sl["IPv4"].ttl()

All compute runs in the HIP kernels of lib/libpktgpu.so through its C ABI; torch only
provides device memory and the stream.  There is no CPU fallback.
"""
import ctypes

import numpy as np

from . import schema
from .schema import (ABI_VERSION, DEPTH_LIMIT, ENTRIES, ENTRY_ID, GROUPS, HDR_ID, HDR_NAMES,  # noqa: F401
                     HDR_SIZES, MAX_HDRS, OK, STATUS_NAMES, TRUNCATED)

__all__ = ["Parser", "FlowTable", "MatchProgram", "Dispatcher", "Lpm", "lpm_routes", "Forwarder", "fwd_adjacencies", "FragResult", "ReasmResult", "Scanner", "ScanResult", "scan_patterns", "match", "dispatch", "reorder", "segments", "flow_keys", "packet_slice", "view", "PacketSlice", "HeaderSlice", "resolve_columns", "schema"]


def resolve_columns(columns):
    """"all" | list of column names and/or group names -> ordered column names."""
    if columns is None or columns == "all":
        return list(schema.COLUMN_NAMES)
    if isinstance(columns, str):
        columns = [columns]
    out = set()
    for c in columns:
        if c in schema.GROUPS:
            out.update(schema.columns_of([c]))
        elif c in schema.COLUMN_NAMES:
            out.add(c)
        else:
            raise ValueError(f"unknown column or group {c!r}")
    return [c for c in schema.COLUMN_NAMES if c in out]


def _torch():
    import torch  # noqa: F401  (must be loaded before libpktgpu: shared HIP runtime)
    return torch


_TORCH_DT = None


def _tdtype(np_dtype):
    torch = _torch()
    global _TORCH_DT
    if _TORCH_DT is None:
        _TORCH_DT = {np.dtype(np.uint8): torch.uint8, np.dtype(np.uint16): torch.uint16,
                     np.dtype(np.uint32): torch.uint32, np.dtype(np.uint64): torch.uint64}
    return _TORCH_DT[np.dtype(np_dtype)]


class Parser:
    """A pkt_ctx bound to one HIP device."""

    def __init__(self, device=0, window=0):
        torch = _torch()
        from . import _lib
        self._L = _lib.load()
        self._lib = _lib
        self.device = int(device)
        self.torch_device = torch.device("cuda", self.device)
        h = ctypes.c_void_p()
        rc = self._L.pkt_ctx_create(self.device, ctypes.byref(h))
        if rc != 0:
            raise RuntimeError(f"pkt_ctx_create({device}) failed: {rc}")
        self._ctx = h
        if window:
            self._L.pkt_ctx_set_window(self._ctx, window)

    def close(self):
        for g in self.__dict__.pop("_gen_udp_cache", {}).values():  # pktgen.gen_udp's generators
            g.close()
        for p in getattr(self, "_pinned", []):
            self._L.pkt_host_free(self._ctx, p)
        self._pinned = []
        if getattr(self, "_ctx", None):
            self._L.pkt_ctx_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_window(self, window_bytes):
        self._L.pkt_ctx_set_window(self._ctx, int(window_bytes))

    def set_fastpath(self, enable):
        """Walk-free fast path for aligned Ether/IPv4/UDP|TCP packets (pkt_ctx_set_fastpath)."""
        self._check(self._L.pkt_ctx_set_fastpath(self._ctx, int(bool(enable))), "pkt_ctx_set_fastpath")

    def set_staging(self, mode):
        """0 = auto, 1 = per-lane windows, 2 = wave spans (pkt_ctx_set_staging)."""
        self._check(self._L.pkt_ctx_set_staging(self._ctx, int(mode)), "pkt_ctx_set_staging")

    def set_walk(self, mode):
        """0 = auto, 1 = waterfall, 2 = lockstep (pkt_ctx_set_walk)."""
        self._check(self._L.pkt_ctx_set_walk(self._ctx, int(mode)), "pkt_ctx_set_walk")

    def set_pcap_scan64(self, enable):
        """pkt_ctx_set_pcap_scan64: the device pcap indexer's 64-bit compositions for every file."""
        self._check(self._L.pkt_ctx_set_pcap_scan64(self._ctx, int(bool(enable))), "pkt_ctx_set_pcap_scan64")

    def set_host_piece(self, nbytes):
        """pkt_ctx_set_host_piece: bytes per copied piece of parse_pcap_host (0 = 16 MiB)."""
        self._check(self._L.pkt_ctx_set_host_piece(self._ctx, int(nbytes)), "pkt_ctx_set_host_piece")

    def _check(self, rc, what):
        if rc != 0:
            msg = self._L.pkt_ctx_last_error(self._ctx)
            raise RuntimeError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")

    def _stream(self, stream):
        torch = _torch()
        if stream is None:
            stream = torch.cuda.current_stream(self.torch_device)
        return ctypes.c_void_p(stream.cuda_stream)

    def _batch(self, slab, n, stride, offsets, lens):
        torch = _torch()
        assert slab.dtype == torch.uint8 and slab.is_cuda and slab.is_contiguous()
        b = self._lib.PktBatch()
        b.slab = slab.data_ptr()
        b.slab_len = slab.numel()
        if offsets is not None:
            assert offsets.dtype == torch.uint64 and lens is not None and lens.dtype == torch.uint32
            b.offsets = offsets.data_ptr()
            b.lens = lens.data_ptr()
            n = offsets.numel() if n is None else n
        else:
            if lens is not None:
                assert lens.dtype == torch.uint32
                b.lens = lens.data_ptr()
            if n is None:
                n = slab.numel() // stride
        b.stride = stride or 0
        b.n = int(n)
        return b

    def alloc(self, n, columns="all"):
        """Device output columns for n packets (torch tensors, uninitialised)."""
        torch = _torch()
        res = {}
        for c in resolve_columns(columns):
            res[c] = torch.empty(schema.column_shape(c, n), dtype=_tdtype(schema.column_dtype(c)),
                                 device=self.torch_device)
        return res

    def out_struct(self, res):
        o = self._lib.PktOut()
        for c, t in res.items():
            setattr(o, c, t.data_ptr() if t.numel() else None)
        return o

    def parse(self, slab, stride=None, n=None, offsets=None, lens=None, entry="parse",
              columns="all", out=None, stream=None):
        """fast::parse_<entry> over every packet of the slab -> {column: device tensor}."""
        e = ENTRY_ID[entry] if isinstance(entry, str) else int(entry)
        b = self._batch(slab, n, stride, offsets, lens)
        res = out if out is not None else self.alloc(b.n, columns)
        o = self.out_struct(res)
        self._check(self._L.pkt_parse_batch(self._ctx, ctypes.byref(b), e, ctypes.byref(o),
                                            self._stream(stream)), "pkt_parse_batch")
        return res

    def parse_host(self, slab, stride=None, n=None, offsets=None, lens=None, entry="parse",
                   columns="all", out=None, chunk=0):
        """The host-memory path (pkt_parse_host): numpy slab/offsets/lens in host memory ->
        {column: numpy array} in host memory, pipelined through the device in chunks.
        `out` may hold preallocated (e.g. pinned, see host_empty) numpy columns."""
        e = ENTRY_ID[entry] if isinstance(entry, str) else int(entry)
        slab = np.ascontiguousarray(slab, np.uint8).reshape(-1)
        b = self._lib.PktBatch()
        b.slab = slab.ctypes.data
        b.slab_len = slab.size
        keep = [slab]
        if offsets is not None:
            offsets = np.ascontiguousarray(offsets, np.uint64)
            lens = np.ascontiguousarray(lens, np.uint32)
            keep += [offsets, lens]
            b.offsets, b.lens = offsets.ctypes.data, lens.ctypes.data
            n = offsets.size if n is None else n
        else:
            if lens is not None:
                lens = np.ascontiguousarray(lens, np.uint32)
                keep.append(lens)
                b.lens = lens.ctypes.data
            n = slab.size // stride if n is None else n
        b.stride = stride or 0
        b.n = int(n)
        if out is None:
            out = {c: np.zeros(schema.column_shape(c, b.n), schema.column_dtype(c))
                   for c in resolve_columns(columns)}
        o = self._lib.PktOut()
        for c, a in out.items():
            setattr(o, c, a.ctypes.data if a.size else None)
        self._check(self._L.pkt_parse_host(self._ctx, ctypes.byref(b), e, ctypes.byref(o), int(chunk)),
                    "pkt_parse_host")
        return out

    def parse_pcap(self, buf, cap=None, entry="parse", columns="all", out=None, offsets=None, lens=None,
                   stream=None):
        """pkt_parse_pcap: a pcap file in the uint8 device tensor `buf` -> (n records, {column: device
        tensor} sized for cap records (slot columns [16][cap]), offsets, lens), index and parse in one
        call with one host synchronisation.  cap=None: the file's size bounds the count (>= 16 B per
        record), which sizes the outputs.  `out` may also be a PktOut built once by out_struct() (it is
        then returned in place of the dict): the 49 column pointers are not marshalled per call."""
        torch = _torch()
        assert buf.dtype == torch.uint8 and buf.is_cuda and buf.is_contiguous()
        e = ENTRY_ID[entry] if isinstance(entry, str) else int(entry)
        if cap is None:
            cap = max(1, (buf.numel() - 24) // 16)
        res = out if out is not None else self.alloc(cap, columns)
        o = res if isinstance(res, self._lib.PktOut) else self.out_struct(res)
        offsets = offsets if offsets is not None else torch.empty(cap, dtype=torch.uint64, device=self.torch_device)
        lens = lens if lens is not None else torch.empty(cap, dtype=torch.uint32, device=self.torch_device)
        n = ctypes.c_uint64()
        self._check(self._L.pkt_parse_pcap(self._ctx, buf.data_ptr(), buf.numel(), e, ctypes.byref(o),
                                           offsets.data_ptr(), lens.data_ptr(), int(cap), ctypes.byref(n),
                                           self._stream(stream)), "pkt_parse_pcap")
        return n.value, res, offsets, lens

    def parse_pcap_async(self, buf, cap, out, offsets, lens, entry="parse", stream=None):
        """pkt_parse_pcap_async: queue the index and the parse of the capture in `buf` on `stream`
        (no host wait) into the caller's `out` / `offsets` / `lens` (sized for cap records).
        pcap_result() waits for it and returns the record count; one capture in flight per Parser."""
        torch = _torch()
        assert buf.dtype == torch.uint8 and buf.is_cuda and buf.is_contiguous()
        e = ENTRY_ID[entry] if isinstance(entry, str) else int(entry)
        o = out if isinstance(out, self._lib.PktOut) else self.out_struct(out)
        self._check(self._L.pkt_parse_pcap_async(self._ctx, buf.data_ptr(), buf.numel(), e, ctypes.byref(o),
                                                 offsets.data_ptr(), lens.data_ptr(), int(cap),
                                                 self._stream(stream)), "pkt_parse_pcap_async")

    def pcap_result(self):
        """pkt_parse_pcap_result: waits for the queued parse_pcap_async and returns its record
        count; raises on its errors."""
        n = ctypes.c_uint64()
        self._check(self._L.pkt_parse_pcap_result(self._ctx, ctypes.byref(n)), "pkt_parse_pcap_result")
        return n.value

    def parse_pcap_host_async(self, buf, cap, out, entry="parse"):
        """pkt_parse_pcap_host_async: queue copy-in, index and parse of the capture in pinned host
        memory `buf` (numpy uint8 from host_empty) into the pinned columns `out` ({column: numpy
        array from host_empty}, sized for cap records); pcap_host_result() waits and returns the
        record count.  One capture in flight per Parser."""
        e = ENTRY_ID[entry] if isinstance(entry, str) else int(entry)
        o = self._lib.PktOut()
        for c, v in out.items():
            setattr(o, c, v.ctypes.data if v.size else None)
        self._check(self._L.pkt_parse_pcap_host_async(self._ctx, buf.ctypes.data, buf.size, e, ctypes.byref(o),
                                                      int(cap)), "pkt_parse_pcap_host_async")

    def pcap_host_result(self):
        n = ctypes.c_uint64()
        self._check(self._L.pkt_parse_pcap_host_result(self._ctx, ctypes.byref(n)), "pkt_parse_pcap_host_result")
        return n.value

    def parse_pcap_host(self, buf, cap, entry="parse", columns="all", out=None, index=True):
        """pkt_parse_pcap_host: a pcap file in host memory (numpy uint8 / bytes; pinned via host_empty
        for the full link rate) -> (n records, {column: numpy array} sized for `cap` records, slot
        columns [16][cap], (offsets, lens) or None).  One blocking call: copy in, device index,
        parse, columns out."""
        e = ENTRY_ID[entry] if isinstance(entry, str) else int(entry)
        a = np.frombuffer(buf, np.uint8) if isinstance(buf, (bytes, bytearray)) else np.ascontiguousarray(buf, np.uint8)
        if out is None:
            out = {c: np.zeros(schema.column_shape(c, cap), schema.column_dtype(c)) for c in resolve_columns(columns)}
        o = self._lib.PktOut()
        for c, v in out.items():
            setattr(o, c, v.ctypes.data if v.size else None)
        offs = np.zeros(cap, np.uint64) if index else None
        lens = np.zeros(cap, np.uint32) if index else None
        n = ctypes.c_uint64()
        self._check(self._L.pkt_parse_pcap_host(self._ctx, a.ctypes.data, a.size, e, ctypes.byref(o),
                                                offs.ctypes.data if index else None,
                                                lens.ctypes.data if index else None, int(cap), ctypes.byref(n)),
                    "pkt_parse_pcap_host")
        m = min(n.value, cap)
        return n.value, out, ((offs[:m], lens[:m]) if index else None)

    def host_empty(self, shape, dtype):
        """A numpy array in pinned host memory (pkt_host_alloc), freed with the Parser."""
        dtype = np.dtype(dtype)
        nbytes = int(np.prod(shape)) * dtype.itemsize
        p = ctypes.c_void_p()
        self._check(self._L.pkt_host_alloc(self._ctx, max(1, nbytes), ctypes.byref(p)), "pkt_host_alloc")
        if not hasattr(self, "_pinned"):
            self._pinned = []
        self._pinned.append(p)
        buf = (ctypes.c_uint8 * max(1, nbytes)).from_address(p.value)
        return np.frombuffer(buf, dtype=np.uint8, count=nbytes).view(dtype).reshape(shape)

    def parse_batches(self, batches, outs, entry="parse", stream=None):
        """pkt_parse_batches: batches = [(slab, n, stride, offsets, lens)], outs = [{column: tensor}]
        -> outs.  One launch over every batch when they share size and layout and their outputs lie
        at one common distance (e.g. one packed buffer each, mgpu.packed_views); else one each."""
        e = ENTRY_ID[entry] if isinstance(entry, str) else int(entry)
        k = len(batches)
        barr = (self._lib.PktBatch * max(1, k))()
        oarr = (self._lib.PktOut * max(1, k))()
        for i, (bt, out) in enumerate(zip(batches, outs)):
            barr[i] = self._batch(*bt)
            oarr[i] = self.out_struct(out)
        self._check(self._L.pkt_parse_batches(self._ctx, barr, k, e, oarr, self._stream(stream)), "pkt_parse_batches")
        return outs

    def batches_call(self, batches, out_structs, entry=0, stream=None):
        """A zero-argument callable issuing one prebuilt pkt_parse_batches (bench loop)."""
        k = len(batches)
        barr = (self._lib.PktBatch * k)(*batches)
        oarr = (self._lib.PktOut * k)(*out_structs)
        f, ctx, s = self._L.pkt_parse_batches, self._ctx, self._stream(stream)

        def call():
            rc = f(ctx, barr, k, entry, oarr, s)
            if rc != 0:
                self._check(rc, "pkt_parse_batches")
        call.keep = (barr, oarr)
        return call

    def launch(self, batch_struct, entry, out_struct, stream=None):
        """Relaunch with prebuilt ctypes structs (no per-call Python allocation; bench loop)."""
        self._check(self._L.pkt_parse_batch(self._ctx, ctypes.byref(batch_struct), entry,
                                            ctypes.byref(out_struct), self._stream(stream)),
                    "pkt_parse_batch")

    def extract_fields(self, slab, chain, specs, stride=None, n=None, offsets=None, lens=None,
                       stream=None):
        """Batched getter: specs = [(hdr_type|name, occurrence, start, end)] -> (values, found)."""
        torch = _torch()
        b = self._batch(slab, n, stride, offsets, lens)
        ch = self._lib.PktChain()
        ch.n_hdrs = chain["n_hdrs"].data_ptr()
        ch.hdr_type = chain["hdr_type"].data_ptr()
        ch.hdr_off = chain["hdr_off"].data_ptr()
        k = len(specs)
        sp = (self._lib.PktFieldSpec * max(1, k))()
        for i, (t, occ, s, e) in enumerate(specs):
            t = HDR_ID[t] if isinstance(t, str) else int(t)
            sp[i] = self._lib.PktFieldSpec(t, occ, s, e, 0)
        vals = [torch.empty(b.n, dtype=torch.uint64, device=self.torch_device) for _ in range(k)]
        found = [torch.empty(b.n, dtype=torch.uint8, device=self.torch_device) for _ in range(k)]
        vp = (ctypes.c_void_p * max(1, k))(*[v.data_ptr() for v in vals])
        fp = (ctypes.c_void_p * max(1, k))(*[f.data_ptr() for f in found])
        self._check(self._L.pkt_extract_fields(self._ctx, ctypes.byref(b), ctypes.byref(ch), sp, k,
                                               vp, fp, self._stream(stream)), "pkt_extract_fields")
        return vals, found

    def to_vec(self, slab, parsed, stride=None, n=None, offsets=None, lens=None, dst=None,
               dst_offsets=None, stream=None):
        """PacketSlice::to_vec of every parsed packet into `dst` (default: a new buffer with
        the input's layout).  Returns (dst, out_len)."""
        torch = _torch()
        b = self._batch(slab, n, stride, offsets, lens)
        if dst is None:
            dst = torch.zeros_like(slab)
        out_len = torch.empty(b.n, dtype=torch.uint32, device=self.torch_device)
        o = self.out_struct(parsed)
        self._check(self._L.pkt_to_vec_batch(self._ctx, ctypes.byref(b), ctypes.byref(o),
                                             ctypes.c_void_p(dst.data_ptr()), dst.numel(),
                                             ctypes.c_void_p(dst_offsets.data_ptr() if dst_offsets is not None else 0),
                                             ctypes.c_void_p(out_len.data_ptr()), self._stream(stream)),
                    "pkt_to_vec_batch")
        return dst, out_len

    def _chain(self, chain):
        ch = self._lib.PktChain()
        ch.n_hdrs = chain["n_hdrs"].data_ptr()
        ch.hdr_type = chain["hdr_type"].data_ptr()
        ch.hdr_off = chain["hdr_off"].data_ptr()
        return ch

    def set_fields(self, slab, chain, specs, values, stride=None, n=None, offsets=None, lens=None,
                   stream=None, ipv4_checksum=None):
        """In-place batched `<Hdr>::set_<field>(v)`: specs = [(hdr_type|name, occurrence, start,
        end)], values = one uint64 device tensor per spec.  ipv4_checksum=occ also refreshes that
        IPv4 header's checksum after the setters, in the same launch (pkt_set_fields_csum)."""
        b = self._batch(slab, n, stride, offsets, lens)
        k = len(specs)
        sp = (self._lib.PktFieldSpec * max(1, k))()
        for i, (t, occ, s, e) in enumerate(specs):
            t = HDR_ID[t] if isinstance(t, str) else int(t)
            sp[i] = self._lib.PktFieldSpec(t, occ, s, e, 0)
        vp = (ctypes.c_void_p * max(1, k))(*[v.data_ptr() for v in values])
        if ipv4_checksum is None:
            self._check(self._L.pkt_set_fields(self._ctx, ctypes.byref(b), ctypes.byref(self._chain(chain)),
                                               sp, k, vp, self._stream(stream)), "pkt_set_fields")
        else:
            self._check(self._L.pkt_set_fields_csum(self._ctx, ctypes.byref(b), ctypes.byref(self._chain(chain)),
                                                    sp, k, vp, int(ipv4_checksum), self._stream(stream)),
                        "pkt_set_fields_csum")

    def ipv4_update_checksum(self, slab, chain, occurrence=0, stride=None, n=None, offsets=None,
                             lens=None, stream=None):
        """In-place: the occurrence-th IPv4 header's checksum := Packet::ipv4_checksum(header)."""
        b = self._batch(slab, n, stride, offsets, lens)
        self._check(self._L.pkt_ipv4_update_checksum(self._ctx, ctypes.byref(b),
                                                     ctypes.byref(self._chain(chain)), occurrence,
                                                     self._stream(stream)), "pkt_ipv4_update_checksum")

    def broadcast(self, src, n, stride, dst=None, stream=None):
        """n clones of the device packet `src` (uint8 tensor) at `stride` -> flat uint8 slab."""
        torch = _torch()
        if dst is None:
            dst = torch.empty(n * stride, dtype=torch.uint8, device=self.torch_device)
        self._check(self._L.pkt_broadcast(self._ctx, ctypes.c_void_p(src.data_ptr()), src.numel(), n,
                                          stride, ctypes.c_void_p(dst.data_ptr()), self._stream(stream)),
                    "pkt_broadcast")
        return dst

    def ipv4_checksum(self, hdrs, stride=20, n=None, stream=None):
        """Packet::ipv4_checksum over n 20-byte headers at a fixed stride (device u8 tensor)."""
        torch = _torch()
        n = hdrs.numel() // stride if n is None else n
        out = torch.empty(n, dtype=torch.uint16, device=self.torch_device)
        self._check(self._L.pkt_ipv4_checksum_batch(self._ctx, ctypes.c_void_p(hdrs.data_ptr()),
                                                    stride, n, ctypes.c_void_p(out.data_ptr()),
                                                    self._stream(stream)), "pkt_ipv4_checksum_batch")
        return out

    def pcap_index(self, buf, cap=None, stream=None):
        """pkt_pcap_index_device: (offsets uint64, lens uint32) device tensors of the records of a
        tests/pcap.rs-format file held in the uint8 device tensor `buf` (16-byte aligned).
        With cap=None the count is found first and exactly that many records are written."""
        torch = _torch()
        assert buf.dtype == torch.uint8 and buf.is_cuda and buf.is_contiguous()
        n = ctypes.c_uint64()
        s = self._stream(stream)
        if cap is None:
            self._check(self._L.pkt_pcap_index_device(self._ctx, buf.data_ptr(), buf.numel(), None, None,
                                                      0, ctypes.byref(n), s), "pkt_pcap_index_device")
            cap = n.value
        offs = torch.empty(cap, dtype=torch.uint64, device=self.torch_device)
        lens = torch.empty(cap, dtype=torch.uint32, device=self.torch_device)
        self._check(self._L.pkt_pcap_index_device(self._ctx, buf.data_ptr(), buf.numel(),
                                                  offs.data_ptr() if cap else None,
                                                  lens.data_ptr() if cap else None, cap,
                                                  ctypes.byref(n), s), "pkt_pcap_index_device")
        k = min(cap, n.value)
        return offs[:k], lens[:k], n.value

    def _pcap_write_args(self, slab, offsets, lens, stride, select, snaplen, ts, dst, index, n=None):
        """The marshalled arguments shared by pcap_write / pcap_write_async."""
        torch = _torch()
        b = self._batch(slab, n, stride, offsets, lens)
        n = b.n
        if select is not None:
            if select.dtype == torch.bool:
                select = select.view(torch.uint8)
            assert select.dtype == torch.uint8 and select.is_cuda and select.numel() == n
        tv, tsp = [0, 0], [None, None]
        for k in range(2):
            if isinstance(ts[k], int):
                tv[k] = ts[k]
            else:
                assert ts[k].dtype == torch.uint32 and ts[k].is_cuda and ts[k].numel() == n
                tsp[k] = ts[k]
        if dst is None:
            # the exact bound: 24 + 16 n + the packets' lengths, each capped as the kernel caps it
            cap = min(65535, int(snaplen)) if snaplen else 65535
            if lens is None:
                data = n * min(int(stride), cap)
            else:
                data = int(lens[:n].view(torch.int32).to(torch.int64).bitwise_and_(0xFFFFFFFF).clamp_(max=cap).sum().item()) if n else 0
            dst = torch.empty(24 + 16 * n + data, dtype=torch.uint8, device=self.torch_device)
        assert dst.dtype == torch.uint8 and dst.is_cuda and dst.is_contiguous()
        rec = (None, None, None)
        if index:
            rec = (torch.empty(n, dtype=torch.uint64, device=self.torch_device),
                   torch.empty(n, dtype=torch.uint32, device=self.torch_device),
                   torch.empty(n, dtype=torch.uint32, device=self.torch_device))
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None  # noqa: E731
        args = (ctypes.byref(b), ptr(select), int(snaplen), tv[0], tv[1], ptr(tsp[0]), ptr(tsp[1]),
                ptr(dst), dst.numel(), ptr(rec[0]), ptr(rec[1]), ptr(rec[2]))
        return args, dst, rec, (b, select, tsp)

    def _pcap_write_done(self, rc, what, total, n, dst, rec):
        if rc != 0 and total > dst.numel():
            raise RuntimeError(f"{what}: dst holds {dst.numel()} bytes, the capture needs {total} "
                               f"({n} records)")
        self._check(rc, what)
        return (dst[:total], n) + tuple(r[:n] if r is not None else None for r in rec)

    def pcap_write(self, slab, offsets=None, lens=None, stride=None, select=None, snaplen=0, ts=(0, 0),
                   dst=None, index=True, stream=None, n=None):
        """pkt_pcap_write: the selected packets of a device batch (fixed `stride`, or `offsets` / `lens`)
        as one tests/pcap.rs capture in device memory -> (capture, n, offsets, lens, src_index).
        `capture` is a uint8 view of exactly the bytes written; `select` a uint8 / bool device tensor
        [n] or None (all); `snaplen` 0 = whole packets; `ts` = (sec, usec), each an int (one time for
        the file) or a uint32 device tensor indexed by source packet.  dst=None allocates the exact
        upper bound (the device sum of `lens` for an indexed batch); a caller's `dst` that is too
        small raises with the size needed.  index=True also returns the written records' (data
        offset, incl_len) — with `capture` an indexed batch — and their source packet indices."""
        args, dst, rec, keep = self._pcap_write_args(slab, offsets, lens, stride, select, snaplen, ts, dst, index, n)
        total, n = ctypes.c_uint64(), ctypes.c_uint64()
        rc = self._L.pkt_pcap_write(self._ctx, *args, ctypes.byref(total), ctypes.byref(n), self._stream(stream))
        return self._pcap_write_done(rc, "pkt_pcap_write", total.value, n.value, dst, rec)

    def pcap_write_async(self, slab, offsets=None, lens=None, stride=None, select=None, snaplen=0, ts=(0, 0),
                         dst=None, index=True, stream=None, n=None):
        """pkt_pcap_write_async: queue pcap_write on `stream` without waiting for its totals (pass
        `dst`: sizing one for an indexed batch waits for the sum of `lens`).  pcap_write_result()
        waits and returns pcap_write's tuple; one write in flight per Parser."""
        args, dst, rec, keep = self._pcap_write_args(slab, offsets, lens, stride, select, snaplen, ts, dst, index, n)
        self._check(self._L.pkt_pcap_write_async(self._ctx, *args, self._stream(stream)), "pkt_pcap_write_async")
        self._pcap_write_queued = (dst, rec, keep, (slab, offsets, lens))

    def pcap_write_result(self):
        """pkt_pcap_write_result: waits for the queued pcap_write_async -> pcap_write's tuple."""
        total, n = ctypes.c_uint64(), ctypes.c_uint64()
        rc = self._L.pkt_pcap_write_result(self._ctx, ctypes.byref(total), ctypes.byref(n))
        q = self.__dict__.pop("_pcap_write_queued", None)
        if q is None:
            self._check(rc, "pkt_pcap_write_result")
            raise RuntimeError("pcap_write_result: no write queued")
        return self._pcap_write_done(rc, "pkt_pcap_write_result", total.value, n.value, q[0], q[1])

    def _compare_args(self, a, b, ignore, chain, outputs=True):
        """The marshalled arguments shared by compare / compare_async."""
        torch = _torch()
        ba, bb = (self._batch(d["slab"], d.get("n"), d.get("stride"), d.get("offsets"), d.get("lens")) for d in (a, b))
        n = ba.n
        sp, k = _cmp_specs(self._lib, ignore)
        if k and chain is None:
            raise ValueError("compare: ignore needs the chain columns of a parse of `a`")
        ch = self._chain(chain) if chain is not None else None
        out = (None, None, None)
        if outputs:
            out = (torch.empty(n, dtype=torch.uint8, device=self.torch_device),
                   torch.empty(n, dtype=torch.uint32, device=self.torch_device),
                   torch.empty(n, dtype=torch.uint32, device=self.torch_device))
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None  # noqa: E731
        args = (ctypes.byref(ba), ctypes.byref(bb), ctypes.byref(ch) if ch is not None else None, sp, k,
                ptr(out[0]), ptr(out[1]), ptr(out[2]))
        return args, out, (ba, bb, ch, sp)

    def compare(self, a, b, ignore=(), chain=None, stream=None):
        """pkt_compare_batch: Packet::compare of packet i of `a` against packet i of `b` ->
        (result uint8, matching uint32, first_diff uint32, summary dict).  `a`, `b`: dicts with the
        batch's `slab` and `stride` or `offsets` / `lens` (optionally `n`), fixed-stride or indexed in
        any mix.  result: 0 equal, 1 the lengths differ, 2 bytes differ (pktgpu.CMP_*); matching =
        the number of equal positions of the common bytes, first_diff = the first unequal one (the
        common length if none).  `ignore` = up to 16 (hdr_type|name, occurrence, start, end) bit
        ranges, as for extract_fields, resolved per packet against `chain`, the chain columns of a
        parse of `a`; their bits never count as a difference.  Both sides are raw bytes: run to_vec
        first for the reference's to_vec order."""
        args, out, keep = self._compare_args(a, b, ignore, chain)
        sm = self._lib.PktCmpSummary()
        self._check(self._L.pkt_compare_batch(self._ctx, *args, ctypes.byref(sm), self._stream(stream)),
                    "pkt_compare_batch")
        return out + (_cmp_summary(sm),)

    def compare_async(self, a, b, ignore=(), chain=None, stream=None):
        """pkt_compare_batch_async: queue compare on `stream` without waiting for its summary.
        compare_result() waits and returns compare's tuple; one compare in flight per Parser."""
        args, out, keep = self._compare_args(a, b, ignore, chain)
        self._check(self._L.pkt_compare_batch_async(self._ctx, *args, self._stream(stream)), "pkt_compare_batch_async")
        self._compare_queued = (out, keep, (a, b, chain))

    def compare_result(self):
        """pkt_compare_result: waits for the queued compare_async -> compare's tuple."""
        sm = self._lib.PktCmpSummary()
        rc = self._L.pkt_compare_result(self._ctx, ctypes.byref(sm))
        q = self.__dict__.pop("_compare_queued", None)
        self._check(rc, "pkt_compare_result")
        if q is None:
            raise RuntimeError("compare_result: no compare queued")
        return q[0] + (_cmp_summary(sm),)

    def _edit_args(self, slab, parsed, ops, stride=None, n=None, offsets=None, lens=None, select=None, dst=None,
                   dst_offsets=None, slot=None, outputs=(True, True, True)):
        """The marshalled arguments of pkt_edit_batch (after ctx, before stream); `outputs`: whether
        out_len, edit_status and out_chain are asked for."""
        torch = _torch()
        b = self._batch(slab, n, stride, offsets, lens)
        n = b.n
        arr, k, data = _edit_ops(self._lib, ops)
        slot = _edit_slot(slot, stride, dst_offsets, arr, k)
        if select is not None:
            if select.dtype == torch.bool:
                select = select.view(torch.uint8)
            assert select.dtype == torch.uint8 and select.is_cuda and select.numel() == n
        if dst is None:
            if dst_offsets is not None:
                raise ValueError("edit: dst_offsets needs dst")
            dst = torch.empty(n * slot, dtype=torch.uint8, device=self.torch_device)
        assert dst.dtype == torch.uint8 and dst.is_cuda and dst.is_contiguous()
        if dst_offsets is not None:
            assert dst_offsets.dtype == torch.uint64 and dst_offsets.is_cuda and dst_offsets.numel() == n
        out_len = torch.empty(n, dtype=torch.uint32, device=self.torch_device) if outputs[0] else None
        status = torch.empty(n, dtype=torch.uint8, device=self.torch_device) if outputs[1] else None
        chain = None
        if outputs[2]:
            chain = {c: torch.zeros(schema.column_shape(c, n), dtype=_tdtype(schema.column_dtype(c)),
                                    device=self.torch_device) for c in schema.columns_of(["chain"])}
        po = self.out_struct(parsed)
        oc = self.out_struct(chain) if chain is not None else None
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None  # noqa: E731
        args = (ctypes.byref(b), ctypes.byref(po), arr, k, data, len(data), ptr(select), ptr(dst), dst.numel(),
                ptr(dst_offsets), slot, ptr(out_len), ptr(status), ctypes.byref(oc) if oc is not None else None)
        return args, (dst, out_len, status, chain), (b, po, oc, arr, data)

    def edit(self, slab, parsed, ops, stride=None, n=None, offsets=None, lens=None, select=None, dst=None,
             dst_offsets=None, slot=None, stream=None):
        """pkt_edit_batch: Packet::push / insert / pop / remove on every packet's header list, then
        to_vec -> (dst, out_len uint32, status uint8, chain).  `parsed`: the chain columns of a parse of
        the batch.  `ops` (at most 8, the same program for every packet): ("pop",), ("remove", k),
        ("remove_hdr", hdr, occurrence), ("insert", hdr, bytes[, index]) (index 0 by default, as
        Packet::insert) and ("push", hdr, bytes).  `select`: a uint8 / bool device tensor [n], the
        packets with 0 are written unedited.  Packet i goes to dst + dst_offsets[i], or i * slot, and
        may take `slot` bytes (default: stride plus the inserted bytes, rounded up to 16); dst=None
        allocates n * slot bytes.  status: pktgpu.EDIT_OK / _SKIPPED / _DEPTH / _NO_ROOM; `chain`: the
        edited packets' chain columns ({column: tensor}; slot rows past n_hdrs are 0), which with
        (dst, out_len) feed set_fields, extract_fields, compare, pcap_write and to_vec with no second
        parse.  Asynchronous on `stream`."""
        args, out, keep = self._edit_args(slab, parsed, ops, stride, n, offsets, lens, select, dst, dst_offsets, slot)
        self._check(self._L.pkt_edit_batch(self._ctx, *args, self._stream(stream)), "pkt_edit_batch")
        return out

    def _l4_args(self, slab, chain, which=0, update=False, keep_zero_udp=False, stride=None, n=None, offsets=None,
                 lens=None, outputs=(True, True, True)):
        """The marshalled arguments of pkt_l4_checksum_batch (after ctx, before stream); `outputs`: whether
        calc, stored and status are asked for."""
        torch = _torch()
        b = self._batch(slab, n, stride, offsets, lens)
        ch = self._chain(chain)
        flags = (schema.L4_UPDATE if update else 0) | (schema.L4_KEEP_ZERO_UDP if keep_zero_udp else 0)
        dts = (torch.uint16, torch.uint16, torch.uint8)
        out = tuple(torch.empty(b.n, dtype=dt, device=self.torch_device) if want else None
                    for dt, want in zip(dts, outputs))
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None  # noqa: E731
        args = (ctypes.byref(b), ctypes.byref(ch), int(which), flags, ptr(out[0]), ptr(out[1]), ptr(out[2]))
        return args, out, (b, ch)

    def l4_checksum(self, slab, chain, which=0, update=False, keep_zero_udp=False, stride=None, n=None, offsets=None,
                    lens=None, stream=None):
        """pkt_l4_checksum_batch: the RFC 1071 checksum of every packet's TCP / UDP / ICMP segment with its
        pseudo-header -> {"calc": uint16, "stored": uint16, "status": uint8} (pktgpu.L4_OK / _BAD /
        _UNCHECKED / _ABSENT / _NO_IP / _SPAN / _FRAGMENT; names in schema.L4_STATUS).  `chain`: the chain
        columns of a parse of the batch, or edit's out chain.  `which`: the k-th TCP / UDP / ICMP header of
        the list, counted together from 0, or pktgpu.L4_LAST.  update=True stores calc into the packets
        (exactly the two checksum bytes of each summed packet; keep_zero_udp=True leaves a UDP/IPv4
        checksum of 0 alone); the status still describes the field as it was read.  Asynchronous on
        `stream`."""
        args, out, keep = self._l4_args(slab, chain, which, update, keep_zero_udp, stride, n, offsets, lens)
        self._check(self._L.pkt_l4_checksum_batch(self._ctx, *args, self._stream(stream)), "pkt_l4_checksum_batch")
        return {"calc": out[0], "stored": out[1], "status": out[2]}

    def _flow_args(self, slab, chain, which_ip=schema.FLOW_LAST, symmetric=False, ports=True, seed=0, rss_key=None,
                   stride=None, n=None, offsets=None, lens=None, outputs=(True,) * 6):
        """The marshalled arguments of pkt_flow_key_batch (after ctx, before stream); `outputs`: whether keys,
        hash, rss, dir, plen and status are asked for (rss only with an rss_key)."""
        torch = _torch()
        b = self._batch(slab, n, stride, offsets, lens)
        ch = self._chain(chain)
        flags = (schema.FLOW_SYMMETRIC if symmetric else 0) | (0 if ports else schema.FLOW_NO_PORTS)
        rk = _rss_key(rss_key)
        shapes = (((b.n, 40), torch.uint8), ((b.n,), torch.uint64), ((b.n,), torch.uint32), ((b.n,), torch.uint8),
                  ((b.n,), torch.uint32), ((b.n,), torch.uint8))
        want = list(outputs)
        want[2] = want[2] and rk is not None
        out = tuple(torch.empty(shp, dtype=dt, device=self.torch_device) if w else None
                    for (shp, dt), w in zip(shapes, want))
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None  # noqa: E731
        args = (ctypes.byref(b), ctypes.byref(ch), int(which_ip), flags, int(seed), rk, *[ptr(t) for t in out])
        return args, out, (b, ch, rk)

    def flow_keys(self, slab, chain, which_ip=schema.FLOW_LAST, symmetric=False, ports=True, seed=0, rss_key=None,
                  stride=None, n=None, offsets=None, lens=None, stream=None):
        """pkt_flow_key_batch: every packet's flow key -> {"keys": uint8 [n, 40] (pkt_flow_key_t:
        schema.FLOW_KEY_DTYPE), "hash": uint64, "rss": uint32 (only with an `rss_key` of 40 bytes: the
        Toeplitz hash NICs compute), "dir": uint8, "plen": uint32, "status": uint8 (pktgpu.FLOW_OK / _NO_IP /
        _SPAN)}.  `chain`: the chain columns of a parse of the batch, a stream's columns over its batch(), or
        edit's out chain.  `which_ip`: the k-th IPv4 / IPv6 header of the list, counted together from 0, or
        pktgpu.FLOW_LAST (the innermost).  symmetric=True orders the two ends, so both directions of a
        connection share a key and `dir` tells them apart; ports=False keys on addresses and protocol alone.
        The dict is what FlowTable.update takes.  Asynchronous on `stream`."""
        args, out, keep = self._flow_args(slab, chain, which_ip, symmetric, ports, seed, rss_key, stride, n, offsets, lens)
        self._check(self._L.pkt_flow_key_batch(self._ctx, *args, self._stream(stream)), "pkt_flow_key_batch")
        res = dict(zip(("keys", "hash", "rss", "dir", "plen", "status"), out))
        if res["rss"] is None:
            del res["rss"]
        return res

    def match_program(self, rules, default=0):
        """pkt_match_create: compile and upload a first-match rule table -> MatchProgram.  `rules`: a list of
        (action, [term, ...]), a rule being the AND of its terms and action 0 meaning "not selected".  A term is
        (hdr, occurrence, field, op, a[, b]) with hdr a header name or id, field a name from pktgpu.fields or a
        (start, end) bit pair (None for "has"), op one of "has", "not has", "==", "!=", "in", "not in"; for
        "==" / "!=" `a` is the value and the optional `b` a mask (default: all ones), for "in" / "not in" a..b
        is the inclusive range.  ("len", "in" | "not in", lo, hi) tests the packet's length.  `default`: the
        action of a packet no rule matches.  (A (PktMatchTerm array, PktMatchRule array) pair is taken as it
        is: rules that share or overlap their terms.)"""
        return MatchProgram(self, rules, default)

    def match(self, slab, chain, prog, stride=None, n=None, offsets=None, lens=None,
              outputs=("rule", "action", "select", "matched"), hits=None, bytes=None, stream=None):
        """pkt_match_batch: evaluate a MatchProgram over a parsed batch in one pass -> a dict of device tensors,
        the `outputs` asked for among "rule" (uint8: the first matching rule, pktgpu.MATCH_NONE = none),
        "action" (uint32), "select" (uint8: action != 0, what pcap_write and edit take) and "matched" (uint64:
        bit r = rule r matches).  hits / bytes: True allocates zeroed uint64 [nrules + 1] counters and returns
        them; a tensor passed in is accumulated into (index nrules = no rule).  `chain`: the chain columns of
        a parse of the batch, a stream's columns over its batch(), or edit's out chain.  Asynchronous on
        `stream`."""
        torch = _torch()
        b = self._batch(slab, n, stride, offsets, lens)
        ch = self._chain(chain)
        dts = {"rule": torch.uint8, "action": torch.uint32, "select": torch.uint8, "matched": torch.uint64}
        res = {k: torch.empty(b.n, dtype=dts[k], device=self.torch_device) for k in outputs}
        for name, c in (("hits", hits), ("bytes", bytes)):
            if c is True:
                c = torch.zeros(prog.nrules + 1, dtype=torch.uint64, device=self.torch_device)
            if c is not None and c is not False:
                assert c.dtype == torch.uint64 and c.numel() == prog.nrules + 1 and c.is_contiguous()
                res[name] = c
        ptr = lambda k: res[k].data_ptr() if k in res and res[k].numel() else None  # noqa: E731
        self._check(self._L.pkt_match_batch(prog._m, ctypes.byref(b), ctypes.byref(ch), ptr("rule"), ptr("action"),
                                            ptr("select"), ptr("matched"), ptr("hits"), ptr("bytes"),
                                            self._stream(stream)), "pkt_match_batch")
        return res

    def dispatcher(self, nbuckets, table=None, max_n=1 << 20):
        """pkt_dispatch_create: a stable partition of up to `max_n` packets into `nbuckets` (1..256) queues ->
        Dispatcher.  table=None is DIRECT mode (bucket = key when key < nbuckets, else dropped: an action, a rule
        id, a shard number); a table (host integers, a power-of-two length up to 4096, entries < nbuckets or
        pktgpu.DISPATCH_DROP) is the RSS indirection table: bucket = table[key & (len - 1)]."""
        return Dispatcher(self, nbuckets, table, max_n)

    def lpm(self, routes, default_nexthop=0, max_bytes=0, host=False):
        """pkt_lpm_create: compile a route table into a multibit trie on this parser's device -> Lpm.  `routes`: an
        iterable of ("10.0.0.0/8", nexthop) / ("2001:db8::/32", nexthop) pairs, or a numpy array of
        schema.LPM_ROUTE_DTYPE (pkt_lpm_route_t).  `default_nexthop`: the next hop of a packet no route covers;
        `max_bytes`: the most the compiled table may take (0 = 1 GiB).  host=True gives the host handle
        (pkt_lpm_create_host: numpy arrays in and out, no device)."""
        return Lpm(None if host else self, routes, default_nexthop, max_bytes)

    def forwarder(self, adj, host=False):
        """pkt_fwd_create: an adjacency table on this parser's device -> Forwarder.  `adj`: an iterable of (dmac, smac,
        port[, mtu[, action]]) with the MACs as "aa:bb:cc:dd:ee:ff" strings or 6-byte objects, mtu 0 = no check and
        action one of schema.FWD_ACT_FORWARD / _DROP / _PUNT, or a numpy array of schema.FWD_ADJ_DTYPE
        (pkt_fwd_adj_t).  host=True gives the host form (pkt_fwd_host: numpy arrays in and out, no device)."""
        return Forwarder(None if host else self, adj)

    def nat(self, pool, ports=(1024, 65535), slots=1 << 16, static=(), host=False):
        """pkt_nat_create: a NAPT44 session table on this parser's device -> Nat.  `pool`: 1..64 outside IPv4 addresses
        ("a.b.c.d" strings or 4-byte objects); `ports`: the dynamic range (lo, hi); `slots`: the forward table's size, a
        power of two in 64..2^26 (at least twice the sessions expected); `static`: port forwards as (proto, in_addr,
        in_port, out_addr, out_port) with proto 6 / 17 / 1 or "tcp" / "udp" / "icmp", or a numpy array of
        schema.NAT_STATIC_DTYPE.  host=True gives the host handle (numpy arrays in and out, no device)."""
        return Nat(None if host else self, pool, ports, slots, static)

    def tunnels(self, entries, host=False):
        """pkt_tunnel_create: a table of 1..65536 VXLAN / GRE / IP-in-IP tunnels on this parser's device -> Tunnels,
        whose encap and decap take a parsed batch.  `entries`: a numpy array of schema.TUNNEL_ENTRY_DTYPE, or dicts
        as tunnel_entries takes them.  host=True gives the host handle (numpy arrays in and out, no device)."""
        return Tunnels(None if host else self, entries)

    def meters(self, cfgs, adjust=0, host=False):
        """pkt_meter_create: a table of 1..2^24 srTCM / trTCM token-bucket policers on this parser's device -> Meters.
        `cfgs`: a numpy array of schema.METER_CFG_DTYPE, or dicts as meter_cfgs takes them.  `adjust` is added to
        every packet's length (+20: preamble and gap, -14: L3 bytes).  host=True gives the host handle (numpy arrays
        in and out, no device)."""
        return Meters(None if host else self, cfgs, adjust)

    def fragment(self, batch, chain, mtu=1500, select=None, which_ip=0, only_split=False, plan_only=False,
                 out_cap=None, dst_bytes=None, hits=None, host=False, stream=None):
        """pkt_frag_batch: every packet whose L3 length is above its mtu becomes IPv4 fragments, every other packet
        that may pass goes through whole, all packed at 16-byte-aligned offsets of a new slab -> FragResult.  `mtu`: one
        number for the batch, or a uint16 [n] array (0 = no limit).  `select` (uint8 [n]): a packet whose byte is 0 is
        skipped.  `which_ip` as Lpm.lookup takes it.  only_split: a packet that fits gives no output.  plan_only: the
        sizing pass (PKT_FRAG_NO_WRITE): status, nfrag, first and the totals alone.  out_cap / dst_bytes: the
        capacities; without them a sizing pass runs first (one more host wait).  hits: True allocates zeroed uint64
        [10] per-status counters, an array passed in is accumulated into.  `batch` / `chain`: the forms Lpm.lookup
        takes.  host=True is pkt_frag_host: numpy arrays in and out, no device."""
        return _fragment(self, batch, chain, mtu, select, which_ip, only_split, plan_only, out_cap, dst_bytes, hits, host,
                         stream)

    def reassemble(self, batch, chain, select=None, which_ip=0, only_joined=False, plan_only=False, out_cap=None,
                   dst_bytes=None, hits=None, host=False, stream=None):
        """pkt_reasm_batch, the inverse of fragment: the IPv4 fragments of the batch are grouped by (src, dst, protocol,
        identification) and every datagram that is complete in this batch is joined into one packet, at the place of
        its last-arriving fragment; packets that are no fragments go through whole -> ReasmResult, whose batch() the
        other calls take (parse it again for the joined datagrams' full chains).  `select` (uint8 [n]): a packet whose
        byte is 0 is skipped.  `which_ip` as Lpm.lookup takes it.  only_joined: a whole packet gives no output.
        plan_only: the sizing pass (PKT_REASM_NO_WRITE): status, out_index and the totals alone.  out_cap /
        dst_bytes: the capacities; without them a sizing pass runs first (one more host wait).  hits: True allocates
        zeroed uint64 [9] per-status counters, an array passed in is accumulated into.  `batch` / `chain`: the forms
        Lpm.lookup takes.  host=True is pkt_reasm_host: numpy arrays in and out, no device."""
        return _reassemble(self, batch, chain, select, which_ip, only_joined, plan_only, out_cap, dst_bytes, hits, host,
                           stream)

    def icmp_errors(self, batch, chain, reason=None, fwd_status=None, frag_status=None, mtu=0, src4=None, src6=None,
                    ttl=64, tos=0, max4=576, max6=1280, ident=0, select=None, which_ip=0, plan_only=False, out_cap=None,
                    dst_bytes=None, hits=None, host=False, stream=None):
        """pkt_icmp_err_batch: one ICMP (IPv4) or ICMPv6 (IPv6) error packet for every packet of the batch that was
        refused and may be answered, packed at 16-byte-aligned offsets of a new slab -> IcmpErrResult.  Exactly one of
        `reason` (an int for the batch or a uint8 [n] array of schema.ICMP_R_*), `fwd_status` (Forwarder.run's status
        array, read through schema.ICMP_MAP_FWD: TTL -> time exceeded, MTU -> too big, NO_ADJ -> net unreachable) and
        `frag_status` (fragment's, through schema.ICMP_MAP_FRAG: DF and IPV6 -> too big) is given.  `mtu`: the next
        hop's mtu a too-big error reports, one number or a uint16 [n] array.  src4 / src6: the router's addresses
        ("192.0.2.1", "2001:db8::1" or 4 / 16 bytes); an IP version without one is not answered.  ttl, tos, ident and
        max4 / max6 (the greatest datagram built) fill the new headers.  `select`, `which_ip`, plan_only, out_cap /
        dst_bytes, hits (uint64 [12]) and host=True are as fragment takes them.  The replies leave by the link the
        packets came in on (MACs swapped); to route them instead:

            r = fwd.run(batch, chain, lpm=lpm)
            e = p.icmp_errors(batch, chain, fwd_status=r["status"], mtu=adj_mtu[r["adj_index"]], src4="192.0.2.1")
            fwd.run(e.batch(), e.out_chain, lpm=lpm)"""
        return _icmp_errors(self, batch, chain, reason, fwd_status, frag_status, mtu, src4, src6, ttl, tos, max4, max6,
                            ident, select, which_ip, plan_only, out_cap, dst_bytes, hits, host, stream)

    def scanner(self, patterns, nocase=False, groups=None, actions=None, default=0, host=False):
        """pkt_scan_create: compile a set of byte strings (bytes or str, 1..64 bytes each, at most 8192 of them and
        131072 bytes in all) on this parser's device -> Scanner.  `nocase`: one bool for the set or one per pattern
        (ASCII letters compare without case).  `groups`: one number 0..63 per pattern, the bit of "matched" it sets
        (default 0).  `actions`: one uint32 per pattern (default 1); a packet's action is that of its lowest
        occurring pattern, `default` where nothing occurs, and "sel" is action != 0.  host=True gives the host handle
        (pkt_scan_create_host: numpy arrays in and out, no device)."""
        return Scanner(None if host else self, patterns, nocase, groups, actions, default)

    def reorder(self, perm, slab=None, stride=None, n=None, offsets=None, lens=None, columns=None, start=None,
                nseg=None, slot=None, m=None, out=None, stream=None):
        """pkt_reorder_batch: packets and columns gathered by `perm` (uint32 device tensor: Dispatcher.run's, or
        any index list; an entry >= n is an empty position) -> {"slab": uint8 [m * slot] or None, "slot", "lens":
        uint32 [m] (min(length, slot)), "m", "columns": {name: tensor}, "start", "nseg"}.  `slab` (with stride /
        offsets / lens as Parser.parse takes them; None = columns only, then pass n) is the source batch; `slot`
        (a multiple of 16; default: a fixed-stride source's stride, rounded up) the bytes each packet gets; `columns`
        a dict of source columns (any of pkt_out_t's, e.g. a parse's result) to gather.  `start` (uint64 device
        tensor, Dispatcher.run's) with nseg (default: its length - 2, the kept buckets) lays the slot columns
        hdr_type / hdr_off out per segment, so that every segment is a batch of its own (pktgpu.segments), and
        leaves positions at or past start[nseg] (the dropped tail) unwritten: the freshly allocated outputs
        hold zeros there.  Without `start` the slot columns come out as [16][m].  `out`: a previous result to
        write into.  Asynchronous on `stream`."""
        torch = _torch()
        assert perm.dtype == torch.uint32 and perm.is_cuda and perm.is_contiguous()
        m = perm.numel() if m is None else int(m)
        if slab is not None:
            b = self._batch(slab, n, stride, offsets, lens)
        else:
            b = self._lib.PktBatch()
            b.n = int(n)
        if start is not None:
            assert start.dtype == torch.uint64 and start.is_cuda and start.is_contiguous()
            nseg = start.numel() - 2 if nseg is None else int(nseg)
        else:
            nseg = 0
        cols = dict(columns or {})
        if out is None:
            out = {"slab": None, "slot": 0, "lens": None, "m": m, "columns": {}, "start": start, "nseg": nseg}
            if slab is not None:
                if slot is None:
                    if not stride:
                        raise ValueError("reorder: an indexed source needs a slot")
                    slot = (max(16, int(stride)) + 15) // 16 * 16
                out["slot"] = int(slot)
                out["slab"] = torch.zeros(m * int(slot), dtype=torch.uint8, device=self.torch_device)
                out["lens"] = torch.zeros(m, dtype=torch.uint32, device=self.torch_device)
            for c, t in cols.items():
                shp = schema.column_shape(c, m)
                if shp[0] == schema.MAX_HDRS and len(shp) == 2 and nseg:
                    shp = (schema.MAX_HDRS * m,)
                out["columns"][c] = torch.zeros(shp, dtype=t.dtype, device=self.torch_device)
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None  # noqa: E731
        ci, co = self._lib.PktOut(), self._lib.PktOut()
        for c, t in cols.items():
            assert t.is_cuda and t.is_contiguous() and t.dtype == _tdtype(schema.column_dtype(c)), c
            setattr(ci, c, ptr(t))
            setattr(co, c, ptr(out["columns"][c]))
        dst = out["slab"] if slab is not None else None
        self._check(self._L.pkt_reorder_batch(self._ctx, ctypes.byref(b), ctypes.byref(ci), ptr(perm), m, ptr(start),
                                              nseg, ptr(dst), dst.numel() if dst is not None else 0, out["slot"],
                                              ptr(out["lens"]) if dst is not None else None, ctypes.byref(co),
                                              self._stream(stream)), "pkt_reorder_batch")
        return out

    def pcap_index_device_timed(self, buf, offsets, lens, stream=None):
        """pkt_pcap_index_device_timed into the caller's device `offsets` / `lens` (cap = their
        length): (record count, [guess, scan, emit] kernel ms from HIP events between them)."""
        n = ctypes.c_uint64()
        ms = (ctypes.c_float * 3)()
        self._check(self._L.pkt_pcap_index_device_timed(self._ctx, buf.data_ptr(), buf.numel(), offsets.data_ptr(),
                                                        lens.data_ptr(), offsets.numel(), ctypes.byref(n),
                                                        self._stream(stream), ms), "pkt_pcap_index_device_timed")
        return n.value, [ms[0], ms[1], ms[2]]


def pcap_index(buf):
    """(offsets uint64, lens uint32) of a tests/pcap.rs-format buffer, via the C ABI."""
    from . import _lib
    L = _lib.load()
    a = np.ascontiguousarray(np.frombuffer(buf, np.uint8) if isinstance(buf, (bytes, bytearray)) else buf)
    n = ctypes.c_uint64()
    rc = L.pkt_pcap_index(a.ctypes.data, a.size, None, None, 0, ctypes.byref(n))
    if rc != 0:
        raise ValueError("bad pcap")
    offs = np.zeros(n.value, np.uint64)
    lens = np.zeros(n.value, np.uint32)
    rc = L.pkt_pcap_index(a.ctypes.data, a.size, offs.ctypes.data, lens.ctypes.data, n.value,
                          ctypes.byref(n))
    if rc != 0:
        raise ValueError("bad pcap")
    return offs, lens


def pcap_write(slab, offsets=None, lens=None, stride=None, select=None, snaplen=0, ts=(0, 0), dst=None,
               n=None):
    """pkt_pcap_write_host over numpy arrays (no device): the selected packets of a host batch as a
    tests/pcap.rs capture -> (capture uint8, n, offsets uint64, lens uint32, src_index uint32).
    Arguments as Parser.pcap_write, with numpy arrays; `dst` (uint8, optional) receives the bytes,
    and one that is too small raises with the size needed."""
    from . import _lib
    L = _lib.load()
    slab = np.ascontiguousarray(slab, np.uint8).reshape(-1)
    b = _lib.PktBatch()
    b.slab = slab.ctypes.data if slab.size else None
    b.slab_len = slab.size
    if offsets is not None:
        offsets = np.ascontiguousarray(offsets, np.uint64)
        lens = np.ascontiguousarray(lens, np.uint32)
        n = offsets.size if n is None else n
        b.offsets = offsets.ctypes.data if n else None
    else:
        n = slab.size // stride if n is None else n
        if lens is not None:
            lens = np.ascontiguousarray(lens, np.uint32)
    if lens is not None:
        b.lens = lens.ctypes.data if n else None
    b.stride = stride or 0
    b.n = int(n)
    if select is not None:
        select = np.ascontiguousarray(np.asarray(select) != 0).view(np.uint8)
        assert select.size == n
    tv, tsp = [0, 0], [None, None]
    for k in range(2):
        if isinstance(ts[k], (int, np.integer)):
            tv[k] = int(ts[k])
        else:
            tsp[k] = np.ascontiguousarray(ts[k], np.uint32)
            assert tsp[k].size == n
    if dst is None:
        cap = min(65535, int(snaplen)) if snaplen else 65535
        data = n * min(int(stride), cap) if lens is None else int(np.minimum(lens[:n].astype(np.int64), cap).sum())
        dst = np.empty(24 + 16 * n + data, np.uint8)
    assert dst.dtype == np.uint8 and dst.flags.c_contiguous
    ro, rl, si = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    ptr = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
    total, cnt = ctypes.c_uint64(), ctypes.c_uint64()
    rc = L.pkt_pcap_write_host(ctypes.byref(b), ptr(select), int(snaplen), tv[0], tv[1], ptr(tsp[0]), ptr(tsp[1]),
                               ptr(dst), dst.size, ptr(ro), ptr(rl), ptr(si), ctypes.byref(total), ctypes.byref(cnt))
    if rc != 0 and total.value > dst.size:
        raise ValueError(f"pcap_write: dst holds {dst.size} bytes, the capture needs {total.value} "
                         f"({cnt.value} records)")
    if rc != 0:
        raise ValueError(f"pkt_pcap_write_host failed ({rc})")
    k = cnt.value
    return dst[:total.value], k, ro[:k], rl[:k], si[:k]


CMP_EQUAL, CMP_LEN, CMP_BYTES = 0, 1, 2


def _cmp_specs(lib, ignore):
    k = len(ignore)
    sp = (lib.PktFieldSpec * max(1, k))()
    for i, (t, occ, s, e) in enumerate(ignore):
        t = HDR_ID[t] if isinstance(t, str) else int(t)
        sp[i] = lib.PktFieldSpec(t, occ, s, e, 0)
    return sp, k


def _cmp_summary(sm):
    return {"n_equal": sm.n_equal, "n_len": sm.n_len, "n_bytes": sm.n_bytes, "first_bad": sm.first_bad}


def _host_batch(lib, d):
    """A PktBatch over the numpy arrays of a batch dict (and the arrays, to keep them alive)."""
    slab = np.ascontiguousarray(d["slab"], np.uint8).reshape(-1)
    offsets, lens, stride, n = d.get("offsets"), d.get("lens"), d.get("stride"), d.get("n")
    b = lib.PktBatch()
    b.slab = slab.ctypes.data if slab.size else None
    b.slab_len = slab.size
    if offsets is not None:
        offsets = np.ascontiguousarray(offsets, np.uint64)
        lens = np.ascontiguousarray(lens, np.uint32)
        n = offsets.size if n is None else n
        b.offsets = offsets.ctypes.data if n else None
    else:
        n = slab.size // stride if n is None else n
        if lens is not None:
            lens = np.ascontiguousarray(lens, np.uint32)
    if lens is not None:
        b.lens = lens.ctypes.data if n else None
    b.stride = stride or 0
    b.n = int(n)
    return b, (slab, offsets, lens)


def compare(a, b, ignore=(), chain=None):
    """pkt_compare_host over numpy arrays (no device): Parser.compare's arguments with numpy arrays
    in the batch dicts and in `chain` -> (result uint8, matching uint32, first_diff uint32, summary)."""
    from . import _lib
    L = _lib.load()
    (ba, keep_a), (bb, keep_b) = _host_batch(_lib, a), _host_batch(_lib, b)
    n = ba.n
    sp, k = _cmp_specs(_lib, ignore)
    ch = None
    if chain is not None:
        cols = (np.ascontiguousarray(chain["n_hdrs"], np.uint8), np.ascontiguousarray(chain["hdr_type"], np.uint8),
                np.ascontiguousarray(chain["hdr_off"], np.uint16))
        ch = _lib.PktChain(*[c.ctypes.data for c in cols])
    res, mt, fd = np.zeros(n, np.uint8), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    sm = _lib.PktCmpSummary()
    ptr = lambda x: x.ctypes.data if x.size else None  # noqa: E731
    rc = L.pkt_compare_host(ctypes.byref(ba), ctypes.byref(bb), ctypes.byref(ch) if ch is not None else None, sp, k,
                            ptr(res), ptr(mt), ptr(fd), ctypes.byref(sm))
    if rc != 0:
        raise ValueError(f"pkt_compare_host failed ({rc})")
    return res, mt, fd, _cmp_summary(sm)


EDIT_OK, EDIT_SKIPPED, EDIT_DEPTH, EDIT_NO_ROOM = 0, 1, 2, 3
EDIT_POP, EDIT_REMOVE_AT, EDIT_REMOVE_HDR, EDIT_INSERT = 0, 1, 2, 3
EDIT_END = 0xFF


def _edit_ops(lib, ops):
    """The op tuples of Parser.edit -> (PktEditOp array, count, hdr_data bytes)."""
    k = len(ops)
    arr = (lib.PktEditOp * max(1, k))()
    # hdr_data in LIST order where the program shows it (an insert at index 0 goes in front of the bytes so
    # far, any other behind them): headers that end up next to each other, as an encap's outer headers do,
    # are then one run of hdr_data, which the kernel copies as one segment
    pieces = []  # (op index, bytes)
    hid = lambda t: HDR_ID[t] if isinstance(t, str) else int(t)  # noqa: E731
    for i, op in enumerate(ops):
        kind = op[0]
        if kind == "pop":
            arr[i] = lib.PktEditOp(EDIT_POP, 0, 0, 0, 0)
        elif kind == "remove":
            arr[i] = lib.PktEditOp(EDIT_REMOVE_AT, 0, int(op[1]), 0, 0)
        elif kind == "remove_hdr":
            arr[i] = lib.PktEditOp(EDIT_REMOVE_HDR, hid(op[1]), int(op[2]) if len(op) > 2 else 0, 0, 0)
        elif kind in ("insert", "push"):
            t = hid(op[1])
            size = HDR_SIZES[t] if 0 < t < len(HDR_SIZES) else 0
            raw = bytes(op[2])
            if len(raw) < size:
                raise ValueError(f"edit: {op[1]!r} needs {size} bytes, got {len(raw)}")
            index = EDIT_END if kind == "push" else (int(op[3]) if len(op) > 3 else 0)
            arr[i] = lib.PktEditOp(EDIT_INSERT, t, index, 0, 0)
            pieces.insert(0 if index == 0 else len(pieces), (i, raw[:size]))
        else:
            raise ValueError(f"edit: unknown op {kind!r}")
    data = b""
    for i, raw in pieces:
        arr[i].data_off = len(data)
        data += raw
    return arr, k, data


def _edit_slot(slot, stride, dst_offsets, arr, k):
    if slot is not None:
        return int(slot)
    if not stride:
        raise ValueError("edit: an indexed batch needs `slot`, the room of every destination packet")
    grow = sum(HDR_SIZES[arr[i].hdr_type] for i in range(k) if arr[i].kind == EDIT_INSERT and arr[i].hdr_type < len(HDR_SIZES))
    return int(stride) + (grow + 15) // 16 * 16


def edit(slab, parsed, ops, stride=None, n=None, offsets=None, lens=None, select=None, dst=None, dst_offsets=None,
         slot=None):
    """pkt_edit_host over numpy arrays (no device): Parser.edit's arguments with numpy arrays ->
    (dst uint8, out_len uint32, status uint8, chain {column: array})."""
    from . import _lib
    L = _lib.load()
    b, keep = _host_batch(_lib, dict(slab=slab, stride=stride, n=n, offsets=offsets, lens=lens))
    n = b.n
    arr, k, data = _edit_ops(_lib, ops)
    slot = _edit_slot(slot, stride, dst_offsets, arr, k)
    need = ("status", "n_hdrs", "hdr_type", "hdr_off", "payload_off", "payload_len")
    cols = {c: np.ascontiguousarray(parsed[c], schema.column_dtype(c)) for c in need}
    po = _lib.PktOut()
    for c in need:
        setattr(po, c, cols[c].ctypes.data if cols[c].size else None)
    if select is not None:
        select = np.ascontiguousarray(np.asarray(select) != 0).view(np.uint8)
        assert select.size == n
    if dst is None:
        if dst_offsets is not None:
            raise ValueError("edit: dst_offsets needs dst")
        dst = np.zeros(n * slot, np.uint8)
    assert dst.dtype == np.uint8 and dst.flags.c_contiguous
    if dst_offsets is not None:
        dst_offsets = np.ascontiguousarray(dst_offsets, np.uint64)
        assert dst_offsets.size == n
    out_len, status = np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    chain = {c: np.zeros(schema.column_shape(c, n), schema.column_dtype(c)) for c in schema.columns_of(["chain"])}
    oc = _lib.PktOut()
    for c, a in chain.items():
        setattr(oc, c, a.ctypes.data if a.size else None)
    ptr = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
    rc = L.pkt_edit_host(ctypes.byref(b), ctypes.byref(po), arr, k, data, len(data), ptr(select), ptr(dst), dst.size,
                         ptr(dst_offsets), slot, ptr(out_len), ptr(status), ctypes.byref(oc))
    if rc != 0:
        raise ValueError(f"pkt_edit_host failed ({rc})")
    return dst, out_len, status, chain


L4_OK, L4_BAD, L4_UNCHECKED, L4_ABSENT, L4_NO_IP, L4_SPAN, L4_FRAGMENT = range(7)
L4_LAST = schema.L4_LAST


def l4_checksum(slab, chain, which=0, update=False, keep_zero_udp=False, stride=None, n=None, offsets=None, lens=None):
    """pkt_l4_checksum_host over numpy arrays (no device): Parser.l4_checksum's arguments with numpy arrays
    -> {"calc", "stored", "status"}.  update=True writes into `slab` itself, which must then be a
    writable C-contiguous uint8 array."""
    from . import _lib
    L = _lib.load()
    if update:
        assert isinstance(slab, np.ndarray) and slab.dtype == np.uint8 and slab.flags.c_contiguous and slab.flags.writeable
    b, keep = _host_batch(_lib, dict(slab=slab, stride=stride, n=n, offsets=offsets, lens=lens))
    cols = (np.ascontiguousarray(chain["n_hdrs"], np.uint8), np.ascontiguousarray(chain["hdr_type"], np.uint8),
            np.ascontiguousarray(chain["hdr_off"], np.uint16))
    ch = _lib.PktChain(*[c.ctypes.data for c in cols])
    flags = (schema.L4_UPDATE if update else 0) | (schema.L4_KEEP_ZERO_UDP if keep_zero_udp else 0)
    calc, stored, status = np.zeros(b.n, np.uint16), np.zeros(b.n, np.uint16), np.zeros(b.n, np.uint8)
    ptr = lambda a: a.ctypes.data if a.size else None  # noqa: E731
    rc = L.pkt_l4_checksum_host(ctypes.byref(b), ctypes.byref(ch), int(which), flags, ptr(calc), ptr(stored), ptr(status))
    if rc != 0:
        raise ValueError(f"pkt_l4_checksum_host failed ({rc})")
    return {"calc": calc, "stored": stored, "status": status}


FLOW_OK, FLOW_NO_IP, FLOW_SPAN = range(3)
FLOW_LAST = schema.FLOW_LAST
FLOW_UPD_OK, FLOW_UPD_SKIPPED, FLOW_UPD_COLLISION, FLOW_UPD_FULL = range(4)
FLOW_NONE = schema.FLOW_NONE


def _rss_key(rss_key):
    """A 40-byte Toeplitz key as a ctypes buffer (None stays None)."""
    if rss_key is None:
        return None
    raw = bytes(rss_key)
    if len(raw) != 40:
        raise ValueError(f"rss_key: 40 bytes, got {len(raw)}")
    return ctypes.create_string_buffer(raw, 40)


def flow_keys(slab, chain, which_ip=FLOW_LAST, symmetric=False, ports=True, seed=0, rss_key=None, stride=None, n=None,
              offsets=None, lens=None):
    """pkt_flow_key_host over numpy arrays (no device): Parser.flow_keys's arguments with numpy arrays ->
    the same dict of numpy arrays, which a host FlowTable (FlowTable(None, slots)) takes."""
    from . import _lib
    L = _lib.load()
    b, keep = _host_batch(_lib, dict(slab=slab, stride=stride, n=n, offsets=offsets, lens=lens))
    cols = (np.ascontiguousarray(chain["n_hdrs"], np.uint8), np.ascontiguousarray(chain["hdr_type"], np.uint8),
            np.ascontiguousarray(chain["hdr_off"], np.uint16))
    ch = _lib.PktChain(*[c.ctypes.data for c in cols])
    flags = (schema.FLOW_SYMMETRIC if symmetric else 0) | (0 if ports else schema.FLOW_NO_PORTS)
    rk = _rss_key(rss_key)
    res = {"keys": np.zeros((b.n, 40), np.uint8), "hash": np.zeros(b.n, np.uint64), "rss": np.zeros(b.n, np.uint32),
           "dir": np.zeros(b.n, np.uint8), "plen": np.zeros(b.n, np.uint32), "status": np.zeros(b.n, np.uint8)}
    if rk is None:
        del res["rss"]
    ptr = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
    rc = L.pkt_flow_key_host(ctypes.byref(b), ctypes.byref(ch), int(which_ip), flags, int(seed), rk, ptr(res["keys"]),
                             ptr(res["hash"]), ptr(res.get("rss")), ptr(res["dir"]), ptr(res["plen"]), ptr(res["status"]))
    if rc != 0:
        raise ValueError(f"pkt_flow_key_host failed ({rc})")
    return res


MATCH_NONE = schema.MATCH_NONE
_MATCH_OPS = {"has": (schema.MATCH_HAS, 0), "not has": (schema.MATCH_HAS, schema.MATCH_NOT),
              "==": (schema.MATCH_EQ, 0), "!=": (schema.MATCH_EQ, schema.MATCH_NOT),
              "in": (schema.MATCH_RANGE, 0), "not in": (schema.MATCH_RANGE, schema.MATCH_NOT)}


def match_term(term):
    """One term of a match program as a PktMatchTerm (Parser.match_program's term forms; a PktMatchTerm is
    returned as it is)."""
    from . import _lib, fields
    if isinstance(term, _lib.PktMatchTerm):
        return term
    U64 = (1 << 64) - 1
    if term[0] == "len":
        _, op, lo, hi = term
        if op not in ("in", "not in"):
            raise ValueError(f"len term: op {op!r} is neither 'in' nor 'not in'")
        return _lib.PktMatchTerm(_lib.PktFieldSpec(), schema.MATCH_LEN, _MATCH_OPS[op][1], 0, 0, int(lo) & U64, int(hi) & U64)
    hdr, occ, field, op = term[:4]
    if op not in _MATCH_OPS:
        raise ValueError(f"unknown match op {op!r}")
    t = HDR_ID[hdr] if isinstance(hdr, str) else int(hdr)
    kind, flags = _MATCH_OPS[op]
    if kind == schema.MATCH_HAS:
        start = end = a = b = 0
    else:
        start, end = fields.FIELDS[t][field] if isinstance(field, str) else field
        a = int(term[4])
        if kind == schema.MATCH_EQ:
            b = int(term[5]) if len(term) > 5 else U64
        else:
            b = int(term[5])
    return _lib.PktMatchTerm(_lib.PktFieldSpec(t, int(occ), int(start), int(end), 0), kind, flags, 0, 0, a & U64, b & U64)


def match_arrays(rules):
    """(PktMatchTerm array, nterms, PktMatchRule array, nrules) of Parser.match_program's `rules`: each rule's
    terms laid out one run after the other.  A (term array, rule array) pair passes through."""
    from . import _lib
    if isinstance(rules, tuple) and len(rules) == 2 and isinstance(rules[1], ctypes.Array):
        return rules[0], len(rules[0]) if rules[0] is not None else 0, rules[1], len(rules[1])
    terms, rr = [], []
    for action, tl in rules:
        rr.append((len(terms), len(tl), int(action)))
        terms.extend(match_term(t) for t in tl)
    ta = (_lib.PktMatchTerm * max(1, len(terms)))(*terms)
    ra = (_lib.PktMatchRule * max(1, len(rr)))(*[_lib.PktMatchRule(*r) for r in rr])
    return ta, len(terms), ra, len(rr)


class MatchProgram:
    """pkt_match_t: a compiled first-match rule table on a parser's device (Parser.match_program)."""

    def __init__(self, parser, rules, default=0):
        self.parser = parser
        self._L = parser._L
        ta, self.nterms, ra, self.nrules = match_arrays(rules)
        self.default = int(default)
        h = ctypes.c_void_p()
        parser._check(self._L.pkt_match_create(parser._ctx, ta, self.nterms, ra, self.nrules, self.default,
                                               ctypes.byref(h)), "pkt_match_create")
        self._m = h

    def close(self):
        if getattr(self, "_m", None):
            self._L.pkt_match_destroy(self._m)
            self._m = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def match(slab, chain, rules, default=0, stride=None, n=None, offsets=None, lens=None,
          outputs=("rule", "action", "select", "matched"), hits=None, bytes=None):
    """pkt_match_host over numpy arrays (no device): Parser.match's arguments with numpy arrays and the rules
    themselves in place of a MatchProgram -> the same dict of numpy arrays.  hits / bytes: True allocates zeroed
    uint64 [nrules + 1] counters; an array passed in (uint64, C-contiguous) is accumulated into."""
    from . import _lib
    L = _lib.load()
    ta, nterms, ra, nrules = match_arrays(rules)
    b, keep = _host_batch(_lib, dict(slab=slab, stride=stride, n=n, offsets=offsets, lens=lens))
    cols = (np.ascontiguousarray(chain["n_hdrs"], np.uint8), np.ascontiguousarray(chain["hdr_type"], np.uint8),
            np.ascontiguousarray(chain["hdr_off"], np.uint16))
    ch = _lib.PktChain(*[c.ctypes.data for c in cols])
    dts = {"rule": np.uint8, "action": np.uint32, "select": np.uint8, "matched": np.uint64}
    res = {k: np.zeros(b.n, dts[k]) for k in outputs}
    for name, c in (("hits", hits), ("bytes", bytes)):
        if c is True:
            c = np.zeros(nrules + 1, np.uint64)
        if c is not None and c is not False:
            assert c.dtype == np.uint64 and c.size == nrules + 1 and c.flags.c_contiguous
            res[name] = c
    ptr = lambda k: res[k].ctypes.data if k in res and res[k].size else None  # noqa: E731
    rc = L.pkt_match_host(ta, nterms, ra, nrules, int(default), ctypes.byref(b), ctypes.byref(ch), ptr("rule"),
                          ptr("action"), ptr("select"), ptr("matched"), ptr("hits"), ptr("bytes"))
    if rc != 0:
        raise ValueError(f"pkt_match_host failed ({rc})")
    return res


DISPATCH_DROP = schema.DISPATCH_DROP
_DISPATCH_OUT = (("bucket", np.uint16), ("perm", np.uint32), ("rank", np.uint32), ("start", np.uint64))


def _dispatch_table(table):
    """(uint16 array or None, its length) of an indirection table given as integers."""
    if table is None:
        return None, 0
    t = np.asarray(table)
    if t.size and (t.min() < 0 or t.max() > 0xFFFF):
        raise ValueError("dispatch: a table entry outside 0..0xFFFF")
    return np.ascontiguousarray(t, np.uint16).reshape(-1), int(t.size)


class Dispatcher:
    """pkt_dispatch_t: a stable bucket partition on a parser's device (Parser.dispatcher).  One run at a time:
    the runs share the handle's scratch."""

    def __init__(self, parser, nbuckets, table=None, max_n=1 << 20):
        self.parser = parser
        self._L = parser._L
        self.nbuckets, self.max_n = int(nbuckets), int(max_n)
        tab, tlen = _dispatch_table(table)
        h = ctypes.c_void_p()
        parser._check(self._L.pkt_dispatch_create(parser._ctx, self.nbuckets, tab.ctypes.data if tab is not None else
                                                  None, tlen, self.max_n, ctypes.byref(h)), "pkt_dispatch_create")
        self._d = h

    def run(self, key, select=None, outputs=("bucket", "perm", "rank", "start"), n=None, stream=None):
        """pkt_dispatch_batch over `key` (uint32 device tensor [n]: flow_keys' "rss", match's "action", ...) and
        an optional `select` (uint8 / bool device tensor: 0 drops the packet) -> a dict of the `outputs` asked
        for among "bucket" (uint16: the packet's bucket, pktgpu.DISPATCH_DROP = dropped), "perm" (uint32:
        perm[pos] = source index, buckets in order, source order within a bucket, the dropped last), "rank"
        (uint32: its inverse) and "start" (uint64 [nbuckets + 2]: bucket b is positions [start[b], start[b + 1]),
        start[nbuckets] the kept count).  Asynchronous on `stream`."""
        torch = _torch()
        p = self.parser
        assert key.dtype == torch.uint32 and key.is_cuda and key.is_contiguous()
        n = key.numel() if n is None else int(n)
        if select is not None:
            if select.dtype == torch.bool:
                select = select.view(torch.uint8)
            assert select.dtype == torch.uint8 and select.is_cuda and select.numel() >= n
        res = {}
        for name, dt in _DISPATCH_OUT:
            if name in outputs:
                res[name] = torch.empty(self.nbuckets + 2 if name == "start" else n, dtype=_tdtype(dt),
                                        device=p.torch_device)
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None  # noqa: E731
        p._check(self._L.pkt_dispatch_batch(self._d, ptr(key), ptr(select), n, *[ptr(res.get(k)) for k, _ in
                                            _DISPATCH_OUT], p._stream(stream)), "pkt_dispatch_batch")
        return res

    def close(self):
        if getattr(self, "_d", None):
            self._L.pkt_dispatch_destroy(self._d)
            self._d = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def dispatch(key, nbuckets, table=None, select=None, outputs=("bucket", "perm", "rank", "start"), n=None):
    """pkt_dispatch_host over numpy arrays (no device): Dispatcher.run's arguments with the definition in place of
    a handle -> the same dict of numpy arrays."""
    from . import _lib
    L = _lib.load()
    key = np.ascontiguousarray(key, np.uint32).reshape(-1)
    n = key.size if n is None else int(n)
    tab, tlen = _dispatch_table(table)
    if select is not None:
        select = np.ascontiguousarray(np.asarray(select) != 0).view(np.uint8)
    res = {name: np.zeros(int(nbuckets) + 2 if name == "start" else n, dt) for name, dt in _DISPATCH_OUT
           if name in outputs}
    ptr = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
    rc = L.pkt_dispatch_host(int(nbuckets), tab.ctypes.data if tab is not None else None, tlen, ptr(key), ptr(select), n,
                             *[ptr(res.get(k)) for k, _ in _DISPATCH_OUT])
    if rc != 0:
        raise ValueError(f"pkt_dispatch_host failed ({rc})")
    return res


def reorder(perm, slab=None, stride=None, n=None, offsets=None, lens=None, columns=None, start=None, nseg=None,
            slot=None, m=None):
    """pkt_reorder_host over numpy arrays (no device): Parser.reorder's arguments with numpy arrays -> the same
    dict of numpy arrays."""
    from . import _lib
    L = _lib.load()
    perm = np.ascontiguousarray(perm, np.uint32).reshape(-1)
    m = perm.size if m is None else int(m)
    keep = None
    if slab is not None:
        b, keep = _host_batch(_lib, dict(slab=slab, stride=stride, n=n, offsets=offsets, lens=lens))
    else:
        b = _lib.PktBatch()
        b.n = int(n)
    if start is not None:
        start = np.ascontiguousarray(start, np.uint64).reshape(-1)
        nseg = start.size - 2 if nseg is None else int(nseg)
    else:
        nseg = 0
    out = {"slab": None, "slot": 0, "lens": None, "m": m, "columns": {}, "start": start, "nseg": nseg}
    if slab is not None:
        if slot is None:
            if not stride:
                raise ValueError("reorder: an indexed source needs a slot")
            slot = (max(16, int(stride)) + 15) // 16 * 16
        out["slot"] = int(slot)
        out["slab"] = _aligned_zeros(m * int(slot))
        out["lens"] = np.zeros(m, np.uint32)
    ptr = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
    ci, co, held = _lib.PktOut(), _lib.PktOut(), []
    for c, a in (columns or {}).items():
        a = np.ascontiguousarray(a, schema.column_dtype(c))
        shp = schema.column_shape(c, m)
        if shp[0] == schema.MAX_HDRS and len(shp) == 2 and nseg:
            shp = (schema.MAX_HDRS * m,)
        out["columns"][c] = np.zeros(shp, a.dtype)
        held.append(a)
        setattr(ci, c, ptr(a))
        setattr(co, c, ptr(out["columns"][c]))
    dst = out["slab"]
    rc = L.pkt_reorder_host(ctypes.byref(b), ctypes.byref(ci), ptr(perm), m, ptr(start), nseg, ptr(dst),
                            dst.size if dst is not None else 0, out["slot"], ptr(out["lens"]), ctypes.byref(co))
    if rc != 0:
        raise ValueError(f"pkt_reorder_host failed ({rc})")
    return out


def _aligned_zeros(nbytes, align=16):
    """A zeroed uint8 array of nbytes whose first byte is `align`-byte aligned."""
    raw = np.zeros(nbytes + align, np.uint8)
    o = (-raw.ctypes.data) % align
    return raw[o:o + nbytes]


def segments(start, reordered):
    """The per-bucket batches of a segmented Parser.reorder (or pktgpu.reorder) result: one small copy of
    `start` to the host, then for each of the nseg buckets a dict {"slab", "stride", "n", "lens", "chain"}, views
    into the reordered tensors.  slab / stride / n / lens are the keyword arguments Parser.pcap_write takes, and
    with "chain" (the bucket's n_hdrs, hdr_type [16][n], hdr_off [16][n]; None when they were not gathered) the
    ones Parser.match, flow_keys and l4_checksum take: `p.match(prog=prog, **seg)`."""
    st = start.cpu().numpy() if hasattr(start, "cpu") else np.asarray(start)
    m, slot, nseg = reordered["m"], reordered["slot"], reordered["nseg"]
    cols = reordered["columns"]
    out = []
    for s in range(nseg):
        s0, s1 = min(int(st[s]), m), min(int(st[s + 1]), m)
        ns = max(0, s1 - s0)
        seg = {"slab": reordered["slab"][s0 * slot:(s0 + ns) * slot] if reordered["slab"] is not None else None,
               "stride": slot, "n": ns,
               "lens": reordered["lens"][s0:s0 + ns] if reordered["lens"] is not None else None, "chain": None}
        if all(c in cols for c in ("n_hdrs", "hdr_type", "hdr_off")):
            seg["chain"] = {"n_hdrs": cols["n_hdrs"][s0:s0 + ns]}
            for c in ("hdr_type", "hdr_off"):
                seg["chain"][c] = cols[c].reshape(-1)[schema.MAX_HDRS * s0:schema.MAX_HDRS * (s0 + ns)].reshape(
                    schema.MAX_HDRS, ns)
        out.append(seg)
    return out


class FlowTable:
    """pkt_flow_table_*: per-flow packet and byte counters that persist from one batch (or stream window) to
    the next.  FlowTable(parser, slots) lives on the parser's device and takes Parser.flow_keys's dict of
    device tensors; FlowTable(None, slots) is the host table over pktgpu.flow_keys's numpy arrays.  `slots`: a
    power of two in 64..2^28, 128 bytes each; the table only grows until clear().

        keys = p.flow_keys(slab, chain, symmetric=True, offsets=offs, lens=lens)
        flow_id, upd = table.update(keys, base=records_so_far)
        table.flows()   # {"key", "first", "pkts", "bytes"} sorted by first
    """

    def __init__(self, parser, slots):
        from . import _lib
        self._lib = _lib
        self._L = _lib.load()
        self.parser = parser
        h = ctypes.c_void_p()
        if parser is None:
            rc = self._L.pkt_flow_table_create_host(int(slots), ctypes.byref(h))
            if rc != 0:
                raise ValueError(f"pkt_flow_table_create_host({slots}) failed ({rc})")
        else:
            parser._check(self._L.pkt_flow_table_create(parser._ctx, int(slots), ctypes.byref(h)), "pkt_flow_table_create")
        self._t = h
        self.slots = int(slots)

    def _check(self, rc, what):
        if rc != 0:
            msg = self._L.pkt_flow_table_last_error(self._t)
            raise RuntimeError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")

    def _stream(self, stream):
        return None if self.parser is None else self.parser._stream(stream)

    def set_tag_bits(self, bits):
        """pkt_flow_table_set_tag_bits: the low `bits` (1..64) of the hash are the tag; on an empty table."""
        self._check(self._L.pkt_flow_table_set_tag_bits(self._t, int(bits)), "pkt_flow_table_set_tag_bits")

    def _update_args(self, keys, weight="plen", base=0, outputs=(True, True)):
        """The marshalled arguments of pkt_flow_table_update (after the table, before stream)."""
        host = self.parser is None
        k = keys["keys"]
        n = int(k.shape[0])
        if isinstance(weight, str):
            weight = keys[weight]
        cols = [k, keys["hash"], keys.get("dir"), weight, keys.get("status")]
        if host:
            dts = (np.uint8, np.uint64, np.uint8, np.uint32, np.uint8)
            cols = [None if c is None else np.ascontiguousarray(c, dt) for c, dt in zip(cols, dts)]
            out = (np.zeros(n, np.uint32) if outputs[0] else None, np.zeros(n, np.uint8) if outputs[1] else None)
            ptr = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
        else:
            torch = _torch()
            dts = (torch.uint8, torch.uint64, torch.uint8, torch.uint32, torch.uint8)
            for c, dt in zip(cols, dts):
                assert c is None or (c.is_cuda and c.dtype == dt and c.is_contiguous())
            dev = self.parser.torch_device
            out = (torch.empty(n, dtype=torch.uint32, device=dev) if outputs[0] else None,
                   torch.empty(n, dtype=torch.uint8, device=dev) if outputs[1] else None)
            ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None  # noqa: E731
        for c in cols[1:]:
            assert c is None or c.shape[0] == n
        args = (*[ptr(c) for c in cols], n, int(base), ptr(out[0]), ptr(out[1]))
        return args, out, cols

    def update(self, keys, weight="plen", base=0, stream=None):
        """pkt_flow_table_update with flow_keys's dict -> (flow_id uint32, upd_status uint8): FLOW_UPD_OK
        (counted; flow_id = its slot), _SKIPPED (status != 0), _COLLISION (its tag's entry holds another
        key), _FULL; flow_id is pktgpu.FLOW_NONE unless OK.  `weight`: the name of the dict's byte column
        ("plen"), an array of uint32, or None (bytes are not counted).  `base`: the global index of packet 0,
        at least the previous update's base + n (a stream: its released_records).  Asynchronous on `stream`."""
        args, out, keep = self._update_args(keys, weight, base)
        self._check(self._L.pkt_flow_table_update(self._t, *args, self._stream(stream)), "pkt_flow_table_update")
        return out

    def count(self, stream=None):
        """pkt_flow_table_count: the number of flows (waits for `stream`)."""
        k = ctypes.c_uint64()
        self._check(self._L.pkt_flow_table_count(self._t, ctypes.byref(k), self._stream(stream)), "pkt_flow_table_count")
        return k.value

    def export(self, cap=None, stream=None):
        """pkt_flow_table_export: (records in slot order as a schema.FLOW_RECORD_DTYPE array of min(cap,
        count) rows, count).  cap=None: every record."""
        if cap is None:
            cap = self.count(stream)
        cap = int(cap)
        k = ctypes.c_uint64()
        if self.parser is None:
            buf = np.zeros(cap * 80, np.uint8)
            p = buf.ctypes.data if cap else None
        else:
            torch = _torch()
            buf = torch.zeros(cap * 80, dtype=torch.uint8, device=self.parser.torch_device)
            p = buf.data_ptr() if cap else None
        self._check(self._L.pkt_flow_table_export(self._t, p, cap, ctypes.byref(k), self._stream(stream)),
                    "pkt_flow_table_export")
        if self.parser is not None:
            buf = buf.cpu().numpy()
        return buf.view(schema.FLOW_RECORD_DTYPE)[:min(cap, k.value)], k.value

    def flows(self, stream=None):
        """The records sorted by `first` (unique per flow: the order is the same from run to run) ->
        {"key": uint8 [k, 40], "first": uint64, "pkts": uint64 [k, 2], "bytes": uint64 [k, 2]}, numpy."""
        rec, _ = self.export(None, stream)
        rec = rec[np.argsort(rec["first"], kind="stable")]
        key = np.ascontiguousarray(rec["key"]).view(np.uint8).reshape(-1, 40)
        return {"key": key, "first": rec["first"].copy(), "pkts": rec["pkts"].copy(), "bytes": rec["bytes"].copy()}

    def clear(self, stream=None):
        """pkt_flow_table_clear: the empty table; `base` may start again from 0."""
        self._check(self._L.pkt_flow_table_clear(self._t, self._stream(stream)), "pkt_flow_table_clear")

    def close(self):
        if getattr(self, "_t", None):
            self._L.pkt_flow_table_destroy(self._t)
            self._t = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


LPM_NONE = schema.LPM_NONE
_LPM_OUT = (("route", np.uint32), ("nexthop", np.uint32), ("plen", np.uint8), ("status", np.uint8))


def lpm_routes(routes):
    """A route list as a C-contiguous array of schema.LPM_ROUTE_DTYPE (pkt_lpm_route_t): an iterable of
    ("10.0.0.0/8", nexthop) / ("2001:db8::/32", nexthop) pairs (strings or stdlib ipaddress networks; host bits
    must be zero), or such an array, which passes through."""
    import ipaddress
    if isinstance(routes, np.ndarray):
        if routes.dtype != schema.LPM_ROUTE_DTYPE:
            raise ValueError("lpm: a route array must have schema.LPM_ROUTE_DTYPE")
        return np.ascontiguousarray(routes).reshape(-1)
    routes = list(routes)
    arr = np.zeros(len(routes), schema.LPM_ROUTE_DTYPE)
    for i, (net, nh) in enumerate(routes):
        net = ipaddress.ip_network(net) if isinstance(net, str) else net
        raw = net.network_address.packed
        arr["addr"][i, :len(raw)] = np.frombuffer(raw, np.uint8)
        arr["ipver"][i] = net.version
        arr["plen"][i] = net.prefixlen
        arr["nexthop"][i] = int(nh)
    return arr


class Lpm:
    """pkt_lpm_t: a compiled longest-prefix-match route table (Parser.lpm).  Lpm(parser, routes) lives on the parser's
    device and takes and gives device tensors; Lpm(None, routes) is the host handle over numpy arrays (no device).

        lpm = p.lpm([("10.0.0.0/8", 1), ("10.1.0.0/16", 2), ("2001:db8::/32", 3)], default_nexthop=255)
        r = lpm.lookup(batch, chain)             # {"route", "nexthop", "plen", "status"}
        d = p.dispatcher(4).run(r["nexthop"])    # next hops 0..3 are queues, the rest is dropped
    """

    def __init__(self, parser, routes, default_nexthop=0, max_bytes=0):
        from . import _lib
        self._lib = _lib
        self._L = _lib.load()
        self.parser = parser
        self.routes = lpm_routes(routes)
        self.default_nexthop = int(default_nexthop)
        n = self.routes.size
        rp = self.routes.ctypes.data if n else None
        h = ctypes.c_void_p()
        if parser is None:
            rc = self._L.pkt_lpm_create_host(rp, n, self.default_nexthop, int(max_bytes), ctypes.byref(h))
            if rc != 0:
                msg = self._L.pkt_lpm_last_error(None)
                raise ValueError(f"pkt_lpm_create_host failed ({rc}): {msg.decode() if msg else ''}")
        else:
            parser._check(self._L.pkt_lpm_create(parser._ctx, rp, n, self.default_nexthop, int(max_bytes),
                                                 ctypes.byref(h)), "pkt_lpm_create")
        self._t = h

    def _check(self, rc, what):
        if rc != 0:
            msg = self._L.pkt_lpm_last_error(self._t)
            raise RuntimeError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")

    def _stream(self, stream):
        return None if self.parser is None else self.parser._stream(stream)

    def _outputs(self, n, outputs):
        """The output arrays asked for (torch on the device handle's device, numpy for a host handle) and their
        addresses in pkt_lpm_lookup_*'s order."""
        bad = set(outputs) - {k for k, _ in _LPM_OUT}
        if bad:
            raise ValueError(f"lpm: unknown outputs {sorted(bad)}")
        if self.parser is None:
            res = {k: np.zeros(n, dt) for k, dt in _LPM_OUT if k in outputs}
            ptr = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
        else:
            torch = _torch()
            res = {k: torch.empty(n, dtype=_tdtype(dt), device=self.parser.torch_device) for k, dt in _LPM_OUT
                   if k in outputs}
            ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None  # noqa: E731
        return res, [ptr(res.get(k)) for k, _ in _LPM_OUT]

    def lookup(self, batch, chain, which_ip=0, src=False, outputs=("route", "nexthop", "plen", "status"), stream=None):
        """pkt_lpm_lookup_batch: the longest matching route of every packet's destination (src=True: source)
        address -> a dict of the `outputs` asked for among "route" (uint32: the route's index in the table given
        to Parser.lpm, pktgpu.LPM_NONE = none), "nexthop" (uint32: the route's, else the default), "plen" (uint8:
        the route's length, 0xFF = none) and "status" (uint8: schema.LPM_OK / _NO_ROUTE / _NO_IP / _SPAN).
        `batch`: a dict with "slab" and "stride" / "n" / "offsets" / "lens" as Parser.parse takes them, or a
        (slab, offsets, lens) tuple (PcapStream.batch()'s); `chain`: the chain columns of a parse of it.  `which_ip`: the k-th IPv4 / IPv6
        header of the list, counted together from 0, or pktgpu.FLOW_LAST (the innermost).  Device tensors for a
        device handle, numpy arrays for a host handle.  Asynchronous on `stream`."""
        if isinstance(batch, (tuple, list)):
            batch = dict(zip(("slab", "offsets", "lens"), batch))
        g = lambda k: batch.get(k)  # noqa: E731
        if self.parser is None:
            b, keep = _host_batch(self._lib, batch)
            cols = (np.ascontiguousarray(chain["n_hdrs"], np.uint8), np.ascontiguousarray(chain["hdr_type"], np.uint8),
                    np.ascontiguousarray(chain["hdr_off"], np.uint16))
            ch = self._lib.PktChain(*[c.ctypes.data for c in cols])
        else:
            b = self.parser._batch(batch["slab"], g("n"), g("stride"), g("offsets"), g("lens"))
            ch = self.parser._chain(chain)
        res, ptrs = self._outputs(b.n, outputs)
        self._check(self._L.pkt_lpm_lookup_batch(self._t, ctypes.byref(b), ctypes.byref(ch), int(which_ip),
                                                 schema.LPM_SRC if src else 0, *ptrs, self._stream(stream)),
                    "pkt_lpm_lookup_batch")
        return res

    def lookup_keys(self, keys, status=None, src=False, outputs=("route", "nexthop", "plen", "status"), stream=None):
        """pkt_lpm_lookup_keys: the same over flow keys (uint8 [n, 40]: flow_keys' "keys", or its whole dict, whose
        "status" is then taken too): the address is the key's dst (src=True: src).  A packet whose `status` is not 0
        or whose key has no IP version is schema.LPM_SKIPPED."""
        if isinstance(keys, dict):
            status = keys.get("status") if status is None else status
            keys = keys["keys"]
        n = int(keys.shape[0])
        if self.parser is None:
            keys = np.ascontiguousarray(keys, np.uint8)
            status = None if status is None else np.ascontiguousarray(status, np.uint8)
            kp = keys.ctypes.data if n else None
            sp = status.ctypes.data if status is not None and n else None
        else:
            torch = _torch()
            assert keys.is_cuda and keys.dtype == torch.uint8 and keys.is_contiguous()
            assert status is None or (status.is_cuda and status.dtype == torch.uint8 and status.numel() >= n)
            kp = keys.data_ptr() if n else None
            sp = status.data_ptr() if status is not None and n else None
        res, ptrs = self._outputs(n, outputs)
        self._check(self._L.pkt_lpm_lookup_keys(self._t, kp, sp, n, schema.LPM_SRC if src else 0, *ptrs,
                                                self._stream(stream)), "pkt_lpm_lookup_keys")
        return res

    def info(self):
        """pkt_lpm_info -> {"routes_v4", "routes_v6", "nodes_v4", "nodes_v6", "depth_v4", "depth_v6", "bytes"}."""
        i = self._lib.PktLpmInfo()
        self._check(self._L.pkt_lpm_info(self._t, ctypes.byref(i)), "pkt_lpm_info")
        return {k: int(getattr(i, k)) for k, _ in i._fields_}

    def close(self):
        if getattr(self, "_t", None):
            self._L.pkt_lpm_destroy(self._t)
            self._t = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


(FWD_OK, FWD_SKIPPED, FWD_NO_IP, FWD_SPAN, FWD_NO_ETHER, FWD_TTL, FWD_NO_ADJ, FWD_DROP, FWD_PUNT, FWD_MTU) = range(10)
FWD_ACT_FORWARD, FWD_ACT_DROP, FWD_ACT_PUNT = schema.FWD_ACT_FORWARD, schema.FWD_ACT_DROP, schema.FWD_ACT_PUNT
FWD_NONE, FWD_KEEP_L2, FWD_NO_WRITE = schema.FWD_NONE, schema.FWD_KEEP_L2, schema.FWD_NO_WRITE
_FWD_OUT = (("status", np.uint8), ("port", np.uint32), ("adj_index", np.uint32))


def _mac(m):
    raw = bytes(int(x, 16) for x in m.split(":")) if isinstance(m, str) else bytes(m)
    if len(raw) != 6:
        raise ValueError(f"forwarder: a MAC address has 6 bytes, not {m!r}")
    return np.frombuffer(raw, np.uint8)


def fwd_adjacencies(adj):
    """An adjacency list as a C-contiguous array of schema.FWD_ADJ_DTYPE (pkt_fwd_adj_t): an iterable of (dmac,
    smac, port[, mtu[, action]]) tuples, or such an array, which passes through."""
    if isinstance(adj, np.ndarray):
        if adj.dtype != schema.FWD_ADJ_DTYPE:
            raise ValueError("forwarder: an adjacency array must have schema.FWD_ADJ_DTYPE")
        return np.ascontiguousarray(adj).reshape(-1)
    adj = list(adj)
    arr = np.zeros(len(adj), schema.FWD_ADJ_DTYPE)
    for i, (dmac, smac, port, *rest) in enumerate(adj):
        arr["dmac"][i], arr["smac"][i], arr["port"][i] = _mac(dmac), _mac(smac), int(port)
        arr["mtu"][i] = int(rest[0]) if rest else 0
        arr["action"][i] = int(rest[1]) if len(rest) > 1 else schema.FWD_ACT_FORWARD
    return arr


class Forwarder:
    """pkt_fwd_t: an adjacency table and the L3 forwarding rewrite over a routed batch (Parser.forwarder).
    Forwarder(parser, adj) lives on the parser's device and takes and gives device tensors; Forwarder(None, adj) is
    the host form over numpy arrays (pkt_fwd_host, no device).

        fwd = p.forwarder([("02:00:00:00:00:01", "02:00:00:00:00:fe", 0), ("02:00:00:00:00:02", "02:00:00:00:00:fe", 1, 1500)])
        r = fwd.run(batch, chain, lpm=lpm)         # {"status", "port", "adj_index"}; the OK packets are rewritten in place
        d = p.dispatcher(4).run(r["port"])         # what was not forwarded has port FWD_NONE and is dropped
    """

    def __init__(self, parser, adj):
        from . import _lib
        self._lib = _lib
        self._L = _lib.load()
        self.parser = parser
        self.adj = fwd_adjacencies(adj)
        self._f = None
        if parser is not None:
            h = ctypes.c_void_p()
            n = self.adj.size
            parser._check(self._L.pkt_fwd_create(parser._ctx, self.adj.ctypes.data if n else None, n, ctypes.byref(h)),
                          "pkt_fwd_create")
            self._f = h

    def run(self, batch, chain, nexthop=None, lpm=None, which_ip=0, keep_l2=False, write=True, select=None,
            outputs=("status", "port", "adj_index"), hits=None, bytes=None, stream=None):
        """pkt_fwd_batch: per packet, find the IP entry (`which_ip` as Lpm.lookup takes it) and the Ether entry before
        it, take the adjacency index from `nexthop` (uint32 [n]) or from `lpm` (an Lpm: the destination's route, fused
        into the same kernel) and, for a packet that may be forwarded, write the adjacency's MACs, decrement the ttl /
        hop limit and update the IPv4 checksum incrementally, IN PLACE in the batch's slab -> a dict of the `outputs`
        asked for among "status" (uint8: pktgpu.FWD_OK / _SKIPPED / _NO_IP / _SPAN / _NO_ETHER / _TTL / _NO_ADJ /
        _DROP / _PUNT / _MTU), "port" (uint32: the adjacency's port for an OK packet, else pktgpu.FWD_NONE) and
        "adj_index" (uint32).  keep_l2: no Ether entry is looked for and no MAC written; write=False: decide only.
        `select` (uint8 [n]): a packet whose byte is 0 is skipped.  hits / bytes: True allocates zeroed uint64 [10]
        per-status counters and returns them; an array passed in is accumulated into.  `batch` / `chain`: the forms
        Lpm.lookup takes.  Device tensors for a device handle, numpy arrays for the host form.  Asynchronous on
        `stream`."""
        bad = set(outputs) - {k for k, _ in _FWD_OUT}
        if bad:
            raise ValueError(f"forwarder: unknown outputs {sorted(bad)}")
        if isinstance(batch, (tuple, list)):
            batch = dict(zip(("slab", "offsets", "lens"), batch))
        g = lambda k: batch.get(k)  # noqa: E731
        host = self.parser is None
        if lpm is not None and (lpm.parser is None) != host:
            raise ValueError("forwarder: a device handle takes a device Lpm, the host form a host Lpm")
        flags = (schema.FWD_KEEP_L2 if keep_l2 else 0) | (0 if write else schema.FWD_NO_WRITE)
        nc = schema.FWD_STATUS_COUNT
        if host:
            slab = batch["slab"]
            if write and not (isinstance(slab, np.ndarray) and slab.dtype == np.uint8 and slab.flags.c_contiguous
                              and slab.flags.writeable):
                raise ValueError("forwarder: the host form rewrites batch['slab'] in place: a writeable C-contiguous uint8 array")
            b, keep = _host_batch(self._lib, batch)
            cols = (np.ascontiguousarray(chain["n_hdrs"], np.uint8), np.ascontiguousarray(chain["hdr_type"], np.uint8),
                    np.ascontiguousarray(chain["hdr_off"], np.uint16))
            ch = self._lib.PktChain(*[c.ctypes.data for c in cols])
            nexthop = None if nexthop is None else np.ascontiguousarray(nexthop, np.uint32)
            select = None if select is None else np.ascontiguousarray(np.asarray(select) != 0).view(np.uint8)
            res = {k: np.zeros(b.n, dt) for k, dt in _FWD_OUT if k in outputs}
            ptr = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
            zeros = lambda: np.zeros(nc, np.uint64)  # noqa: E731
            ok = lambda c: isinstance(c, np.ndarray) and c.dtype == np.uint64 and c.size == nc and c.flags.c_contiguous  # noqa: E731
        else:
            torch = _torch()
            b = self.parser._batch(batch["slab"], g("n"), g("stride"), g("offsets"), g("lens"))
            ch = self.parser._chain(chain)
            assert nexthop is None or (nexthop.is_cuda and nexthop.dtype == torch.uint32 and nexthop.is_contiguous()
                                       and nexthop.numel() >= b.n)
            assert select is None or (select.is_cuda and select.dtype == torch.uint8 and select.is_contiguous()
                                      and select.numel() >= b.n)
            dev = self.parser.torch_device
            res = {k: torch.empty(b.n, dtype=_tdtype(dt), device=dev) for k, dt in _FWD_OUT if k in outputs}
            ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None  # noqa: E731
            zeros = lambda: torch.zeros(nc, dtype=torch.uint64, device=dev)  # noqa: E731
            ok = lambda c: c.is_cuda and c.dtype == torch.uint64 and c.numel() == nc and c.is_contiguous()  # noqa: E731
        for name, c in (("hits", hits), ("bytes", bytes)):
            if c is True:
                c = zeros()
            if c is not None and c is not False:
                assert ok(c), f"forwarder: {name} is a contiguous uint64 [{nc}] array"
                res[name] = c
        args = (ctypes.byref(b), ctypes.byref(ch), int(which_ip), flags, None if lpm is None else lpm._t, ptr(nexthop),
                ptr(select), *[ptr(res.get(k)) for k, _ in _FWD_OUT], ptr(res.get("hits")), ptr(res.get("bytes")))
        if host:
            n = self.adj.size
            rc = self._L.pkt_fwd_host(self.adj.ctypes.data if n else None, n, *args)
            if rc != 0:
                raise ValueError(f"pkt_fwd_host failed ({rc})")
        else:
            self.parser._check(self._L.pkt_fwd_batch(self._f, *args, self.parser._stream(stream)), "pkt_fwd_batch")
        return res

    def close(self):
        if getattr(self, "_f", None):
            self._L.pkt_fwd_destroy(self._f)
            self._f = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


(NAT_OK, NAT_SKIPPED, NAT_NO_IP, NAT_SPAN, NAT_IPV6, NAT_BAD_HDR, NAT_FRAGMENT, NAT_NO_L4, NAT_NO_SESSION, NAT_NOT_OURS,
 NAT_EXHAUSTED, NAT_TABLE_FULL) = range(12)
NAT_OUT, NAT_IN, NAT_NONE, NAT_STATIC, NAT_NO_WRITE = (schema.NAT_OUT, schema.NAT_IN, schema.NAT_NONE, schema.NAT_STATIC,
                                                       schema.NAT_NO_WRITE)
_NAT_OUT = (("status", np.uint8), ("entry", np.uint32), ("created", np.uint8))
_NAT_PROTO = {"tcp": 6, "udp": 17, "icmp": 1}


def _ip4(a):
    raw = bytes(int(x) for x in a.split(".")) if isinstance(a, str) else bytes(a)
    if len(raw) != 4:
        raise ValueError(f"nat: an IPv4 address has 4 bytes, not {a!r}")
    return np.frombuffer(raw, np.uint8)


def nat_statics(static):
    """Port forwards as a C-contiguous array of schema.NAT_STATIC_DTYPE (pkt_nat_static_t): an iterable of (proto,
    in_addr, in_port, out_addr, out_port) tuples, or such an array, which passes through."""
    if isinstance(static, np.ndarray):
        if static.dtype != schema.NAT_STATIC_DTYPE:
            raise ValueError("nat: a statics array must have schema.NAT_STATIC_DTYPE")
        return np.ascontiguousarray(static).reshape(-1)
    static = list(static)
    arr = np.zeros(len(static), schema.NAT_STATIC_DTYPE)
    for i, (proto, ia, ip, oa, op) in enumerate(static):
        arr["proto"][i] = _NAT_PROTO.get(proto, proto)
        arr["in_addr"][i], arr["in_port"][i], arr["out_addr"][i], arr["out_port"][i] = _ip4(ia), int(ip), _ip4(oa), int(op)
    return arr


class NatResult:
    """What Nat.run gives: status (uint8 [n]: pktgpu.NAT_OK / _SKIPPED / _NO_IP / _SPAN / _IPV6 / _BAD_HDR / _FRAGMENT /
    _NO_L4 / _NO_SESSION / _NOT_OURS / _EXHAUSTED / _TABLE_FULL), entry (uint32 [n]: p * E + e of a dynamic session,
    NAT_STATIC | index of a static, NAT_NONE otherwise) and created (uint8 [n]: 1 for the first packet of a session the
    call created); hits / bytes (uint64 [12]) where they were asked for.  Outputs not asked for are None."""

    def __init__(self, **kw):
        self.status = self.entry = self.created = self.hits = self.bytes = None
        self.__dict__.update(kw)


class Nat:
    """pkt_nat_t: NAPT44 sessions and the translation of a parsed batch, IN PLACE (Parser.nat).  Nat(parser, ...) lives
    on the parser's device and takes and gives device tensors; Nat(None, ...) is the host handle over numpy arrays (the
    sequential model, no device).

        nat = p.nat(["192.0.2.1"], ports=(1024, 65535), slots=1 << 20, static=[("tcp", "10.0.0.5", 80, "192.0.2.1", 80)])
        r = nat.run(batch, chain, dir=m["action"], now=t)    # dir 0: inside -> outside, 1: outside -> inside, else skipped
        fwd.run(batch, chain, lpm=lpm)                       # the chain columns stay valid: no second parse
        nat.expire(t, idle=(7440, 300, 60))                  # TCP, UDP, ICMP idle times in seconds (0: never)
    """

    def __init__(self, parser, pool, ports=(1024, 65535), slots=1 << 16, static=()):
        from . import _lib
        self._lib = _lib
        self._L = _lib.load()
        self.parser = parser
        self.pool = np.ascontiguousarray(np.stack([_ip4(a) for a in pool]) if len(pool) else np.zeros((0, 4), np.uint8))
        self.statics = nat_statics(static)
        self.ports = (int(ports[0]), int(ports[1]))
        self.slots = int(slots)
        self.nports = self.ports[1] - self.ports[0] + 1
        self.entries = len(self.pool) * self.nports  # E
        ns = self.statics.size
        args = (self.pool.ctypes.data if len(self.pool) else None, len(self.pool), self.ports[0] & 0xFFFFFFFF,
                self.ports[1] & 0xFFFFFFFF, self.slots, self.statics.ctypes.data if ns else None, ns)
        h = ctypes.c_void_p()
        self._t = None
        if parser is None:
            rc = self._L.pkt_nat_create_host(*args, ctypes.byref(h))
            if rc != 0:
                msg = self._L.pkt_nat_last_error(None)
                raise ValueError(f"pkt_nat_create_host failed ({rc}): {msg.decode() if msg else ''}")
        else:
            parser._check(self._L.pkt_nat_create(parser._ctx, *args, ctypes.byref(h)), "pkt_nat_create")
        self._t = h

    def _check(self, rc, what):
        if rc != 0:
            msg = self._L.pkt_nat_last_error(self._t)
            raise RuntimeError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")

    def run(self, batch, chain, dir=NAT_OUT, now=0, select=None, which_ip=0, write=True,
            outputs=("status", "entry", "created"), counters=None, stream=None):
        """pkt_nat_batch: translate the batch IN PLACE -> NatResult.  `dir`: NAT_OUT / NAT_IN for every packet, or a
        uint8 [n] array (a match action; values above 1 skip the packet).  `now`: the caller's clock in seconds.
        `select` (uint8 [n]): a packet whose byte is 0 is skipped.  write=False: create, refresh and decide, store
        nothing.  `outputs`: which of "status", "entry", "created" to produce.  counters: True allocates zeroed uint64
        [12] hits and bytes and returns them; a (hits, bytes) pair passed in is accumulated into (either may be None).
        `batch` / `chain`: the forms Lpm.lookup takes.  Device tensors for a device handle, numpy arrays for a host
        handle.  Asynchronous on `stream`."""
        bad = set(outputs) - {k for k, _ in _NAT_OUT}
        if bad:
            raise ValueError(f"nat: unknown outputs {sorted(bad)}")
        if isinstance(batch, (tuple, list)):
            batch = dict(zip(("slab", "offsets", "lens"), batch))
        g = lambda k: batch.get(k)  # noqa: E731
        host = self.parser is None
        nc = schema.NAT_STATUS_COUNT
        dir_all, dir_arr = (int(dir), None) if isinstance(dir, (int, np.integer)) else (0, dir)
        if host:
            slab = batch["slab"]
            if write and not (isinstance(slab, np.ndarray) and slab.dtype == np.uint8 and slab.flags.c_contiguous
                              and slab.flags.writeable):
                raise ValueError("nat: the host handle rewrites batch['slab'] in place: a writeable C-contiguous uint8 array")
            b, keep = _host_batch(self._lib, batch)
            cols = (np.ascontiguousarray(chain["n_hdrs"], np.uint8), np.ascontiguousarray(chain["hdr_type"], np.uint8),
                    np.ascontiguousarray(chain["hdr_off"], np.uint16))
            ch = self._lib.PktChain(*[c.ctypes.data for c in cols])
            dir_arr = None if dir_arr is None else np.ascontiguousarray(dir_arr, np.uint8)
            select = None if select is None else np.ascontiguousarray(np.asarray(select) != 0).view(np.uint8)
            res = {k: np.zeros(b.n, dt) for k, dt in _NAT_OUT if k in outputs}
            ptr = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
            zeros = lambda: np.zeros(nc, np.uint64)  # noqa: E731
            ok = lambda c: isinstance(c, np.ndarray) and c.dtype == np.uint64 and c.size == nc and c.flags.c_contiguous  # noqa: E731
        else:
            torch = _torch()
            b = self.parser._batch(batch["slab"], g("n"), g("stride"), g("offsets"), g("lens"))
            ch = self.parser._chain(chain)
            for a in (dir_arr, select):
                assert a is None or (a.is_cuda and a.dtype == torch.uint8 and a.is_contiguous() and a.numel() >= b.n)
            dev = self.parser.torch_device
            res = {k: torch.empty(b.n, dtype=_tdtype(dt), device=dev) for k, dt in _NAT_OUT if k in outputs}
            ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None  # noqa: E731
            zeros = lambda: torch.zeros(nc, dtype=torch.uint64, device=dev)  # noqa: E731
            ok = lambda c: c.is_cuda and c.dtype == torch.uint64 and c.numel() == nc and c.is_contiguous()  # noqa: E731
        hits, nbytes = (zeros(), zeros()) if counters is True else (None, None) if not counters else counters
        for name, c in (("hits", hits), ("bytes", nbytes)):
            if c is not None:
                assert ok(c), f"nat: {name} is a contiguous uint64 [{nc}] array"
                res[name] = c
        self._check(self._L.pkt_nat_batch(self._t, ctypes.byref(b), ctypes.byref(ch), int(which_ip),
                                          0 if write else schema.NAT_NO_WRITE, dir_all & 0xFFFFFFFF, ptr(dir_arr), ptr(select),
                                          int(now) & 0xFFFFFFFF, *[ptr(res.get(k)) for k, _ in _NAT_OUT], ptr(hits),
                                          ptr(nbytes), None if host else self.parser._stream(stream)), "pkt_nat_batch")
        return NatResult(**res)

    def expire(self, now, idle):
        """pkt_nat_expire (blocking): remove the dynamic sessions of protocol p (TCP, UDP, ICMP) with idle[p] != 0 and
        last_seen + idle[p] <= now -> how many were removed.  `idle`: one number for all three, or three."""
        idle = [int(idle)] * 3 if isinstance(idle, (int, np.integer)) else [int(x) for x in idle]
        if len(idle) != 3:
            raise ValueError("nat: idle is one number or three (TCP, UDP, ICMP)")
        arr = (ctypes.c_uint32 * 3)(*idle)
        gone = ctypes.c_uint64()
        self._check(self._L.pkt_nat_expire(self._t, int(now) & 0xFFFFFFFF, arr, ctypes.byref(gone)), "pkt_nat_expire")
        return gone.value

    def count(self):
        """pkt_nat_count (blocking) -> the dynamic sessions per protocol (TCP, UDP, ICMP)."""
        c = (ctypes.c_uint64 * 3)()
        self._check(self._L.pkt_nat_count(self._t, c), "pkt_nat_count")
        return tuple(int(x) for x in c)

    def sessions(self):
        """pkt_nat_export (blocking) -> a numpy array of schema.NAT_RECORD_DTYPE: the dynamic sessions in ascending
        (protocol index, pool entry), then the statics (flags = schema.NAT_REC_STATIC) in the order given."""
        cap = sum(self.count()) + self.statics.size
        n = ctypes.c_uint64()
        if self.parser is None:
            rec = np.zeros(cap, schema.NAT_RECORD_DTYPE)
            self._check(self._L.pkt_nat_export(self._t, rec.ctypes.data if cap else None, cap, ctypes.byref(n)),
                        "pkt_nat_export")
        else:
            torch = _torch()
            t = torch.zeros(max(cap, 1) * schema.NAT_RECORD_DTYPE.itemsize, dtype=torch.uint8, device=self.parser.torch_device)
            self._check(self._L.pkt_nat_export(self._t, t.data_ptr(), cap, ctypes.byref(n)), "pkt_nat_export")
            rec = t.cpu().numpy()[:cap * schema.NAT_RECORD_DTYPE.itemsize].view(schema.NAT_RECORD_DTYPE)
        return rec[:min(cap, n.value)].copy()

    def clear(self, stream=None):
        """pkt_nat_clear: no dynamic session, cursors 0; the statics stay.  Asynchronous on `stream`."""
        self._check(self._L.pkt_nat_clear(self._t, None if self.parser is None else self.parser._stream(stream)),
                    "pkt_nat_clear")

    def close(self):
        if getattr(self, "_t", None):
            self._L.pkt_nat_destroy(self._t)
            self._t = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


METER_GREEN, METER_YELLOW, METER_RED, METER_UNMETERED = range(4)
METER_SRTCM, METER_TRTCM, METER_PASS, METER_DROP, METER_REMARK = (schema.METER_SRTCM, schema.METER_TRTCM, schema.METER_PASS,
                                                                  schema.METER_DROP, schema.METER_REMARK)
_METER_OUT = (("color", np.uint8), ("passed", np.uint8), ("marked", np.uint8))


def ns_from_sec_usec(ts_sec, ts_usec):
    """A capture's timestamps (the ts_sec and ts_usec columns of a pcap index) as the uint64 nanoseconds Meters.run's
    `time` takes: numpy arrays or torch tensors, elementwise."""
    if isinstance(ts_sec, np.ndarray) or np.isscalar(ts_sec):
        return np.asarray(ts_sec).astype(np.uint64) * np.uint64(10 ** 9) + np.asarray(ts_usec).astype(np.uint64) * np.uint64(1000)
    torch = _torch()
    ns = ts_sec.to(torch.int64) * 10 ** 9 + ts_usec.to(torch.int64) * 1000  # below 2^63 for every 32-bit second
    return ns.view(torch.uint64)


def meter_cfgs(cfgs):
    """Meter configurations as a C-contiguous array of schema.METER_CFG_DTYPE (pkt_meter_cfg_t): such an array passes
    through; otherwise an iterable of dicts with cir, cbs and optionally pir, xbs (EBS for srTCM, PBS for trTCM), mode
    ("srtcm" / "trtcm" or the number), color_aware, action (three of "pass" / "drop" / "remark" or the numbers, for
    green, yellow, red; default pass, pass, drop) and dscp (three of 0..63)."""
    if isinstance(cfgs, np.ndarray):
        if cfgs.dtype != schema.METER_CFG_DTYPE:
            raise ValueError("meters: a cfg array must have schema.METER_CFG_DTYPE")
        return np.ascontiguousarray(cfgs).reshape(-1)
    cfgs = list(cfgs)
    arr = np.zeros(len(cfgs), schema.METER_CFG_DTYPE)
    for i, d in enumerate(cfgs):
        bad = set(d) - {"cir", "pir", "cbs", "xbs", "mode", "color_aware", "action", "dscp"}
        if bad:
            raise ValueError(f"meters: unknown cfg keys {sorted(bad)}")
        arr["cir"][i], arr["pir"][i] = int(d["cir"]), int(d.get("pir", 0))
        arr["cbs"][i], arr["xbs"][i] = int(d["cbs"]), int(d.get("xbs", 0))
        mode = d.get("mode", schema.METER_SRTCM)
        arr["mode"][i] = schema.METER_MODE[mode] if isinstance(mode, str) else int(mode)
        arr["flags"][i] = schema.METER_F_COLOR_AWARE if d.get("color_aware") else 0
        act = d.get("action", ("pass", "pass", "drop"))
        arr["action"][i] = [schema.METER_ACTION[a] if isinstance(a, str) else int(a) for a in act]
        arr["dscp"][i] = [int(x) for x in d.get("dscp", (0, 0, 0))]
    return arr


class MeterResult:
    """What Meters.run gives: color (uint8 [n]: pktgpu.METER_GREEN / _YELLOW / _RED / _UNMETERED), passed (uint8 [n]: 0
    for a packet its colour's action drops; pcap_write's `select`), marked (uint8 [n]: 1 where a DSCP was written);
    hits / bytes (uint64 [4], per colour) where they were asked for.  Outputs not asked for are None."""

    def __init__(self, **kw):
        self.color = self.passed = self.marked = self.hits = self.bytes = None
        self.__dict__.update(kw)


class Meters:
    """pkt_meter_t: a table of srTCM (RFC 2697) / trTCM (RFC 2698) policers and the metering of a batch (Parser.meters).
    Meters(parser, ...) lives on the parser's device and takes and gives device tensors; Meters(None, ...) is the host
    handle over numpy arrays (the sequential model, no device).

        m = p.meters([dict(cir=125_000_000, cbs=1 << 16, xbs=1 << 17)] * nflows, adjust=20)
        u = table.update(keys)                                   # its flow_id is the meter index
        r = m.run(st.batch(), meter=u["flow_id"], time=pktgpu.ns_from_sec_usec(ts_sec, ts_usec))
        p.pcap_write(..., select=r.passed)
    """

    def __init__(self, parser, cfgs, adjust=0):
        from . import _lib
        self._lib = _lib
        self._L = _lib.load()
        self.parser = parser
        self.cfgs = meter_cfgs(cfgs)
        self.nmeters = int(self.cfgs.size)
        self.adjust = int(adjust)
        if not -(1 << 31) <= self.adjust < (1 << 31):
            raise ValueError("meters: adjust is an int32")
        args = (self.cfgs.ctypes.data if self.nmeters else None, self.nmeters, self.adjust)
        h = ctypes.c_void_p()
        self._t = None
        if parser is None:
            rc = self._L.pkt_meter_create_host(*args, ctypes.byref(h))
            if rc != 0:
                msg = self._L.pkt_meter_last_error(None)
                raise ValueError(f"pkt_meter_create_host failed ({rc}): {msg.decode() if msg else ''}")
        else:
            parser._check(self._L.pkt_meter_create(parser._ctx, *args, ctypes.byref(h)), "pkt_meter_create")
        self._t = h

    def _check(self, rc, what):
        if rc != 0:
            msg = self._L.pkt_meter_last_error(self._t)
            raise RuntimeError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")

    def run(self, batch, chain=None, meter=0, now=0, time=None, in_color=None, select=None, mark=False, which_ip=0,
            outputs=("color", "passed", "marked"), counters=None, stream=None):
        """pkt_meter_batch: meter the batch -> MeterResult.  `meter`: one index for every packet, or a uint32 [n]
        array (a flow_id, a rule id, a port; an index at or above nmeters leaves the packet unmetered).  `now`: the
        batch's time in ns, or `time`: a uint64 [n] array of per-packet times (ns_from_sec_usec).  `in_color` (uint8
        [n]): the colour a colour-aware meter starts from.  `select` (uint8 [n]): a packet whose byte is 0 is
        unmetered.  mark=True writes the DSCP of the REMARK actions IN PLACE and needs `chain` (`which_ip` as
        Lpm.lookup takes it).  `outputs`: which of "color", "passed", "marked" to produce.  counters: True allocates
        zeroed uint64 [4] hits and bytes and returns them; a (hits, bytes) pair passed in is accumulated into (either
        may be None).  `batch` / `chain`: the forms Lpm.lookup takes.  Device tensors for a device handle, numpy arrays
        for a host handle.  Asynchronous on `stream`."""
        bad = set(outputs) - {k for k, _ in _METER_OUT}
        if bad:
            raise ValueError(f"meters: unknown outputs {sorted(bad)}")
        if mark and chain is None:
            raise ValueError("meters: mark=True needs the chain")
        if isinstance(batch, (tuple, list)):
            batch = dict(zip(("slab", "offsets", "lens"), batch))
        g = lambda k: batch.get(k)  # noqa: E731
        host = self.parser is None
        nc = schema.METER_COLORS
        meter_all, meter_arr = (int(meter), None) if isinstance(meter, (int, np.integer)) else (0, meter)
        if host:
            slab = batch["slab"]
            if mark and not (isinstance(slab, np.ndarray) and slab.dtype == np.uint8 and slab.flags.c_contiguous
                             and slab.flags.writeable):
                raise ValueError("meters: the host handle remarks batch['slab'] in place: a writeable C-contiguous uint8 array")
            b, keep = _host_batch(self._lib, batch)
            ch = None
            if chain is not None:
                cols = (np.ascontiguousarray(chain["n_hdrs"], np.uint8), np.ascontiguousarray(chain["hdr_type"], np.uint8),
                        np.ascontiguousarray(chain["hdr_off"], np.uint16))
                ch = self._lib.PktChain(*[c.ctypes.data for c in cols])
            meter_arr = None if meter_arr is None else np.ascontiguousarray(meter_arr, np.uint32)
            time = None if time is None else np.ascontiguousarray(time, np.uint64)
            in_color = None if in_color is None else np.ascontiguousarray(in_color, np.uint8)
            select = None if select is None else np.ascontiguousarray(np.asarray(select) != 0).view(np.uint8)
            for a in (meter_arr, time, in_color, select):
                assert a is None or a.size >= b.n, "meters: a per-packet array is shorter than the batch"
            res = {k: np.zeros(b.n, dt) for k, dt in _METER_OUT if k in outputs}
            ptr = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
            zeros = lambda: np.zeros(nc, np.uint64)  # noqa: E731
            ok = lambda c: isinstance(c, np.ndarray) and c.dtype == np.uint64 and c.size == nc and c.flags.c_contiguous  # noqa: E731
        else:
            torch = _torch()
            b = self.parser._batch(batch["slab"], g("n"), g("stride"), g("offsets"), g("lens"))
            ch = None if chain is None else self.parser._chain(chain)
            for a, dt in ((meter_arr, torch.uint32), (time, torch.uint64), (in_color, torch.uint8), (select, torch.uint8)):
                assert a is None or (a.is_cuda and a.dtype == dt and a.is_contiguous() and a.numel() >= b.n)
            dev = self.parser.torch_device
            res = {k: torch.empty(b.n, dtype=_tdtype(dt), device=dev) for k, dt in _METER_OUT if k in outputs}
            ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None  # noqa: E731
            zeros = lambda: torch.zeros(nc, dtype=torch.uint64, device=dev)  # noqa: E731
            ok = lambda c: c.is_cuda and c.dtype == torch.uint64 and c.numel() == nc and c.is_contiguous()  # noqa: E731
        hits, nbytes = (zeros(), zeros()) if counters is True else (None, None) if not counters else counters
        for name, c in (("hits", hits), ("bytes", nbytes)):
            if c is not None:
                assert ok(c), f"meters: {name} is a contiguous uint64 [{nc}] array"
                res[name] = c
        self._check(self._L.pkt_meter_batch(self._t, ctypes.byref(b), None if ch is None else ctypes.byref(ch),
                                            int(which_ip), schema.METER_MARK if mark else 0, meter_all & 0xFFFFFFFF,
                                            ptr(meter_arr), int(now) & 0xFFFFFFFFFFFFFFFF, ptr(time), ptr(in_color),
                                            ptr(select), *[ptr(res.get(k)) for k, _ in _METER_OUT], ptr(hits), ptr(nbytes),
                                            None if host else self.parser._stream(stream)), "pkt_meter_batch")
        return MeterResult(**res)

    def export(self, first=0, count=None):
        """pkt_meter_export (blocking) -> a numpy array of schema.METER_STATE_DTYPE: the buckets (10^-9 byte), `last`
        (ns) and the per-colour packet and byte counters of meters [first, first + count)."""
        count = self.nmeters - first if count is None else int(count)
        if self.parser is None:
            st = np.zeros(count, schema.METER_STATE_DTYPE)
            self._check(self._L.pkt_meter_export(self._t, first, count, st.ctypes.data if count else None), "pkt_meter_export")
            return st
        torch = _torch()
        size = schema.METER_STATE_DTYPE.itemsize
        t = torch.zeros(max(count, 1) * size, dtype=torch.uint8, device=self.parser.torch_device)
        self._check(self._L.pkt_meter_export(self._t, first, count, t.data_ptr()), "pkt_meter_export")
        return t.cpu().numpy()[:count * size].view(schema.METER_STATE_DTYPE).copy()

    def reset(self, stream=None):
        """pkt_meter_reset: full buckets, last = 0, zero counters, as after create.  Asynchronous on `stream`."""
        self._check(self._L.pkt_meter_reset(self._t, None if self.parser is None else self.parser._stream(stream)),
                    "pkt_meter_reset")

    def close(self):
        if getattr(self, "_t", None):
            self._L.pkt_meter_destroy(self._t)
            self._t = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


(FRAG_FITS, FRAG_SPLIT, FRAG_SKIPPED, FRAG_NO_IP, FRAG_SPAN, FRAG_IPV6, FRAG_BAD_HDR, FRAG_TRUNC, FRAG_DF,
 FRAG_MTU) = range(10)
FRAG_NONE, FRAG_ONLY_SPLIT, FRAG_NO_WRITE = schema.FRAG_NONE, schema.FRAG_ONLY_SPLIT, schema.FRAG_NO_WRITE


class _Produced:
    """What the results of Parser.fragment, .reassemble and .icmp_errors share (_produce fills them in)."""
    slab = offsets = lens = src_index = out_chain = hits = None

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def batch(self):
        return dict(slab=self.slab, offsets=self.offsets, lens=self.lens)


def _produce(parser, e, batch, chain, select, which_ip, flags, inputs, plan_only, out_cap, dst_bytes, hits, host, stream):
    """The call sequence of the three entries that pack outputs into a second slab (pktgpu_outbatch.hpp's contract).
    `e`: the entry (its C functions' stem, result class, status count, NO_WRITE flag, per-packet outputs and its own
    per-output column, if any); `inputs(per_packet)`: the entry's own C arguments, between flags and select, where
    per_packet(v, dtype) turns a value for all packets or one per packet into the (array, scalar) argument pair."""
    from . import _lib
    L = _lib.load()
    if hasattr(batch, "batch") and callable(batch.batch):
        batch = batch.batch()
    if isinstance(batch, (tuple, list)):
        batch = dict(zip(("slab", "offsets", "lens"), batch))
    g = lambda k: batch.get(k)  # noqa: E731
    fn, nc, what = e["fn"], e["nc"], e["what"]
    if host:
        b, keep = _host_batch(_lib, batch)
        cols = (np.ascontiguousarray(chain["n_hdrs"], np.uint8), np.ascontiguousarray(chain["hdr_type"], np.uint8),
                np.ascontiguousarray(chain["hdr_off"], np.uint16))
        ch = _lib.PktChain(*[c.ctypes.data for c in cols])
        select = None if select is None else np.ascontiguousarray(np.asarray(select) != 0).view(np.uint8)
        empty = lambda k, dt: np.zeros(k, dt)  # noqa: E731
        ptr = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
        ok = lambda c: isinstance(c, np.ndarray) and c.dtype == np.uint64 and c.size == nc and c.flags.c_contiguous  # noqa: E731
        column = lambda v, dt: np.ascontiguousarray(v, dt)  # noqa: E731
    else:
        torch = _torch()
        b = parser._batch(batch["slab"], g("n"), g("stride"), g("offsets"), g("lens"))
        ch = parser._chain(chain)
        dev = parser.torch_device
        assert select is None or (select.is_cuda and select.dtype == torch.uint8 and select.is_contiguous()
                                  and select.numel() >= b.n)
        empty = lambda k, dt: torch.zeros(k, dtype=_tdtype(dt), device=dev)  # noqa: E731
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None  # noqa: E731
        ok = lambda c: c.is_cuda and c.dtype == torch.uint64 and c.numel() == nc and c.is_contiguous()  # noqa: E731

        def column(v, dt):
            assert v.is_cuda and v.dtype == _tdtype(dt) and v.is_contiguous() and v.numel() >= b.n
            return v
    held = []  # the per-packet inputs, alive until the calls are done

    def per_packet(v, dt):
        if isinstance(v, (int, np.integer)):
            return None, int(v)
        held.append(column(v, dt))
        return ptr(held[-1]), 0

    ins = inputs(per_packet)
    if hits is True:
        hits = empty(nc, np.uint64)
    if hits is not None and hits is not False:
        assert ok(hits), f"{what}: hits is a contiguous uint64 [{nc}] array"
    else:
        hits = None
    res = e["result"](hits=hits, **{k: empty(b.n, dt) for k, dt in e["per_packet"]})
    extra = [e["extra"]] if e["extra"] else []
    tot, cnt = ctypes.c_uint64(0), ctypes.c_uint64(0)

    def call(fl, out, with_hits):
        dst = out.get("slab")
        oc = None
        if out:
            oc = _lib.PktChain(*[ptr(out["out_chain"][k]) for k in ("n_hdrs", "hdr_type", "hdr_off")])
        args = (ctypes.byref(b), ctypes.byref(ch), int(which_ip), fl, *ins, ptr(select),
                *[ptr(getattr(res, k)) for k, _ in e["per_packet"]],
                ptr(dst), 0 if dst is None else int(dst.size if host else dst.numel()), out.get("cap", 0),
                ptr(out.get("offsets")), ptr(out.get("lens")), ptr(out.get("src_index")), *[ptr(out.get(k)) for k, _ in extra],
                ctypes.byref(oc) if oc is not None else None, ptr(hits) if with_hits else None, ctypes.byref(tot),
                ctypes.byref(cnt))
        if host:
            rc = getattr(L, fn + "_host")(*args)
            if rc != 0:
                raise ValueError(f"{fn}_host failed ({rc}); it needs {cnt.value} outputs and {tot.value} bytes")
        else:
            parser._check(getattr(L, fn + "_batch")(parser._ctx, *args, parser._stream(stream)), fn + "_batch")

    sized = out_cap is not None and dst_bytes is not None
    if plan_only or not sized:
        call(flags | e["no_write"], {}, plan_only)
        if plan_only:
            res.n_out, res.bytes_out = cnt.value, tot.value
            return res
        out_cap = cnt.value if out_cap is None else out_cap
        dst_bytes = tot.value if dst_bytes is None else dst_bytes
    cap = max(1, int(out_cap))
    out = dict(slab=empty(max(16, int(dst_bytes)), np.uint8), cap=cap, offsets=empty(cap, np.uint64),
               lens=empty(cap, np.uint32), src_index=empty(cap, np.uint32), **{k: empty(cap, dt) for k, dt in extra},
               out_chain=dict(n_hdrs=empty(cap, np.uint8), hdr_type=empty((schema.MAX_HDRS, cap), np.uint8),
                              hdr_off=empty((schema.MAX_HDRS, cap), np.uint16)))
    call(flags, out, True)
    out.pop("cap")
    res.__dict__.update(out, n_out=cnt.value, bytes_out=tot.value)
    return res


class FragResult(_Produced):
    """What Parser.fragment gives.  Per source packet: status (uint8: pktgpu.FRAG_FITS / _SPLIT / _SKIPPED / _NO_IP /
    _SPAN / _IPV6 / _BAD_HDR / _TRUNC / _DF / _MTU), nfrag, first (uint32; FRAG_NONE where nfrag is 0).  The totals:
    n_out, bytes_out.  Unless plan_only, per output (arrays of out_cap entries, empty past n_out): slab, offsets,
    lens, src_index, frag_index and out_chain ({"n_hdrs", "hdr_type", "hdr_off"}, slot-major over out_cap); batch()
    is the output as the batch dict the other calls take.  hits: the per-status counters, if asked for."""
    frag_index = None


_FRAG = dict(what="fragment", fn="pkt_frag", result=FragResult, nc=schema.FRAG_STATUS_COUNT, no_write=schema.FRAG_NO_WRITE,
             per_packet=(("status", np.uint8), ("nfrag", np.uint32), ("first", np.uint32)), extra=("frag_index", np.uint16))


def _fragment(parser, batch, chain, mtu, select, which_ip, only_split, plan_only, out_cap, dst_bytes, hits, host, stream):
    return _produce(parser, _FRAG, batch, chain, select, which_ip, schema.FRAG_ONLY_SPLIT if only_split else 0,
                    lambda per_packet: per_packet(mtu, np.uint16), plan_only, out_cap, dst_bytes, hits, host, stream)


(ICMPE_SENT, ICMPE_SKIPPED, ICMPE_BAD_REASON, ICMPE_NO_IP, ICMPE_SPAN, ICMPE_NO_ETHER, ICMPE_NO_SRC, ICMPE_BAD_HDR,
 ICMPE_FRAGMENT, ICMPE_BAD_SRC, ICMPE_MCAST, ICMPE_ICMP_ERR) = range(12)
ICMPE_NONE, ICMPE_NO_WRITE = schema.ICMPE_NONE, schema.ICMPE_NO_WRITE


class IcmpErrResult(_Produced):
    """What Parser.icmp_errors gives.  Per source packet: status (uint8: pktgpu.ICMPE_SENT / _SKIPPED / _BAD_REASON /
    _NO_IP / _SPAN / _NO_ETHER / _NO_SRC / _BAD_HDR / _FRAGMENT / _BAD_SRC / _MCAST / _ICMP_ERR) and out_index (uint32:
    the packet's output, ICMPE_NONE where there is none).  The totals: n_out, bytes_out.  Unless plan_only, per output
    (arrays of out_cap entries, empty past n_out): slab, offsets, lens, src_index and out_chain ({"n_hdrs",
    "hdr_type", "hdr_off"}, slot-major over out_cap); batch() is the output as the batch dict the other calls take.
    hits: the per-status counters, if asked for."""


def _icmp_addr(a, size, what):
    """An address given as a string or as bytes -> `size` wire bytes (None: all zero, no errors of that version)."""
    import socket
    if a is None:
        return bytes(size)
    if isinstance(a, str):
        a = socket.inet_pton(socket.AF_INET if size == 4 else socket.AF_INET6, a)
    a = bytes(a)
    if len(a) != size:
        raise ValueError(f"icmp_errors: {what} is {size} bytes or an address string")
    return a


_ICMPE = dict(what="icmp_errors", fn="pkt_icmp_err", result=IcmpErrResult, nc=schema.ICMPE_STATUS_COUNT,
              no_write=schema.ICMPE_NO_WRITE, per_packet=(("status", np.uint8), ("out_index", np.uint32)), extra=None)


def _icmp_errors(parser, batch, chain, reason, fwd_status, frag_status, mtu, src4, src6, ttl, tos, max4, max6, ident,
                 select, which_ip, plan_only, out_cap, dst_bytes, hits, host, stream):
    from . import _lib
    if sum(x is not None for x in (reason, fwd_status, frag_status)) != 1:
        raise ValueError("icmp_errors: exactly one of reason, fwd_status and frag_status")
    code, cmap = reason, None
    if fwd_status is not None:
        code, cmap = fwd_status, schema.ICMP_MAP_FWD
    elif frag_status is not None:
        code, cmap = frag_status, schema.ICMP_MAP_FRAG
    cfg = _lib.PktIcmpCfg()
    cfg.src4[:] = _icmp_addr(src4, 4, "src4")
    cfg.src6[:] = _icmp_addr(src6, 16, "src6")
    cfg.max4, cfg.max6, cfg.ident, cfg.ttl, cfg.tos = int(max4), int(max6), int(ident) & 0xFFFF, int(ttl), int(tos)
    inputs = lambda per_packet: (ctypes.byref(cfg), *per_packet(code, np.uint8),  # noqa: E731
                                 None if cmap is None else cmap.ctypes.data, *per_packet(mtu, np.uint16))
    return _produce(parser, _ICMPE, batch, chain, select, which_ip, 0, inputs, plan_only, out_cap, dst_bytes, hits, host,
                    stream)


(TUNE_OK, TUNE_SKIPPED, TUNE_NO_TUNNEL, TUNE_NO_IP, TUNE_SPAN, TUNE_BAD_L2, TUNE_BAD_HDR, TUNE_TRUNC, TUNE_TOO_BIG,
 TUNE_DEPTH) = range(10)
(TUND_OK, TUND_SKIPPED, TUND_NO_IP, TUND_SPAN, TUND_BAD_HDR, TUND_FRAGMENT, TUND_NOT_TUNNEL, TUND_BAD_GRE, TUND_NO_MATCH,
 TUND_TRUNC, TUND_NO_INNER) = range(11)
TUN_NONE, TUN_NO_WRITE = schema.TUN_NONE, schema.TUN_NO_WRITE


class TunnelResult(_Produced):
    """What Tunnels.encap and Tunnels.decap give.  Per source packet: status (uint8: pktgpu.TUNE_* / TUND_*), out_index
    (uint32: the packet's output, TUN_NONE where there is none) and, for decap, tunnel_out (uint32: the matched entry,
    TUN_NONE where none was).  The totals: n_out, bytes_out.  Unless plan_only, per output (arrays of out_cap entries,
    empty past n_out): slab, offsets, lens, src_index and out_chain ({"n_hdrs", "hdr_type", "hdr_off"}, slot-major over
    out_cap); batch() is the output as the batch dict the other calls take.  hits: the per-status counters, if asked for."""
    tunnel_out = None


_TUNE = dict(what="tunnels.encap", fn="pkt_tunnel_encap", result=TunnelResult, nc=schema.TUNE_STATUS_COUNT,
             no_write=schema.TUN_NO_WRITE, per_packet=(("status", np.uint8), ("out_index", np.uint32)), extra=None)
_TUND = dict(what="tunnels.decap", fn="pkt_tunnel_decap", result=TunnelResult, nc=schema.TUND_STATUS_COUNT,
             no_write=schema.TUN_NO_WRITE,
             per_packet=(("status", np.uint8), ("out_index", np.uint32), ("tunnel_out", np.uint32)), extra=None)


def tunnel_entries(entries):
    """Tunnel table entries -> a numpy array of schema.TUNNEL_ENTRY_DTYPE.  An entry is a dict: kind ("vxlan" / "gre" /
    "ipip" or schema.TUN_*), src and dst (address strings, or 4 / 16 bytes; they give ipver), and optionally ttl, tos,
    id (the VNI or the GRE key), sport (lo, hi), eth_dst / eth_src ("aa:bb:.." or 6 bytes), flags (schema.TUN_F_*)."""
    import socket
    if isinstance(entries, np.ndarray):
        if entries.dtype != schema.TUNNEL_ENTRY_DTYPE:
            raise ValueError("tunnels: an entries array has dtype schema.TUNNEL_ENTRY_DTYPE")
        return np.ascontiguousarray(entries)

    def addr(a):
        if isinstance(a, str):
            a = socket.inet_pton(socket.AF_INET6 if ":" in a else socket.AF_INET, a)
        a = bytes(a)
        if len(a) not in (4, 16):
            raise ValueError("tunnels: an address is a string or 4 / 16 bytes")
        return a

    def mac(m):
        m = bytes.fromhex(m.replace(":", "")) if isinstance(m, str) else bytes(m)
        if len(m) != 6:
            raise ValueError("tunnels: a MAC address is 6 bytes")
        return m

    out = np.zeros(len(entries), schema.TUNNEL_ENTRY_DTYPE)
    for k, e in enumerate(entries):
        src, dst = addr(e["src"]), addr(e["dst"])
        if len(src) != len(dst):
            raise ValueError("tunnels: src and dst of an entry are of one IP version")
        r = out[k]
        kind = e["kind"]
        r["kind"] = schema.TUN_KIND[kind] if isinstance(kind, str) else int(kind)
        r["ipver"] = 4 if len(src) == 4 else 6
        r["ttl"], r["tos"], r["flags"], r["id"] = e.get("ttl", 0), e.get("tos", 0), e.get("flags", 0), e.get("id", 0)
        r["sport_lo"], r["sport_hi"] = e.get("sport", (49152, 65535))
        r["src"][:len(src)] = np.frombuffer(src, np.uint8)
        r["dst"][:len(dst)] = np.frombuffer(dst, np.uint8)
        r["eth_dst"][:] = np.frombuffer(mac(e.get("eth_dst", bytes(6))), np.uint8)
        r["eth_src"][:] = np.frombuffer(mac(e.get("eth_src", bytes(6))), np.uint8)
    return out


class Tunnels:
    """A tunnel table (pkt_tunnel_create): VXLAN, GRE and IP-in-IP entries that `encap` puts packets into and `decap`
    takes them out of; Parser.tunnels makes one, Tunnels(None, entries) is the host form (pkt_tunnel_create_host: numpy
    arrays in and out, no device).  The table is read-only: calls on several streams share it.

        tun = p.tunnels([dict(kind="vxlan", src="192.0.2.1", dst="192.0.2.2", id=2000, flags=schema.TUN_F_UDP_CSUM)])
        keys = p.flow_keys(batch, chain)
        e = tun.encap(batch, chain, tunnel=0, entropy=keys)      # one VXLAN packet per packet, lengths and checksums set
        fwd.run(e.batch(), e.out_chain, lpm=lpm, which_ip=0)     # route on the outer header
        d = tun.decap(e.batch(), e.out_chain)                    # and back: d.batch() holds the inner frames
    """

    def __init__(self, parser, entries):
        from . import _lib
        self._lib = _lib
        self._L = _lib.load()
        self.parser = parser
        self.entries = tunnel_entries(entries)
        n = len(self.entries)
        h = ctypes.c_void_p()
        self._t = None
        ptr = self.entries.ctypes.data if n else None
        if parser is None:
            rc = self._L.pkt_tunnel_create_host(ptr, n, ctypes.byref(h))
            if rc != 0:
                msg = self._L.pkt_tunnel_last_error(None)
                raise ValueError(f"pkt_tunnel_create_host failed ({rc}): {msg.decode() if msg else ''}")
        else:
            parser._check(self._L.pkt_tunnel_create(parser._ctx, ptr, n, ctypes.byref(h)), "pkt_tunnel_create")
        self._t = h

    def __len__(self):
        return len(self.entries)

    def _run(self, e, batch, chain, inputs, select, which_ip, plan_only, out_cap, dst_bytes, hits, stream):
        host = self.parser is None
        try:
            return _produce(self.parser, e, batch, chain, select, which_ip, 0, inputs, plan_only, out_cap, dst_bytes, hits,
                            host, stream)
        except ValueError as ex:  # the host twins keep their refusal's text in the handle
            msg = self._L.pkt_tunnel_last_error(self._t) if host else None
            if msg:
                raise ValueError(f"{ex}: {msg.decode()}") from None
            raise

    def _entropy(self, entropy):
        """None, a uint32 [n] array, or Parser.flow_keys' result: its "rss", else the low 32 bits of its "hash"."""
        if not isinstance(entropy, dict):
            return entropy
        if entropy.get("rss") is not None:
            return entropy["rss"]
        h = entropy["hash"]
        if isinstance(h, np.ndarray):
            return (h & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        return h.view(_torch().uint32)[::2].contiguous()

    def encap(self, batch, chain, tunnel=0, entropy=None, ident=0, select=None, which_ip=0, plan_only=False, out_cap=None,
              dst_bytes=None, hits=None, stream=None):
        """pkt_tunnel_encap_batch: every packet of the batch that may goes into its tunnel, all packed at
        16-byte-aligned offsets of a new slab -> TunnelResult.  `tunnel`: one entry index for the batch, or a uint32 [n]
        array (Lpm.lookup's nexthop, Forwarder.run's adj_index or port).  `entropy`: a uint32 [n] array or
        Parser.flow_keys' result, which spreads VXLAN's UDP source port over the entry's range; None takes sport_lo.
        `ident`: the outer IPv4 identification of output q is (ident + q) & 0xFFFF.  `which_ip`: the IP entry GRE and
        IPIP wrap.  `select`, plan_only, out_cap / dst_bytes and hits (uint64 [10]) are as Parser.fragment takes them.
        Parser.fragment over the result splits the OUTER datagram, so encap comes before it."""
        entropy = self._entropy(entropy)
        inputs = lambda per_packet: (self._t, *per_packet(tunnel, np.uint32),  # noqa: E731
                                     None if entropy is None else per_packet(entropy, np.uint32)[0],
                                     int(ident) & 0xFFFFFFFF)
        return self._run(_TUNE, batch, chain, inputs, select, which_ip, plan_only, out_cap, dst_bytes, hits, stream)

    def decap(self, batch, chain, select=None, which_ip=0, plan_only=False, out_cap=None, dst_bytes=None, hits=None,
              stream=None):
        """pkt_tunnel_decap_batch, the inverse of encap: every packet whose `which_ip`-th IP entry is the outer header of
        a tunnel of the table gives its inner packet (VXLAN: the inner frame; GRE / IPIP: the L2 prefix and the inner IP
        packet) -> TunnelResult with tunnel_out, the matched entry per packet.  Checksums are not verified
        (Parser.l4_checksum first), outer IPv4 fragments are refused (Parser.reassemble first).  hits: uint64 [11]."""
        inputs = lambda per_packet: (self._t,)  # noqa: E731
        return self._run(_TUND, batch, chain, inputs, select, which_ip, plan_only, out_cap, dst_bytes, hits, stream)

    def close(self):
        if getattr(self, "_t", None):
            self._L.pkt_tunnel_destroy(self._t)
            self._t = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


(REASM_WHOLE, REASM_JOINED, REASM_PENDING, REASM_SKIPPED, REASM_NO_IP, REASM_SPAN, REASM_BAD_HDR, REASM_TRUNC,
 REASM_TOO_BIG) = range(9)
REASM_NONE, REASM_ONLY_JOINED, REASM_NO_WRITE = schema.REASM_NONE, schema.REASM_ONLY_JOINED, schema.REASM_NO_WRITE


class ReasmResult(_Produced):
    """What Parser.reassemble gives.  Per source packet: status (uint8: pktgpu.REASM_WHOLE / _JOINED / _PENDING /
    _SKIPPED / _NO_IP / _SPAN / _BAD_HDR / _TRUNC / _TOO_BIG) and out_index (uint32: the output carrying the packet's
    bytes; REASM_NONE where there is none).  The totals: n_out, bytes_out.  Unless plan_only, per output (arrays of
    out_cap entries, empty past n_out): slab, offsets, lens, src_index (the owner: the last-arriving member), nfrag
    and out_chain ({"n_hdrs", "hdr_type", "hdr_off"}, slot-major over out_cap); batch() is the output as the batch
    dict the other calls take.  pending: the mask of the fragments to carry over to the next batch.  hits: the
    per-status counters, if asked for."""
    nfrag = None

    @property
    def pending(self):
        return self.status == REASM_PENDING


_REASM = dict(what="reassemble", fn="pkt_reasm", result=ReasmResult, nc=schema.REASM_STATUS_COUNT,
              no_write=schema.REASM_NO_WRITE, per_packet=(("status", np.uint8), ("out_index", np.uint32)),
              extra=("nfrag", np.uint32))


def _reassemble(parser, batch, chain, select, which_ip, only_joined, plan_only, out_cap, dst_bytes, hits, host, stream):
    return _produce(parser, _REASM, batch, chain, select, which_ip, schema.REASM_ONLY_JOINED if only_joined else 0,
                    lambda per_packet: (), plan_only, out_cap, dst_bytes, hits, host, stream)


# ----------------------------------------------------------------- PacketSlice-style host views
(SCAN_MISS, SCAN_HIT, SCAN_SKIPPED, SCAN_NO_CHAIN, SCAN_SPAN) = range(5)
SCAN_NONE, SCAN_NOCASE = schema.SCAN_NONE, schema.SCAN_NOCASE
_SCAN_OUT = (("status", np.uint8), ("pat", np.uint32), ("off", np.uint16), ("action", np.uint32), ("sel", np.uint8),
             ("count", np.uint32), ("matched", np.uint64))


def scan_patterns(patterns, nocase=False, groups=None, actions=None):
    """A pattern list as pkt_scan_create takes it: (blob, table) with `blob` a uint8 array of the patterns' bytes end
    to end and `table` a C-contiguous array of schema.SCAN_PATTERN_DTYPE (pkt_scan_pattern_t).  `patterns`: an
    iterable of bytes / str (UTF-8), or such a (blob, table) pair, which is passed through."""
    if isinstance(patterns, tuple) and len(patterns) == 2 and isinstance(patterns[1], np.ndarray) \
            and patterns[1].dtype == schema.SCAN_PATTERN_DTYPE:
        return np.ascontiguousarray(patterns[0], np.uint8).reshape(-1), np.ascontiguousarray(patterns[1])
    pats = [p.encode() if isinstance(p, str) else bytes(p) for p in patterns]
    n = len(pats)
    per = lambda v, d: [d] * n if v is None else ([v] * n if np.isscalar(v) else list(v))  # noqa: E731
    nc, gr, ac = per(nocase, False), per(groups, 0), per(actions, 1)
    if not (len(nc) == len(gr) == len(ac) == n):
        raise ValueError("scanner: nocase / groups / actions must have one entry per pattern")
    tab = np.zeros(n, schema.SCAN_PATTERN_DTYPE)
    lens = np.array([len(p) for p in pats], np.int64)
    if n and (lens.max() > 0xFFFF or max(gr) > 0xFF or min(gr) < 0):
        raise ValueError("scanner: a pattern's length or group does not fit pkt_scan_pattern_t")
    tab["off"] = np.concatenate(([0], np.cumsum(lens)[:-1])) if n else 0
    tab["len"] = lens
    tab["flags"] = [schema.SCAN_NOCASE if x else 0 for x in nc]
    tab["group"] = gr
    tab["action"] = ac
    return np.frombuffer(b"".join(pats), np.uint8), tab


class ScanResult:
    """What Scanner.run gives, the arrays asked for among: status (uint8: pktgpu.SCAN_MISS / _HIT / _SKIPPED /
    _NO_CHAIN / _SPAN), pat (uint32: the lowest occurring pattern, SCAN_NONE = none), off (uint16: its first
    occurrence, from the packet's first byte), action (uint32), sel (uint8: action != 0, the mask pcap_write and edit
    take), count (uint32: all occurrences), matched (uint64: bit g = a pattern of group g occurs); hits (uint64
    [npatterns + 1]: occurrences per pattern, then the MISS packets), if asked for.  The rest is None."""

    def __init__(self, **kw):
        self.status = self.pat = self.off = self.action = self.sel = self.count = self.matched = self.hits = None
        self.__dict__.update(kw)

    @property
    def hit(self):
        return self.status == SCAN_HIT


class Scanner:
    """pkt_scan_t: a compiled pattern set (Parser.scanner).  Scanner(parser, patterns) lives on the parser's device
    and takes and gives device tensors; Scanner(None, patterns) is the host handle over numpy arrays (no device).

        sc = p.scanner([b"GET /", b"POST /", "user-agent:"], nocase=[False, False, True], groups=[0, 0, 1])
        r = sc.run(batch, chain)                     # ScanResult: the payloads, from a parse's chain
        p.pcap_write(slab, offsets, lens, select=r.sel)
    """

    def __init__(self, parser, patterns, nocase=False, groups=None, actions=None, default=0):
        from . import _lib
        self._lib = _lib
        self._L = _lib.load()
        self.parser = parser
        self.blob, self.table = scan_patterns(patterns, nocase, groups, actions)
        self.default = int(default)
        n = self.table.size
        bp = self.blob.ctypes.data if self.blob.size else None
        tp = self.table.ctypes.data if n else None
        h = ctypes.c_void_p()
        if parser is None:
            rc = self._L.pkt_scan_create_host(bp, self.blob.size, tp, n, self.default, ctypes.byref(h))
            if rc != 0:
                msg = self._L.pkt_scan_last_error(None)
                raise ValueError(f"pkt_scan_create_host failed ({rc}): {msg.decode() if msg else ''}")
        else:
            parser._check(self._L.pkt_scan_create(parser._ctx, bp, self.blob.size, tp, n, self.default, ctypes.byref(h)),
                          "pkt_scan_create")
        self._t = h

    def __len__(self):
        return int(self.table.size)

    def _check(self, rc, what):
        if rc != 0:
            msg = self._L.pkt_scan_last_error(self._t)
            raise RuntimeError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")

    def run(self, batch, chain=None, region="payload", select=None,
            want=("status", "pat", "off", "action", "sel", "count", "matched"), hits=None, stream=None):
        """pkt_scan_batch: search every packet's region for the set -> ScanResult with the `want`ed arrays.  `region`:
        "payload" (the bytes after every header of `chain`, the chain columns of a parse of the batch) or "packet"
        (the whole packet; `chain` may be None).  `select` (uint8 [n]): a packet whose byte is 0 is skipped.  `hits`:
        True allocates zeroed uint64 [npatterns + 1] counters, an array passed in is accumulated into.  `batch`: the
        forms Lpm.lookup takes (a dict, PcapStream.batch()'s tuple), or a FragResult / ReasmResult.  Device tensors
        for a device handle, numpy arrays for a host handle.  Asynchronous on `stream`."""
        if hasattr(batch, "batch") and callable(batch.batch):
            batch = batch.batch()
        if isinstance(batch, (tuple, list)):
            batch = dict(zip(("slab", "offsets", "lens"), batch))
        bad = set(want) - {k for k, _ in _SCAN_OUT}
        if bad:
            raise ValueError(f"scanner: unknown outputs {sorted(bad)}")
        reg = schema.SCAN_REGION[region] if isinstance(region, str) else int(region)
        g = lambda k: batch.get(k)  # noqa: E731
        host = self.parser is None
        keep = []
        ch = None
        if host:
            b, arrs = _host_batch(self._lib, batch)
            keep.append(arrs)
            if chain is not None:
                cols = (np.ascontiguousarray(chain["n_hdrs"], np.uint8), np.ascontiguousarray(chain["hdr_type"], np.uint8),
                        np.ascontiguousarray(chain["hdr_off"], np.uint16))
                keep.append(cols)
                ch = self._lib.PktChain(*[c.ctypes.data for c in cols])
            if select is not None:
                select = np.ascontiguousarray(select, np.uint8)
            res = {k: np.zeros(b.n, dt) for k, dt in _SCAN_OUT if k in want}
            if hits is True:
                hits = np.zeros(len(self) + 1, np.uint64)
            ptr = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
        else:
            torch = _torch()
            b = self.parser._batch(batch["slab"], g("n"), g("stride"), g("offsets"), g("lens"))
            if chain is not None:
                ch = self.parser._chain(chain)
            if select is not None:
                assert select.is_cuda and select.dtype == torch.uint8 and select.numel() >= b.n
            dev = self.parser.torch_device
            res = {k: torch.empty(b.n, dtype=_tdtype(dt), device=dev) for k, dt in _SCAN_OUT if k in want}
            if hits is True:
                hits = torch.zeros(len(self) + 1, dtype=_tdtype(np.uint64), device=dev)
            elif hits is not None:
                assert hits.is_cuda and hits.element_size() == 8 and hits.numel() >= len(self) + 1
            ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None  # noqa: E731
        self._check(self._L.pkt_scan_batch(self._t, ctypes.byref(b), None if ch is None else ctypes.byref(ch), reg,
                                           ptr(select), *[ptr(res.get(k)) for k, _ in _SCAN_OUT], ptr(hits),
                                           None if host else self.parser._stream(stream)), "pkt_scan_batch")
        return ScanResult(hits=hits, **res)

    @property
    def info(self):
        """pkt_scan_info -> {"npatterns", "nstates", "max_len", "placement", "table_bytes"}."""
        i = self._lib.PktScanInfo()
        self._check(self._L.pkt_scan_info(self._t, ctypes.byref(i)), "pkt_scan_info")
        return {k: int(getattr(i, k)) for k, _ in i._fields_}

    def close(self):
        if getattr(self, "_t", None):
            self._L.pkt_scan_destroy(self._t)
            self._t = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HeaderSlice:
    """A `<Hdr>Slice` (headers.rs:172-296): a name and a view of `len()` bytes of the packet.
    Field getters are generated from the header's make_header! table."""

    def __init__(self, hdr_type, data):
        self.hdr_type = hdr_type
        self._data = data

    def name(self):
        return HDR_NAMES[self.hdr_type]

    def len(self):
        return HDR_SIZES[self.hdr_type]

    def as_slice(self):
        return bytes(self._data[:self.len()])

    def bit_range(self, msb, lsb):
        """headers.rs:253-263 (release semantics for widths > 64, Q8)."""
        v = 0
        for i in range(lsb, msb + 1):
            v = (v << 1) | ((self._data[i // 8] >> (7 - i % 8)) & 1)
        w = msb - lsb + 1
        v &= (1 << 64) - 1
        sh = (64 - w) & 63
        return ((v << sh) & ((1 << 64) - 1)) >> sh

    def bytes(self, msb, lsb):
        return bytes(self.bit_range(i + 7, i) for i in range(lsb, msb + 1, 8))

    def __getattr__(self, field):
        from . import fields
        rng = fields.FIELDS.get(self.hdr_type, {}).get(field)
        if rng is None:
            raise AttributeError(field)
        return lambda: self.bit_range(rng[1], rng[0])


class PacketSlice:
    """packet_rs::PacketSlice (lib.rs:136-140, packet.rs:714-761) over one parsed packet."""

    def __init__(self, hdrs, payload):
        self.hdrs = hdrs
        self._payload = payload

    def payload(self):
        return self._payload

    def len(self):
        return sum(h.len() for h in self.hdrs) + len(self._payload)

    def to_vec(self):
        return b"".join(h.as_slice() for h in self.hdrs) + bytes(self._payload)

    def __getitem__(self, name):  # first match, like Packet's Index<&str> (packet.rs:64-66)
        for h in self.hdrs:
            if h.name() == name:
                return h
        raise KeyError(name)


def view(res, i):
    """pkt_view (the C ABI's PacketSlice of packet i) over host (numpy) chain columns:
    (status, [(hdr_type, offset)], payload_off, payload_len); no headers unless status is OK."""
    from . import _lib
    L = _lib.load()
    need = ("status", "n_hdrs", "hdr_type", "hdr_off", "payload_off", "payload_len")
    cols = {c: np.ascontiguousarray(res[c]) for c in need}
    n = cols["status"].shape[0]
    o = _lib.PktOut()
    for c in need:
        setattr(o, c, cols[c].ctypes.data)
    ty, of = (ctypes.c_uint8 * MAX_HDRS)(), (ctypes.c_uint16 * MAX_HDRS)()
    nh, po, pl = ctypes.c_uint32(), ctypes.c_uint16(), ctypes.c_uint16()
    rc = L.pkt_view(ctypes.byref(o), n, int(i), ty, of, ctypes.byref(nh), ctypes.byref(po), ctypes.byref(pl))
    if rc < 0:
        raise ValueError(f"pkt_view({i}) failed ({rc})")
    return rc, [(ty[k], of[k]) for k in range(nh.value)], po.value, pl.value


def packet_slice(res, i, pkt):
    """Build the PacketSlice of packet i from host (numpy) result columns and its bytes, through
    pkt_view (the same per-packet view a Rust caller builds its PacketSlice from)."""
    st, hl, po, pl = view(res, i)
    if st != OK:
        raise ValueError(f"packet {i}: {STATUS_NAMES[st]} (the reference panics)")
    pkt = bytes(pkt)
    hdrs = [HeaderSlice(t, memoryview(pkt)[o:]) for t, o in hl]
    return PacketSlice(hdrs, pkt[po:po + pl])
