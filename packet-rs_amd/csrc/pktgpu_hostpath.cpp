// pktgpu_hostpath.cpp — every path of the C ABI (include/pktgpu.h) that reads or writes host memory:
// pkt_host_alloc / _free, pkt_parse_host, pkt_parse_pcap_host[_async / _result] and pkt_pcap_stream_* (the
// window's release included).
// Host code only: it launches no kernel of its own, but queues copies and the internal entries of
// pktgpu_ctx.hpp (pktgpu_parse, the pcap indexer, the column export) on the ctx's three host streams.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "pktgpu_ctx.hpp"
#include "pktgpu_device.hpp"  // kLaunchChunk, kMaxSpread

using pktgpu::kLaunchChunk;
using pktgpu::kMaxSpread;

namespace {

// Is `p` pinned host memory the device can address?  On success `dev` = its device address.
template <class T>
bool host_mapped(const T* p, const T*& dev) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();  // pageable memory: not an error for the caller
        return false;
    }
    if (a.type != hipMemoryTypeHost || !a.devicePointer) return false;
    dev = reinterpret_cast<const T*>(a.devicePointer);
    return true;
}

// Grow one device buffer of every pipeline slot to `need` bytes (all slots idle: the caller has
// synchronised the pipeline streams).
template <class T>
hipError_t grow(T* (&buf)[HostPipe::kSlots], uint64_t& cap, uint64_t need) {
    if (need <= cap) return hipSuccess;
    for (int k = 0; k < HostPipe::kSlots; k++) {
        if (buf[k]) (void)hipFree(buf[k]);
        buf[k] = nullptr;
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&buf[k]), need);
        if (e != hipSuccess) { cap = 0; return e; }
    }
    cap = need;
    return hipSuccess;
}

// The packed device layout of the requested columns of `out` for n packets (slot columns: PKT_MAX_HDRS
// rows of n): column c at byte off[c], each at a 256-byte boundary.  Returns the layout's bytes.
uint64_t packed_layout(const pkt_out_t* out, uint64_t n, uint64_t (&off)[kNumCols]) {
    const void* const* col = reinterpret_cast<const void* const*>(out);
    uint64_t bytes = 0;
    for (int c = 0; c < kNumCols; c++) {
        off[c] = bytes;
        if (col[c]) bytes += (col_bytes(c, n) + 255) & ~(uint64_t)255;
    }
    return bytes;
}

// xa.col / xa.ncol: one row per requested per-packet column, PKT_MAX_HDRS per slot column, from the device
// columns `dev` (slot rows dstride elements apart) to the device-mapped host columns `host` (slot rows
// hstride elements apart), the host side starting at element h0.
void export_table(ExportArgs& xa, const pkt_out_t& dev, const pkt_out_t& host, uint64_t dstride, uint64_t hstride,
                  uint64_t h0) {
    const uint8_t* const* dc = reinterpret_cast<const uint8_t* const*>(&dev);
    const uint8_t* const* hc = reinterpret_cast<const uint8_t* const*>(&host);
    xa.ncol = 0;
    for (int c = 0; c < kNumCols; c++) {
        if (!dc[c]) continue;
        const bool slot = c == kColHdrType || c == kColHdrOff;
        const uint64_t sz = kColSize[c];
        for (uint32_t r = 0; r < (slot ? (uint32_t)PKT_MAX_HDRS : 1u); r++)
            xa.col[xa.ncol++] = ExportCol{reinterpret_cast<uint64_t>(dc[c]) + (uint64_t)r * dstride * sz,
                                          reinterpret_cast<uint64_t>(hc[c]) + ((uint64_t)r * hstride + h0) * sz,
                                          (uint32_t)sz, slot ? r : kExportNoRow};
    }
}

}  // namespace

// The staged host pipeline: the batch cut into chunks of `cn` packets over the ctx's three streams,
// each chunk parsed into a device output slot and its columns copied to the host rows (the slot rows
// once the chunk's n_hdrs maximum, reduced inside its parse, is known — one chunk later, so the host
// never waits on the chunk it has just queued).  dev_in = false: `b` is host memory and each chunk's
// bytes (+ offsets / lens) are copied in first; dev_in = true: `b` is already in device memory.
// hout (non-NULL: every requested host column is pinned, these are their device-mapped addresses): each
// chunk's columns leave by one export_kernel launch writing 16-byte chunks over the link (pktgpu_gather.hip)
// instead of one DMA copy per column — ~30 small copies per chunk, each with its own setup.
static int staged_parse(pkt_ctx_t* ctx, const pkt_batch_t* b, int entry, const pkt_out_t* out, uint64_t chunk,
                        bool dev_in, uint64_t slot_stride = 0, const pkt_out_t* hout = nullptr) {
    HostPipe& hp = ctx->hp;
    hipError_t e = hipSuccess;
    const uint64_t n = b->n, hstride = slot_stride ? slot_stride : n;  // host slot rows: [16][hstride]
    const uint64_t cn = std::min<uint64_t>(chunk ? chunk : (hout ? (1ull << 17) : (1ull << 18)), n);
    const uint64_t nchunks = (n + cn - 1) / cn;

    // bytes of input each chunk needs on the device (indexed: the span its records cover,
    // from the 16-byte-aligned start of the first)
    auto span = [&](uint64_t lo, uint64_t hi, uint64_t& base, uint64_t& bytes) {
        uint64_t a = UINT64_MAX, z = 0;
        if (b->offsets) {
            for (uint64_t i = lo; i < hi; i++) {
                a = std::min(a, b->offsets[i]);
                z = std::max(z, b->offsets[i] + b->lens[i]);
            }
        } else {
            a = lo * (uint64_t)b->stride;
            z = hi * (uint64_t)b->stride;
        }
        a = std::min(a, b->slab_len);
        if (b->offsets) a &= ~(uint64_t)15;  // fixed stride: the chunk starts at its first packet
        z = std::min(z, b->slab_len);
        base = a;
        bytes = z > a ? z - a : 0;
    };
    uint64_t slab_need = 16;
    if (!dev_in)
        for (uint64_t k = 0; k < nchunks; k++) {
            uint64_t base, bytes;
            span(k * cn, std::min(n, (k + 1) * cn), base, bytes);
            slab_need = std::max(slab_need, bytes);
        }
    // device output layout of one chunk: the requested columns, packed, 256-byte aligned
    const uint8_t* const* hcol = reinterpret_cast<const uint8_t* const*>(out);
    uint64_t col_off[kNumCols];
    const uint64_t out_need = packed_layout(out, cn, col_off);
    for (int k = 0; k < HostPipe::kSlots; k++) (void)hipStreamSynchronize(hp.s[k]);
    if ((!dev_in && (e = grow(hp.slab, hp.slab_cap, (slab_need + 15) & ~(uint64_t)15)) != hipSuccess) ||
        (e = grow(hp.out, hp.out_cap, std::max<uint64_t>(out_need, 256))) != hipSuccess)
        return hip_fail(ctx, e, "hipMalloc (host pipeline)");
    if (!dev_in && (b->offsets || b->lens)) {
        uint64_t cap8 = hp.pkt_cap, cap4 = hp.pkt_cap;
        if ((e = grow(hp.offs, cap8, cn * 8)) != hipSuccess || (e = grow(hp.lens, cap4, cn * 8)) != hipSuccess)
            return hip_fail(ctx, e, "hipMalloc (host pipeline)");
        hp.pkt_cap = std::min(cap8, cap4);
    }

    // Slot rows move only as far as each chunk's largest n_hdrs (when n_hdrs is requested)
    const bool slot_rows = (hcol[kColHdrType] || hcol[kColHdrOff]) && hcol[1] != nullptr;
    if (slot_rows && (e = pktgpu_ensure_max_scratch(ctx)) != hipSuccess) return hip_fail(ctx, e, "max scratch");
    auto copy_slots = [&](uint64_t kk) -> hipError_t {  // chunk kk's slot rows [0, R) to the host
        const int q = (int)(kk % HostPipe::kSlots);
        const uint64_t lo = kk * cn, m = std::min(n, lo + cn) - lo;
        uint32_t rows = PKT_MAX_HDRS;
        if (slot_rows) {
            hipError_t es = hipEventSynchronize(hp.ev[q]);
            if (es != hipSuccess) return es;
            rows = std::min<uint32_t>(ctx->mx.host_max(q), PKT_MAX_HDRS);
        }
        for (int c : {kColHdrType, kColHdrOff}) {
            if (!hcol[c] || !rows) continue;
            const uint64_t sz = kColSize[c];
            hipError_t es = hipMemcpy2DAsync(const_cast<uint8_t*>(hcol[c]) + lo * sz, hstride * sz, hp.out[q] + col_off[c],
                                             m * sz, m * sz, rows, hipMemcpyDeviceToHost, hp.s[q]);
            if (es != hipSuccess) return es;
        }
        return hipSuccess;
    };
    int rc = PKT_SUCCESS;
    for (uint64_t k = 0; k < nchunks && rc == PKT_SUCCESS; k++) {
        const int q = (int)(k % HostPipe::kSlots);
        hipStream_t s = hp.s[q];
        const uint64_t lo = k * cn, hi = std::min(n, lo + cn), m = hi - lo;
        pkt_batch_t db;
        uint64_t bias = 0;
        if (dev_in) {
            db = *b;
            if (b->offsets) {
                db.offsets = b->offsets + lo;
                db.lens = b->lens + lo;
            } else {
                const uint64_t a = std::min<uint64_t>(lo * (uint64_t)b->stride, b->slab_len);
                db.slab = b->slab + a;  // 16-byte aligned: stride % 16 == 0 is checked by the caller
                db.slab_len = std::max<uint64_t>(b->slab_len - a, 16);
                if (b->lens) db.lens = b->lens + lo;
            }
            db.n = m;
        } else {
            uint64_t base, bytes;
            span(lo, hi, base, bytes);
            // in: the chunk's bytes (+ offsets / lens)
            if (bytes) e = hipMemcpyAsync(hp.slab[q], b->slab + base, bytes, hipMemcpyHostToDevice, s);
            if (e == hipSuccess && b->offsets)
                e = hipMemcpyAsync(hp.offs[q], b->offsets + lo, m * 8, hipMemcpyHostToDevice, s);
            if (e == hipSuccess && b->lens)
                e = hipMemcpyAsync(hp.lens[q], b->lens + lo, m * 4, hipMemcpyHostToDevice, s);
            if (e != hipSuccess) { rc = hip_fail(ctx, e, "hipMemcpyAsync H2D"); break; }
            // a chunk whose records cover no byte still parses (all TRUNCATED) against a 1-byte view;
            // fixed-stride chunks index from the chunk's first packet
            db.slab = hp.slab[q];
            db.slab_len = std::max<uint64_t>(bytes, 1);
            db.offsets = b->offsets ? hp.offs[q] : nullptr;
            db.lens = b->lens ? hp.lens[q] : nullptr;
            db.stride = b->stride;
            db.reserved = 0;
            db.n = m;
            bias = b->offsets ? base : 0;
        }
        pkt_out_t dout;
        uint8_t** dcol = reinterpret_cast<uint8_t**>(&dout);
        for (int c = 0; c < kNumCols; c++) dcol[c] = hcol[c] ? hp.out[q] + col_off[c] : nullptr;
        // (the device buffer always has >= 16 readable bytes, so a view shorter than 16 is safe)
        if (slot_rows && (e = hipMemsetAsync(ctx->mx.dgroup(q), 0, MaxScratch::kSpread * sizeof(uint32_t), s)) != hipSuccess) {
            rc = hip_fail(ctx, e, "hipMemsetAsync");
            break;
        }
        ParseOpts po;
        po.off_bias = bias;
        po.nh_max = slot_rows ? ctx->mx.dgroup(q) : nullptr;
        rc = pktgpu_parse(ctx, &db, entry, &dout, s, po);
        if (rc != PKT_SUCCESS) break;
        if (hout) {  // every column of the chunk by one export launch (slot rows up to the chunk's n_hdrs max)
            ExportArgs xa;
            xa.lo_dev = xa.hi_dev = nullptr;
            xa.lo_h = 0;
            xa.hi_h = m;
            xa.cap = m;
            xa.nhw = po.nh_max;
            export_table(xa, dout, *hout, m, hstride, lo);
            if ((e = pktgpu_export_launch(xa, s)) != hipSuccess) {
                rc = hip_fail(ctx, e, "export_kernel");
                break;
            }
            continue;
        }
        // out: every requested per-packet column into its host rows [lo, hi); the slot rows of this
        // chunk once its count is known (after the next chunk is queued)
        for (int c = 0; c < kNumCols && e == hipSuccess; c++) {
            if (!hcol[c] || c == kColHdrType || c == kColHdrOff) continue;
            const uint64_t sz = kColSize[c];
            e = hipMemcpyAsync(const_cast<uint8_t*>(hcol[c]) + lo * sz, dcol[c], m * sz, hipMemcpyDeviceToHost, s);
        }
        if (e == hipSuccess && slot_rows) {
            e = hipMemcpyAsync(ctx->mx.hgroup(q), ctx->mx.dgroup(q), MaxScratch::kSpread * sizeof(uint32_t),
                               hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipEventRecord(hp.ev[q], s);
        }
        if (e == hipSuccess && k > 0) e = copy_slots(k - 1);
        if (e != hipSuccess) rc = hip_fail(ctx, e, "hipMemcpyAsync D2H");
    }
    if (rc == PKT_SUCCESS && nchunks > 0 && !hout) {
        e = copy_slots(nchunks - 1);
        if (e != hipSuccess) rc = hip_fail(ctx, e, "hipMemcpyAsync D2H");
    }
    for (int k = 0; k < HostPipe::kSlots; k++) {
        hipError_t es = hipStreamSynchronize(hp.s[k]);
        if (es != hipSuccess && rc == PKT_SUCCESS) rc = hip_fail(ctx, es, "hipStreamSynchronize");
    }
    return rc;
}

static int host_pipe_init(pkt_ctx_t* ctx) {
    HostPipe& hp = ctx->hp;
    if (hp.init) return PKT_SUCCESS;
    for (int k = 0; k < HostPipe::kSlots; k++) {
        hipError_t e = hipStreamCreateWithFlags(&hp.s[k], hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&hp.ev[k], hipEventDisableTiming);
        if (e != hipSuccess) return hip_fail(ctx, e, "hipStreamCreate");
    }
    hp.init = true;
    return PKT_SUCCESS;
}

// Are the requested columns of `out` all pinned host memory mapped into the device?  `dout` = the
// same columns by their device addresses.
static bool out_mapped(const pkt_out_t* out, pkt_out_t& dout) {
    dout = *out;
    const uint8_t** dc = reinterpret_cast<const uint8_t**>(&dout);
    bool mapped = true;
    for (int c = 0; c < kNumCols && mapped; c++)
        if (dc[c]) mapped = host_mapped(dc[c], dc[c]);
    return mapped;
}

extern "C" {

int pkt_host_alloc(pkt_ctx_t* ctx, uint64_t bytes, void** p) {
    if (!ctx || !p) return fail(ctx, PKT_ERR_INVALID_ARG, "null argument");
    *p = nullptr;
    hipError_t e = hipSetDevice(ctx->device);
    if (e == hipSuccess) e = hipHostMalloc(p, bytes ? bytes : 1, hipHostMallocDefault);
    return e == hipSuccess ? PKT_SUCCESS : hip_fail(ctx, e, "hipHostMalloc");
}

int pkt_host_free(pkt_ctx_t* ctx, void* p) {
    if (!p) return PKT_SUCCESS;
    hipError_t e = hipHostFree(p);
    return e == hipSuccess ? PKT_SUCCESS : hip_fail(ctx, e, "hipHostFree");
}

int pkt_parse_host(pkt_ctx_t* ctx, const pkt_batch_t* b, int entry, const pkt_out_t* out, uint64_t chunk) {
    if (!ctx || !b || !out) return fail(ctx, PKT_ERR_INVALID_ARG, "null argument");
    if (entry < 0 || entry >= PKT_ENTRY_COUNT) return fail(ctx, PKT_ERR_INVALID_ARG, "bad entry");
    if (b->n == 0) return PKT_SUCCESS;
    if (!b->slab || b->slab_len == 0) return fail(ctx, PKT_ERR_INVALID_ARG, "null or empty slab");
    int rc = check_batch_index(ctx, b);
    if (rc != PKT_SUCCESS) return rc;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    rc = host_pipe_init(ctx);
    if (rc != PKT_SUCCESS) return rc;
    HostPipe& hp = ctx->hp;
    // Zero copy: when the slab, the index arrays and every requested column are pinned host memory
    // mapped into the device (pkt_host_alloc), the kernel reads and writes them over PCIe directly —
    // one launch, no staging copies, both link directions busy at once.  (Chunks copied
    // in by DMA, parsed on the device and their columns exported by a kernel writing 16-byte chunks —
    // the route the piecewise capture takes — measured slower here: C2 2.10 vs 1.86 ms, C4 6.63 vs
    // 6.28 ms per 2^20 packets, profiles/host/r05e_host_export_vs_zero_copy.jsonl; it serves pinned
    // columns of a pageable slab instead of one DMA copy per column.)
    pkt_batch_t db = *b;
    pkt_out_t dout;
    const bool omap = out_mapped(out, dout);
    const bool mapped = omap && host_mapped(b->slab, db.slab) && (!b->offsets || host_mapped(b->offsets, db.offsets)) &&
                        (!b->lens || host_mapped(b->lens, db.lens));
    if (omap && !(mapped && ((uintptr_t)db.slab & 15) == 0 && b->slab_len >= 16))
        return staged_parse(ctx, b, entry, out, chunk, false, 0, &dout);
    if (mapped && ((uintptr_t)db.slab & 15) == 0 && b->slab_len >= 16) {
        // wave spans read the link in 1-KiB contiguous pieces and never go back to host memory
        // for a deep header (per-lane windows would, one dependent PCIe read each)
        ParseOpts po;
        po.staging = ctx->staging == 0 ? 2 : ctx->staging;
        rc = pktgpu_parse(ctx, &db, entry, &dout, hp.s[0], po);
        if (rc != PKT_SUCCESS) return rc;
        e = hipStreamSynchronize(hp.s[0]);
        return e == hipSuccess ? PKT_SUCCESS : hip_fail(ctx, e, "hipStreamSynchronize");
    }
    return staged_parse(ctx, b, entry, out, chunk, false);
}

}  // extern "C"

// The host pipeline's streams and the capture's device buffers (file + index, grown on demand; +16:
// the kernels' readable tail), after the ctx's earlier host-path work has finished.
static int pcap_host_buffers(pkt_ctx_t* ctx, uint64_t len, uint64_t cap) {
    if (ctx->pc.pending)
        return fail(ctx, PKT_ERR_INVALID_ARG, "a queued capture's outcome has not been taken on this ctx (pkt_parse_pcap_result)");
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    int rc = host_pipe_init(ctx);
    if (rc != PKT_SUCCESS) return rc;
    HostPipe& hp = ctx->hp;
    for (int k = 0; k < HostPipe::kSlots; k++) (void)hipStreamSynchronize(hp.s[k]);
    const uint64_t fbytes = ((len + 15) & ~(uint64_t)15) + 16;
    if (fbytes > hp.file_cap) {
        (void)hipFree(hp.file);
        hp.file = nullptr;
        hp.file_cap = 0;
        if ((e = hipMalloc(reinterpret_cast<void**>(&hp.file), fbytes + fbytes / 4)) != hipSuccess)
            return hip_fail(ctx, e, "hipMalloc (pcap file)");
        hp.file_cap = fbytes + fbytes / 4;
    }
    if (cap > hp.idx_cap) {
        (void)hipFree(hp.ioffs);
        (void)hipFree(hp.ilens);
        hp.ioffs = nullptr;
        hp.ilens = nullptr;
        hp.idx_cap = 0;
        const uint64_t c2 = cap + cap / 4;
        e = hipMalloc(reinterpret_cast<void**>(&hp.ioffs), c2 * 8);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&hp.ilens), c2 * 4);
        if (e != hipSuccess) return hip_fail(ctx, e, "hipMalloc (pcap index)");
        hp.idx_cap = c2;
    }
    return PKT_SUCCESS;
}

// The first n records of those buffers' capture, as indexed, within its first `len` bytes.
static pkt_batch_t pcap_host_batch(const HostPipe& hp, uint64_t len, uint64_t n) {
    return pkt_batch_t{hp.file, len, hp.ioffs, hp.ilens, 0, 0, n};
}

// A capture indexed and parsed as its bytes arrive (pkt_parse_pcap_host's pieces, pkt_pcap_stream_*), on
// the ctx's three host streams: hp.s[1] copies bytes in; hp.s[0] runs one STEP per batch of new bytes —
// the device indexer over the new regions only (segment mode: it starts from the previous step's carry,
// the first record start that step did not count and its record count, kept in device words, so the
// whole capture is indexed once, O(file), however many steps) and the parse of the records the step
// added into the device columns; hp.s[2] exports those records' column ranges to the caller's pinned
// columns in 16-byte chunks while the next bytes copy in (the link is full duplex).  The parse kernel
// writing the host columns itself (its 1-8 B per-lane stores over the link) moved them at ~21 GB/s
// against ~57 GB/s for wide chunks (profiles/host/r05b_pcap_host_pieces.jsonl).  The records a step adds
// all end in (its start, its end] and are disjoint (>= 16 B each): at most (end - start) / 16 + 1 of
// them, which sizes the step's parse grid.  Nothing on the host waits for the device between steps.
struct Ingest {
    pkt_ctx_t* ctx = nullptr;
    int entry = 0;
    uint64_t cap = 0;      // records the columns hold (slot rows strided by cap)
    pkt_out_t dcols{};     // the parse's output: the caller's device columns or the ctx's hp.dcol
    bool exporting = false;
    ExportArgs xa{};       // exporting: hp.dcol -> the caller's pinned columns
    uint64_t hi = 0;       // bytes copied to the device (hp.file[0, hi)), queued
    uint64_t indexed = 0;  // the prefix the last step indexed
    uint64_t steps = 0;
    uint64_t copies = 0;   // copies queued; copy c ends the capture's first copy_end[c % kCopyRing] bytes
    uint64_t copy_end[HostPipe::kCopyRing] = {};
    int rc = PKT_SUCCESS;  // the first failure (every later call returns it)
};
constexpr uint64_t kHostPiece = 16ull << 20;  // pkt_parse_pcap_host: default bytes per copied piece

static int ingest_fail(Ingest& ig, int code) {  // nothing left in flight that reads the caller's bytes
    HostPipe& hp = ig.ctx->hp;
    for (int k = 0; k < HostPipe::kSlots; k++) (void)hipStreamSynchronize(hp.s[k]);
    if (ig.rc == PKT_SUCCESS) ig.rc = code;
    return code;
}

// The buffers, ring and events of a capture of up to len_cap bytes and cap records into `out`: pinned host
// columns (hout = their device addresses: the parse writes hp.dcol, exported after each step) or the
// caller's device columns (hout NULL: the parse writes them).  Waits for the ctx's earlier host-path work.
static int ingest_begin(Ingest& ig, pkt_ctx_t* ctx, uint64_t len_cap, uint64_t cap, int entry, const pkt_out_t* out,
                        const pkt_out_t* hout) {
    ig.ctx = ctx;
    ig.entry = entry;
    ig.cap = cap;  // (a fresh Ingest: nothing copied, indexed or failed yet)
    int rc = pcap_host_buffers(ctx, len_cap, cap);
    if (rc != PKT_SUCCESS) return rc;
    HostPipe& hp = ctx->hp;
    hipError_t e = hipSuccess;
    if (!hp.pcarry) e = hipMalloc(reinterpret_cast<void**>(&hp.pcarry), HostPipe::kRing * kPcapCarryWords * 8);
    if (e == hipSuccess && !hp.pnh) e = hipMalloc(reinterpret_cast<void**>(&hp.pnh), HostPipe::kRing * kMaxSpread * 4);
    for (int j = 0; j < HostPipe::kCopyRing && e == hipSuccess; j++)
        if (!hp.ev_copy[j]) e = hipEventCreateWithFlags(&hp.ev_copy[j], hipEventDisableTiming);
    if (e == hipSuccess && !hp.ev_parsed) e = hipEventCreateWithFlags(&hp.ev_parsed, hipEventDisableTiming);
    for (int j = 0; j < HostPipe::kRing && e == hipSuccess; j++)
        if (!hp.ev_xdone[j]) e = hipEventCreateWithFlags(&hp.ev_xdone[j], hipEventDisableTiming);
    if (e != hipSuccess) return hip_fail(ctx, e, "capture ring");
    ig.exporting = hout != nullptr;
    if (!ig.exporting) {
        ig.dcols = *out;
    } else {
        // the device columns: the requested ones, each at a 256-byte boundary, the caller's shapes
        const uint8_t* const* hcol = reinterpret_cast<const uint8_t* const*>(out);
        uint64_t coff[kNumCols];
        const uint64_t need = packed_layout(out, cap, coff);
        if (need > hp.dcol_cap) {
            (void)hipFree(hp.dcol);
            hp.dcol = nullptr;
            hp.dcol_cap = 0;
            if ((e = hipMalloc(reinterpret_cast<void**>(&hp.dcol), need)) != hipSuccess)
                return hip_fail(ctx, e, "hipMalloc (capture columns)");
            hp.dcol_cap = need;
        }
        uint8_t** dc = reinterpret_cast<uint8_t**>(&ig.dcols);
        for (int c = 0; c < kNumCols; c++) dc[c] = hcol[c] ? hp.dcol + coff[c] : nullptr;
        ig.xa.cap = cap;
        ig.xa.lo_h = ig.xa.hi_h = 0;
        export_table(ig.xa, ig.dcols, *hout, cap, cap, 0);  // (hout: the host columns' device-mapped addresses)
    }
    return pktgpu_pcap_reserve(ctx, len_cap, hp.s[0]);  // the whole capture's scratch: no growth between steps
}

// Copy the next n bytes of the capture in (hp.s[1], asynchronous: `src` must stay valid until the copy has
// landed, ingest_copied).
static int ingest_copy(Ingest& ig, const uint8_t* src, uint64_t n) {
    if (ig.rc != PKT_SUCCESS) return ig.rc;
    HostPipe& hp = ig.ctx->hp;
    const uint32_t c = (uint32_t)(ig.copies % HostPipe::kCopyRing);
    hipError_t e = hipMemcpyAsync(hp.file + ig.hi, src, n, hipMemcpyHostToDevice, hp.s[1]);
    if (e == hipSuccess) e = hipEventRecord(hp.ev_copy[c], hp.s[1]);
    if (e != hipSuccess) return ingest_fail(ig, hip_fail(ig.ctx, e, "hipMemcpyAsync H2D (capture bytes)"));
    ig.hi += n;
    ig.copy_end[c] = ig.hi;
    ig.copies++;
    return PKT_SUCCESS;
}

// The event of the queued copy that ends the first `upto` bytes (one of the last kCopyRing copies).
static hipEvent_t ingest_copied(const Ingest& ig, uint64_t upto) {
    for (uint64_t c = ig.copies; c > 0 && c + HostPipe::kCopyRing > ig.copies; c--)
        if (ig.copy_end[(c - 1) % HostPipe::kCopyRing] == upto) return ig.ctx->hp.ev_copy[(c - 1) % HostPipe::kCopyRing];
    return nullptr;
}

// One step over the first `upto` bytes (0: every byte copied so far; `upto` ends a queued copy among the
// last kCopyRing) (last: the capture is complete — a record running past its end is the capture's error;
// otherwise such a record waits for the next step).  Needs upto >= 24.
static int ingest_step(Ingest& ig, bool last, uint64_t upto = 0) {
    if (ig.rc != PKT_SUCCESS) return ig.rc;
    pkt_ctx_t* ctx = ig.ctx;
    HostPipe& hp = ctx->hp;
    hipStream_t ps = hp.s[0], es = hp.s[2];
    constexpr uint32_t R = HostPipe::kRing;
    const uint64_t k = ig.steps;
    const uint32_t j = (uint32_t)(k % R), jp = (uint32_t)((k + R - 1) % R);
    const uint64_t hi = upto ? upto : ig.hi;
    const uint64_t region = pktgpu_pcap_region_bytes(), K = (hi + region - 1) / region;
    // the segment: from the region holding the previous step's end (its carry decides the exact entry),
    // at least the last region (a final step with no new bytes still decides the carried record)
    const uint32_t r0 = k ? (uint32_t)std::min<uint64_t>(ig.indexed / region, K - 1) : 0u;
    const hipEvent_t landed = ingest_copied(ig, hi);
    if (!landed || hi < ig.indexed) return ingest_fail(ig, fail(ctx, PKT_ERR_INVALID_ARG, "capture step past its copies"));
    hipError_t e = hipStreamWaitEvent(ps, landed, 0);
    // the ring slot this step writes was last read by step k - R + 1's export
    if (e == hipSuccess && ig.exporting && k + 1 >= R) e = hipStreamWaitEvent(ps, hp.ev_xdone[(k + 1) % R], 0);
    if (e != hipSuccess) return ingest_fail(ig, hip_fail(ctx, e, "hipStreamWaitEvent (capture step)"));
    uint64_t* carry = hp.pcarry + (uint64_t)j * kPcapCarryWords;
    const uint64_t* cin = k ? hp.pcarry + (uint64_t)jp * kPcapCarryWords : nullptr;
    const uint64_t* cnt = nullptr;
    int rc = pktgpu_pcap_launch(ctx, hp.file, hi, hp.ioffs, hp.ilens, ig.cap, ps, &cnt, !last, carry + 1, r0, cin, carry);
    if (rc != PKT_SUCCESS) return ingest_fail(ig, rc);
    const pkt_batch_t db = pcap_host_batch(hp, hi, ig.cap);  // the prefix: every record parsed here lies inside it
    uint32_t* nh = ig.exporting ? hp.pnh + (uint64_t)j * kMaxSpread : nullptr;
    if (nh && (e = hipMemsetAsync(nh, 0, kMaxSpread * 4, ps)) != hipSuccess)
        return ingest_fail(ig, hip_fail(ctx, e, "hipMemsetAsync"));
    // the records this step added: [the previous step's count, this step's count)
    ParseOpts po;
    po.nh_max = nh;
    po.slot_stride = ig.cap;
    po.n_dev = cnt;
    po.i0_dev = cin ? cin + 1 : nullptr;
    po.grid_n = (hi - ig.indexed) / 16 + 1;
    rc = pktgpu_parse(ctx, &db, ig.entry, &ig.dcols, ps, po);
    if (rc != PKT_SUCCESS) return ingest_fail(ig, rc);
    if (ig.exporting) {
        if ((e = hipEventRecord(hp.ev_parsed, ps)) != hipSuccess || (e = hipStreamWaitEvent(es, hp.ev_parsed, 0)) != hipSuccess)
            return ingest_fail(ig, hip_fail(ctx, e, "hipEventRecord (step parsed)"));
        ig.xa.lo_dev = cin ? cin + 1 : nullptr;
        ig.xa.hi_dev = cnt;
        ig.xa.nhw = nh;
        if ((e = pktgpu_export_launch(ig.xa, es)) != hipSuccess || (e = hipEventRecord(hp.ev_xdone[j], es)) != hipSuccess)
            return ingest_fail(ig, hip_fail(ctx, e, "export_kernel"));
    }
    ig.indexed = hi;
    ig.steps++;
    return PKT_SUCCESS;
}

// Wait for every queued step: the capture's outcome (pcap_finish: count, magic, a record past the end),
// the index of the first min(count, cap) records copied to offsets / lens (host, may be NULL).
static int ingest_wait(Ingest& ig, uint64_t* n_out, uint64_t* offsets, uint32_t* lens) {
    if (ig.rc != PKT_SUCCESS) return ig.rc;
    pkt_ctx_t* ctx = ig.ctx;
    HostPipe& hp = ctx->hp;
    hipError_t e = hipStreamSynchronize(hp.s[0]);
    if (e != hipSuccess) return ingest_fail(ig, hip_fail(ctx, e, "hipStreamSynchronize"));
    int rc = pktgpu_pcap_finish(ctx, n_out);
    if (rc != PKT_SUCCESS) return ingest_fail(ig, rc);
    const uint64_t m = std::min(*n_out, ig.cap);
    if (m && offsets && (e = hipMemcpyAsync(offsets, hp.ioffs, m * 8, hipMemcpyDeviceToHost, hp.s[1])) != hipSuccess)
        return ingest_fail(ig, hip_fail(ctx, e, "hipMemcpyAsync D2H (offsets)"));
    if (m && lens && (e = hipMemcpyAsync(lens, hp.ilens, m * 4, hipMemcpyDeviceToHost, hp.s[1])) != hipSuccess)
        return ingest_fail(ig, hip_fail(ctx, e, "hipMemcpyAsync D2H (lens)"));
    if ((e = hipStreamSynchronize(hp.s[1])) != hipSuccess || (e = hipStreamSynchronize(hp.s[2])) != hipSuccess)
        return ingest_fail(ig, hip_fail(ctx, e, "hipStreamSynchronize"));
    return PKT_SUCCESS;
}

// pkt_parse_pcap_host with pinned columns: the file copied in pieces of the ctx's host_piece bytes, one step
// per piece (n_out NULL, pkt_parse_pcap_host_async: everything queued, the capture left pending on the ctx).
static int pcap_host_pieces(pkt_ctx_t* ctx, const uint8_t* buf, uint64_t len, int entry, const pkt_out_t* out,
                            const pkt_out_t& hout, uint64_t* offsets, uint32_t* lens, uint64_t cap, uint64_t* n_out) {
    Ingest ig;
    int rc = ingest_begin(ig, ctx, len, cap, entry, out, &hout);
    if (rc != PKT_SUCCESS) return rc;
    // at most kMaxHostSteps pieces per capture: each step costs ~50 us of host API time (13 calls), so
    // tiny pieces over a large file would make the host the bottleneck (1 MiB pieces: 12.2 ms per 195 MB
    // against 4.8 ms at 16 MiB, r06)
    constexpr uint64_t kMaxHostSteps = 1024;
    const uint64_t piece = std::max<uint64_t>(ctx->host_piece ? ctx->host_piece : kHostPiece,
                                              (len + kMaxHostSteps - 1) / kMaxHostSteps);
    // the copies run kAhead pieces ahead of the steps that wait for them (queued before the step's
    // kernels on the host: a copy queued behind an export waited for that export's parse, r06e trace)
    constexpr uint64_t kAhead = 3;
    static_assert(kAhead < HostPipe::kCopyRing, "a step's copy is among the last kCopyRing");
    const uint64_t np = (len + piece - 1) / piece;
    for (uint64_t p = 0; p < np && p < kAhead; p++)
        if ((rc = ingest_copy(ig, buf + p * piece, std::min(len, (p + 1) * piece) - p * piece)) != PKT_SUCCESS) return rc;
    for (uint64_t p = 0; p < np; p++) {
        const uint64_t q = p + kAhead;
        if (q < np && (rc = ingest_copy(ig, buf + q * piece, std::min(len, (q + 1) * piece) - q * piece)) != PKT_SUCCESS)
            return rc;
        if ((rc = ingest_step(ig, p + 1 == np, std::min(len, (p + 1) * piece))) != PKT_SUCCESS) return rc;
    }
    if (!n_out) {
        ctx->pc.mark(ctx->hp.s[0]);
        return PKT_SUCCESS;
    }
    return ingest_wait(ig, n_out, offsets, lens);
}

extern "C" {

int pkt_parse_pcap_host_async(pkt_ctx_t* ctx, const uint8_t* buf, uint64_t len, int entry, const pkt_out_t* out,
                              uint64_t cap) {
    if (!ctx || !buf || !out || !cap) return fail(ctx, PKT_ERR_INVALID_ARG, "null argument");
    if (entry < 0 || entry >= PKT_ENTRY_COUNT) return fail(ctx, PKT_ERR_INVALID_ARG, "bad entry");
    if (cap > kLaunchChunk) return fail(ctx, PKT_ERR_INVALID_ARG, "pkt_parse_pcap_host_async: cap > 2^26 records");
    pkt_out_t dout;
    if (!out_mapped(out, dout))
        return fail(ctx, PKT_ERR_INVALID_ARG, "pkt_parse_pcap_host_async: the columns must be pinned (pkt_host_alloc)");
    int rc = pcap_host_buffers(ctx, len, cap);
    if (rc != PKT_SUCCESS) return rc;
    if (len < 24) return fail(ctx, PKT_ERR_INVALID_ARG, "pcap shorter than its global header");
    // the blocking call's pieces, queued on the ctx's three streams (pkt_parse_pcap_host_result waits)
    return pcap_host_pieces(ctx, buf, len, entry, out, dout, nullptr, nullptr, cap, nullptr);
}

int pkt_parse_pcap_host_result(pkt_ctx_t* ctx, uint64_t* n_out) {
    if (!ctx || !n_out) return fail(ctx, PKT_ERR_INVALID_ARG, "null argument");
    *n_out = 0;
    if (ctx->pc.pending && ctx->hp.init) {  // the copy and export streams of the queued capture
        (void)hipSetDevice(ctx->device);
        const hipError_t e1 = hipStreamSynchronize(ctx->hp.s[1]), e2 = hipStreamSynchronize(ctx->hp.s[2]);
        if (e1 != hipSuccess || e2 != hipSuccess) {
            uint64_t ignored = 0;
            (void)pktgpu_pcap_take(ctx, &ignored);
            return hip_fail(ctx, e1 != hipSuccess ? e1 : e2, "pkt_parse_pcap_host_result");
        }
    }
    return pktgpu_pcap_take(ctx, n_out);
}

int pkt_parse_pcap_host(pkt_ctx_t* ctx, const uint8_t* buf, uint64_t len, int entry, const pkt_out_t* out,
                        uint64_t* offsets, uint32_t* lens, uint64_t cap, uint64_t* n_out) {
    if (!ctx || !buf || !out || !n_out) return fail(ctx, PKT_ERR_INVALID_ARG, "null argument");
    if (entry < 0 || entry >= PKT_ENTRY_COUNT) return fail(ctx, PKT_ERR_INVALID_ARG, "bad entry");
    *n_out = 0;
    hipError_t e;
    int rc = pcap_host_buffers(ctx, len, cap);
    if (rc != PKT_SUCCESS) return rc;
    HostPipe& hp = ctx->hp;
    hipStream_t s = hp.s[0];
    {  // pinned columns: copy, index, parse and export piece by piece (one piece for a short file)
        pkt_out_t dout;
        if (len >= 24 && cap && cap <= kLaunchChunk && out_mapped(out, dout))
            return pcap_host_pieces(ctx, buf, len, entry, out, dout, offsets, lens, cap, n_out);
    }
    // every error return after the first queued copy waits for the ctx's streams first: a copy from
    // `buf` or into `offsets` / `lens` must not outlive the call
    auto bail = [&](int code) {
        (void)hipStreamSynchronize(hp.s[0]);
        (void)hipStreamSynchronize(hp.s[1]);
        return code;
    };
    // in: the whole file, one copy (the record chain is sequential: the index needs all of it)
    if ((e = hipMemcpyAsync(hp.file, buf, len, hipMemcpyHostToDevice, s)) != hipSuccess)
        return bail(hip_fail(ctx, e, "hipMemcpyAsync H2D (pcap file)"));
    uint64_t n = 0;
    rc = pkt_pcap_index_device(ctx, hp.file, len, hp.ioffs, hp.ilens, cap, &n, s);
    if (rc != PKT_SUCCESS) return bail(rc);
    *n_out = n;
    const uint64_t m = std::min(n, cap);
    if (m == 0) return PKT_SUCCESS;
    if (offsets && (e = hipMemcpyAsync(offsets, hp.ioffs, m * 8, hipMemcpyDeviceToHost, hp.s[1])) != hipSuccess)
        return bail(hip_fail(ctx, e, "hipMemcpyAsync D2H (offsets)"));
    if (lens && (e = hipMemcpyAsync(lens, hp.ilens, m * 4, hipMemcpyDeviceToHost, hp.s[1])) != hipSuccess)
        return bail(hip_fail(ctx, e, "hipMemcpyAsync D2H (lens)"));
    const pkt_batch_t db = pcap_host_batch(hp, len, m);
    // out: pinned (mapped) columns are written by the parse kernel over the link directly; else the
    // staged pipeline (device output slots, copies per chunk)
    pkt_out_t dout;
    if (out_mapped(out, dout)) {
        ParseOpts po;
        po.slot_stride = cap;
        rc = pktgpu_parse(ctx, &db, entry, &dout, s, po);
        if (rc != PKT_SUCCESS) return bail(rc);
        for (int k = 0; k < 2; k++)
            if ((e = hipStreamSynchronize(hp.s[k])) != hipSuccess) return hip_fail(ctx, e, "hipStreamSynchronize");
        return PKT_SUCCESS;
    }
    rc = staged_parse(ctx, &db, entry, out, 0, true, cap);
    if (rc != PKT_SUCCESS) return bail(rc);
    if ((e = hipStreamSynchronize(hp.s[1])) != hipSuccess) return hip_fail(ctx, e, "hipStreamSynchronize");
    return PKT_SUCCESS;
}

}  // extern "C"

// ---- a capture that arrives in pieces (pkt_pcap_stream_*, include/pktgpu.h) ----
struct pkt_pcap_stream {
    pkt_ctx_t* ctx = nullptr;  // its own: the open capture holds the ctx's index scratch and host pipeline
    Ingest ig;
    uint64_t max_bytes = 0;
    uint64_t step = 0;  // bytes of new data that start a step at a push
    bool done = false;
    std::string err;
    // Pushes below kStageMax bytes are gathered in a pinned staging ring (host memcpy) and copied in
    // by the slot, so push returns without waiting for a copy (a wait per push is ~20 us: 64 KiB
    // pushes ran at 3.2 GB/s, r06z4; staged 16.6, r06z6); larger pushes are copied from the caller's
    // buffer directly and waited for (195 MB in pushes of 256 KiB: 17.6 ms direct, 8.3 staged; 512 KiB
    // direct 11.2; 1 MiB direct 7.7).  A slot is refilled once its copy has landed (stage_ev).
    static constexpr uint32_t kStageSlots = 4;
    static constexpr uint64_t kStageSlot = 1ull << 20;
    static constexpr uint64_t kStageMax = 1ull << 20;
    uint8_t* stage = nullptr;  // pinned, kStageSlots x kStageSlot
    hipEvent_t stage_ev[kStageSlots] = {};
    bool stage_used[kStageSlots] = {};
    uint32_t cur = 0;   // the slot being filled
    uint64_t fill = 0;  // its bytes
    // The window (include/pktgpu.h): ig is the ingest of the window's bytes, a capture of its own since the
    // last release.  polled / polled_len: the count the last poll / finish returned and the bytes it had
    // indexed (0 before the first and after a release); released_*: what pkt_pcap_stream_release has cut.
    uint64_t polled = 0, polled_len = 0;
    uint64_t released_records = 0, released_bytes = 0;
};

namespace {
constexpr uint64_t kStreamStep = 4ull << 20;
int st_fail(pkt_pcap_stream* st, int code, const std::string& msg) {
    if (st) st->err = msg;
    return code;
}
int st_ctx_fail(pkt_pcap_stream* st, int code) { return st_fail(st, code, st->ctx ? st->ctx->err : "ctx"); }
// The staged bytes of the current slot to the device (in order with every earlier copy: one copy stream).
int st_flush(pkt_pcap_stream* st) {
    if (!st->fill) return PKT_SUCCESS;
    const uint32_t c = st->cur;
    int rc = ingest_copy(st->ig, st->stage + (uint64_t)c * pkt_pcap_stream::kStageSlot, st->fill);
    if (rc != PKT_SUCCESS) return rc;
    const hipError_t e = hipEventRecord(st->stage_ev[c], st->ctx->hp.s[1]);
    if (e != hipSuccess) return ingest_fail(st->ig, hip_fail(st->ctx, e, "hipEventRecord (staging)"));
    st->stage_used[c] = true;
    st->cur = (c + 1) % pkt_pcap_stream::kStageSlots;
    st->fill = 0;
    return PKT_SUCCESS;
}
// poll / finish after their last step: wait, and remember what the window's index now holds.
int st_wait(pkt_pcap_stream* st, uint64_t* n_records, uint64_t* offsets, uint32_t* lens) {
    const int rc = ingest_wait(st->ig, n_records, offsets, lens);
    if (rc == PKT_SUCCESS) {
        st->polled = *n_records;
        st->polled_len = st->ig.indexed;
    }
    return rc;
}
// Move hp.file[p, hi) down to hp.file + 24 on the copy stream (the streams are idle).  The ranges overlap
// when the kept bytes outnumber the freed ones: forward chunks of at most p - 24 bytes are each disjoint
// from their destination and never overwrite bytes a later chunk reads; past kMoveChunks of them, once
// through a temporary buffer (*tmp, freed by the caller after the stream has drained).
constexpr uint64_t kMoveChunks = 64;
hipError_t st_move_down(HostPipe& hp, uint64_t p, uint64_t hi, void** tmp) {
    const uint64_t kept = hi - p, d = p - 24;
    if (!kept || !d) return hipSuccess;
    hipStream_t s = hp.s[1];
    if ((kept + d - 1) / d > kMoveChunks) {
        hipError_t e = hipMalloc(tmp, kept);
        if (e == hipSuccess) e = hipMemcpyAsync(*tmp, hp.file + p, kept, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(hp.file + 24, *tmp, kept, hipMemcpyDeviceToDevice, s);
        return e;
    }
    for (uint64_t o = 0; o < kept; o += d) {
        const hipError_t e = hipMemcpyAsync(hp.file + 24 + o, hp.file + p + o, std::min(d, kept - o), hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
}  // namespace

extern "C" {

int pkt_pcap_stream_open(int device, uint64_t max_bytes, uint64_t cap, int entry, const pkt_out_t* out,
                         uint64_t step_bytes, pkt_pcap_stream_t** out_st) {
    if (!out_st || !out || !cap || max_bytes < 24) return PKT_ERR_INVALID_ARG;
    *out_st = nullptr;
    if (entry < 0 || entry >= PKT_ENTRY_COUNT || cap > kLaunchChunk) return PKT_ERR_INVALID_ARG;
    pkt_out_t dout;
    const bool pinned = out_mapped(out, dout);
    if (!pinned) {  // then every requested column is device memory (none mapped host memory)
        const uint8_t* const* oc = reinterpret_cast<const uint8_t* const*>(out);
        for (int c = 0; c < kNumCols; c++) {
            const uint8_t* unused = nullptr;
            if (oc[c] && host_mapped(oc[c], unused)) return PKT_ERR_INVALID_ARG;  // mixed host / device columns
        }
    }
    pkt_pcap_stream* st = new pkt_pcap_stream();
    int rc = pkt_ctx_create(device, &st->ctx);
    if (rc == PKT_SUCCESS) rc = ingest_begin(st->ig, st->ctx, max_bytes, cap, entry, out, pinned ? &dout : nullptr);
    if (rc != PKT_SUCCESS) {
        pkt_pcap_stream_close(st);
        return rc;
    }
    st->max_bytes = max_bytes;
    st->step = step_bytes ? step_bytes : kStreamStep;
    hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&st->stage), pkt_pcap_stream::kStageSlots * pkt_pcap_stream::kStageSlot, 0);
    for (uint32_t k = 0; k < pkt_pcap_stream::kStageSlots && e == hipSuccess; k++)
        e = hipEventCreateWithFlags(&st->stage_ev[k], hipEventDisableTiming);
    if (e != hipSuccess) {
        rc = hip_fail(st->ctx, e, "pinned staging ring");
        pkt_pcap_stream_close(st);
        return rc;
    }
    *out_st = st;
    return PKT_SUCCESS;
}

int pkt_pcap_stream_push(pkt_pcap_stream_t* st, const uint8_t* bytes, uint64_t n) {
    if (!st || (n && !bytes)) return st_fail(st, PKT_ERR_INVALID_ARG, "null argument");
    if (st->done) return st_fail(st, PKT_ERR_INVALID_ARG, "the capture is finished");
    if (n > st->max_bytes - st->ig.hi - st->fill) return st_fail(st, PKT_ERR_INVALID_ARG, "push past the capture's max_bytes");
    if (!n) return PKT_SUCCESS;
    if (st->ig.rc != PKT_SUCCESS) return st_ctx_fail(st, st->ig.rc);
    int rc = PKT_SUCCESS;
    // the caller may reuse its buffer once this returns: its bytes are staged, or their copy has landed
    if (n < pkt_pcap_stream::kStageMax) {
        while (n && rc == PKT_SUCCESS) {
            const uint32_t c = st->cur;
            if (!st->fill && st->stage_used[c]) {  // the slot's previous copy must have landed
                const hipError_t e = hipEventSynchronize(st->stage_ev[c]);
                if (e != hipSuccess) rc = ingest_fail(st->ig, hip_fail(st->ctx, e, "hipEventSynchronize (staging)"));
                st->stage_used[c] = false;
            }
            const uint64_t take = std::min(n, pkt_pcap_stream::kStageSlot - st->fill);
            if (rc == PKT_SUCCESS) std::memcpy(st->stage + (uint64_t)c * pkt_pcap_stream::kStageSlot + st->fill, bytes, take);
            st->fill += take;
            bytes += take;
            n -= take;
            if (rc == PKT_SUCCESS && st->fill == pkt_pcap_stream::kStageSlot) rc = st_flush(st);
        }
        // a step is due: its bytes go now (steps run over copied bytes)
        const uint64_t have = st->ig.hi + st->fill;
        if (rc == PKT_SUCCESS && have >= 24 && have - st->ig.indexed >= st->step) rc = st_flush(st);
    } else {
        rc = st_flush(st);  // the staged bytes first: the file's order
        if (rc == PKT_SUCCESS) rc = ingest_copy(st->ig, bytes, n);
        const hipEvent_t landed = rc == PKT_SUCCESS ? ingest_copied(st->ig, st->ig.hi) : nullptr;
        const hipError_t e = landed ? hipEventSynchronize(landed) : hipSuccess;
        if (e != hipSuccess) rc = ingest_fail(st->ig, hip_fail(st->ctx, e, "hipEventSynchronize (push)"));
    }
    if (rc == PKT_SUCCESS && st->ig.hi >= 24 && st->ig.hi - st->ig.indexed >= st->step) rc = ingest_step(st->ig, false);
    return rc == PKT_SUCCESS ? rc : st_ctx_fail(st, rc);
}

int pkt_pcap_stream_poll(pkt_pcap_stream_t* st, uint64_t* n_records, uint64_t* offsets, uint32_t* lens) {
    if (!st || !n_records) return st_fail(st, PKT_ERR_INVALID_ARG, "null argument");
    *n_records = 0;
    int rc = st->done ? PKT_SUCCESS : st_flush(st);
    if (rc != PKT_SUCCESS) return st_ctx_fail(st, rc);
    if (st->ig.hi < 24) return st->ig.rc;  // not even the global header yet
    if (!st->done && st->ig.hi > st->ig.indexed) rc = ingest_step(st->ig, false);
    if (rc == PKT_SUCCESS) rc = st_wait(st, n_records, offsets, lens);
    return rc == PKT_SUCCESS ? rc : st_ctx_fail(st, rc);
}

int pkt_pcap_stream_finish(pkt_pcap_stream_t* st, uint64_t* n_records, uint64_t* offsets, uint32_t* lens) {
    if (!st || !n_records) return st_fail(st, PKT_ERR_INVALID_ARG, "null argument");
    *n_records = 0;
    int rc = st->done ? PKT_SUCCESS : st_flush(st);
    if (rc != PKT_SUCCESS) return st_ctx_fail(st, rc);
    if (st->ig.hi < 24) return st_fail(st, PKT_ERR_INVALID_ARG, "pcap shorter than its global header");
    if (!st->done) rc = ingest_step(st->ig, true);  // the tail as pkt_pcap_index takes it (errors included)
    st->done = true;
    if (rc == PKT_SUCCESS) rc = st_wait(st, n_records, offsets, lens);
    return rc == PKT_SUCCESS ? rc : st_ctx_fail(st, rc);
}

// A release restarts the ingest on the kept bytes: they move down to offset 24 and the window becomes a
// fresh capture of 24 + kept bytes already copied, whose first step (no carry-in) indexes and parses the kept
// records again.  The cost is proportional to the kept bytes — one partial record for a consumer that
// releases what it polled.
int pkt_pcap_stream_release(pkt_pcap_stream_t* st, uint64_t n_records) {
    if (!st) return PKT_ERR_INVALID_ARG;
    if (st->done) return st_fail(st, PKT_ERR_INVALID_ARG, "release after finish");
    if (n_records > std::min(st->polled, st->ig.cap))
        return st_fail(st, PKT_ERR_INVALID_ARG, "release of more records than the last poll's columns hold");
    Ingest& ig = st->ig;
    if (ig.rc != PKT_SUCCESS) return st_ctx_fail(st, ig.rc);
    if (!n_records) return PKT_SUCCESS;  // p = 24: the window stays as it is
    pkt_ctx_t* ctx = st->ctx;
    HostPipe& hp = ctx->hp;
    int rc = st_flush(st);  // the staged bytes follow the kept ones
    if (rc != PKT_SUCCESS) return st_ctx_fail(st, rc);
    hipError_t e = hipSuccess;
    for (int k = 0; k < HostPipe::kSlots && e == hipSuccess; k++) e = hipStreamSynchronize(hp.s[k]);
    // the cut: the end of window record n - 1
    uint64_t off = 0;
    uint32_t len = 0;
    if (e == hipSuccess) e = hipMemcpy(&off, hp.ioffs + (n_records - 1), 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(&len, hp.ilens + (n_records - 1), 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return st_ctx_fail(st, ingest_fail(ig, hip_fail(ctx, e, "pkt_pcap_stream_release (cut)")));
    const uint64_t p = off + len, hi = ig.hi;
    if (p < 24 + 16 || p > st->polled_len || p > hi)  // (the index of a counted record: never)
        return st_ctx_fail(st, ingest_fail(ig, fail(ctx, PKT_ERR_INVALID_ARG, "pkt_pcap_stream_release: bad cut")));
    void* tmp = nullptr;
    e = st_move_down(hp, p, hi, &tmp);
    // the window as a fresh capture whose 24 + kept bytes are one landed copy
    if (e == hipSuccess) e = hipEventRecord(hp.ev_copy[0], hp.s[1]);
    if (e == hipSuccess) e = hipStreamSynchronize(hp.s[1]);
    if (tmp) (void)hipFree(tmp);
    if (e != hipSuccess) return st_ctx_fail(st, ingest_fail(ig, hip_fail(ctx, e, "pkt_pcap_stream_release (move)")));
    ig.hi = 24 + (hi - p);
    ig.indexed = 0;
    ig.steps = 0;
    ig.copies = 1;
    ig.copy_end[0] = ig.hi;
    st->released_records += n_records;
    st->released_bytes += p - 24;
    st->polled = st->polled_len = 0;
    return PKT_SUCCESS;
}

int pkt_pcap_stream_room(const pkt_pcap_stream_t* st, uint64_t* bytes) {
    if (!st || !bytes) return PKT_ERR_INVALID_ARG;
    *bytes = st->max_bytes - st->ig.hi - st->fill;
    return PKT_SUCCESS;
}

int pkt_pcap_stream_released(const pkt_pcap_stream_t* st, uint64_t* records, uint64_t* bytes) {
    if (!st) return PKT_ERR_INVALID_ARG;
    if (records) *records = st->released_records;
    if (bytes) *bytes = st->released_bytes;
    return PKT_SUCCESS;
}

int pkt_pcap_stream_batch(pkt_pcap_stream_t* st, pkt_batch_t* batch) {
    if (!st || !batch) return PKT_ERR_INVALID_ARG;
    *batch = pcap_host_batch(st->ctx->hp, st->polled_len, std::min(st->polled, st->ig.cap));
    return PKT_SUCCESS;
}

pkt_ctx_t* pkt_pcap_stream_ctx(pkt_pcap_stream_t* st) { return st ? st->ctx : nullptr; }

const char* pkt_pcap_stream_last_error(const pkt_pcap_stream_t* st) { return st ? st->err.c_str() : "null stream"; }

int pkt_pcap_stream_close(pkt_pcap_stream_t* st) {
    if (!st) return PKT_SUCCESS;
    if (st->ctx) pkt_ctx_destroy(st->ctx);  // waits for its streams (the staging ring's copies too)
    for (hipEvent_t ev : st->stage_ev)
        if (ev) (void)hipEventDestroy(ev);
    if (st->stage) (void)hipHostFree(st->stage);
    delete st;
    return PKT_SUCCESS;
}

}  // extern "C"
