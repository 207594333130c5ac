// pktgpu_pcapw.hip — pkt_pcap_write: the selected packets of a batch as one capture in device
// memory (tests/pcap.rs:7-37 as a batch operation), in four launches with no waiting between blocks:
//   pw_reduce_kernel  per tile of 1024 packets, the bytes (16 + incl_len per selected packet) and the
//                     count of the records it contributes;
//   pw_scan_kernel    one block: the exclusive prefix of the tile sums (the file starts at 24, after
//                     the global header), the two totals to a device word pair and to the ctx's pinned
//                     words, i.e. total > dst_len is known on the device before anything is written;
//   pw_emit_kernel    per tile again: each selected packet's record position — rec_offsets / rec_lens /
//                     src_index, and first[w] = the record holding byte 4096 w of the file for every
//                     4 KiB window start the record covers (at most 17: a record is <= 65551 bytes);
//   pw_copy_kernel    one wave per aligned 4 KiB window of dst: the records of the window staged in LDS
//                     (their position, source, lengths and time), a 256-bit map of the record starts,
//                     then every 16-byte chunk built in registers — the tail of a record's header or
//                     data, the head of the next record's header, the global header in chunks 0 and 1 —
//                     and stored whole; only the file's last chunk may be partial.
// Every record is at least 16 bytes, so a chunk holds bytes of at most two records and at most one
// record starts in it.  dst is never read; emit and copy exit when the total exceeds dst_len.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "pktgpu_ctx.hpp"

namespace {

constexpr uint32_t kPwBlock = 256;
constexpr uint32_t kPwPer = 4;                    // consecutive packets per thread
constexpr uint32_t kPwTile = kPwBlock * kPwPer;   // packets per block of reduce / emit
constexpr uint32_t kPwScanPer = 16;               // tile sums per thread and round of the scan
constexpr uint32_t kPwWin = 4096;                 // destination bytes per wave of the copy
constexpr uint32_t kPwWaves = kPwBlock / 64;
// records a window can hold: the one holding its first byte, then starts >= 16 bytes apart
constexpr uint32_t kPwRec = kPwWin / 16 + 1;
constexpr uint32_t kPwSlots = 264;
static_assert(kPwSlots >= kPwRec, "LDS slots per wave");

struct WSrc {
    BatchSrc b;
    const uint8_t* select;
    const uint32_t* ts_sec;
    const uint32_t* ts_usec;
    uint32_t snaplen, tv_sec, tv_usec;
    uint64_t n;  // < 2^32
};

__device__ __forceinline__ uint32_t w_incl(const WSrc& a, uint32_t len) {
    return a.snaplen && len > a.snaplen ? a.snaplen : len;
}

// packet i's record bytes (low half) and record count (high half); 0 when not selected
__device__ __forceinline__ uint64_t w_contrib(const WSrc& a, uint64_t i) {
    if (i >= a.n || (a.select && !a.select[i])) return 0;
    return (uint64_t)(16u + w_incl(a, pkt_len(a.b, i, pkt_off(a.b, i)))) | 1ull << 32;
}

// a tile's sums: at most 1024 * 65551 bytes and 1024 records, so both halves of the packed word hold
__global__ __launch_bounds__(kPwBlock) void pw_reduce_kernel(WSrc a, uint64_t* __restrict__ blk_bytes,
                                                             uint32_t* __restrict__ blk_cnt) {
    __shared__ uint64_t s_w[kPwWaves];
    const uint64_t i0 = (uint64_t)blockIdx.x * kPwTile + threadIdx.x * kPwPer;
    uint64_t v = 0;
#pragma unroll
    for (uint32_t j = 0; j < kPwPer; j++) v += w_contrib(a, i0 + j);
    uint64_t total;
    (void)block_excl_scan<kPwWaves>(v, s_w, total);
    if (threadIdx.x == 0) {
        blk_bytes[blockIdx.x] = total & 0xFFFFFFFFull;
        blk_cnt[blockIdx.x] = (uint32_t)(total >> 32);
    }
}

// tot: [total bytes, records] on the device; host: the same two words in pinned memory
__global__ __launch_bounds__(kPwBlock) void pw_scan_kernel(uint64_t* __restrict__ blk_bytes, uint32_t* __restrict__ blk_cnt,
                                                           uint32_t nb, uint64_t* __restrict__ tot,
                                                           uint64_t* __restrict__ host) {
    __shared__ uint64_t s_w[kPwWaves];
    uint64_t cb = 24, cc = 0;  // the global header comes first
    for (uint64_t base = 0; base < nb; base += (uint64_t)kPwBlock * kPwScanPer) {
        const uint64_t i0 = base + (uint64_t)threadIdx.x * kPwScanPer;
        uint64_t b[kPwScanPer], sb = 0, sc = 0;
        uint32_t c[kPwScanPer];
#pragma unroll
        for (uint32_t j = 0; j < kPwScanPer; j++) {
            const bool in = i0 + j < nb;
            b[j] = in ? blk_bytes[i0 + j] : 0;
            c[j] = in ? blk_cnt[i0 + j] : 0;
            sb += b[j];
            sc += c[j];
        }
        uint64_t tb, tc;
        uint64_t eb = cb + block_excl_scan<kPwWaves>(sb, s_w, tb);
        uint64_t ec = cc + block_excl_scan<kPwWaves>(sc, s_w, tc);
#pragma unroll
        for (uint32_t j = 0; j < kPwScanPer; j++) {
            if (i0 + j < nb) {
                blk_bytes[i0 + j] = eb;
                blk_cnt[i0 + j] = (uint32_t)ec;  // records before a tile: < n < 2^32
            }
            eb += b[j];
            ec += c[j];
        }
        cb += tb;
        cc += tc;
    }
    if (threadIdx.x == 0) {
        tot[0] = cb;
        tot[1] = cc;
        host[0] = cb;
        host[1] = cc;
    }
}

__global__ __launch_bounds__(kPwBlock) void pw_emit_kernel(WSrc a, const uint64_t* __restrict__ blk_bytes,
                                                           const uint32_t* __restrict__ blk_cnt,
                                                           const uint64_t* __restrict__ tot, uint64_t dst_len,
                                                           uint64_t* __restrict__ k_off, uint32_t* __restrict__ rec_lens,
                                                           uint32_t* __restrict__ k_src, uint32_t* __restrict__ first,
                                                           uint64_t nwin) {
    __shared__ uint64_t s_w[kPwWaves];
    if (tot[0] > dst_len) return;  // (uniform) the capture does not fit: nothing is written
    const uint64_t i0 = (uint64_t)blockIdx.x * kPwTile + threadIdx.x * kPwPer;
    uint64_t c[kPwPer], v = 0;
#pragma unroll
    for (uint32_t j = 0; j < kPwPer; j++) {
        c[j] = w_contrib(a, i0 + j);
        v += c[j];
    }
    uint64_t total;
    const uint64_t ex = block_excl_scan<kPwWaves>(v, s_w, total);
    const uint64_t kbase = blk_cnt[blockIdx.x];
    uint64_t pos = blk_bytes[blockIdx.x] + (ex & 0xFFFFFFFFull);
    uint32_t lk = (uint32_t)(ex >> 32);  // the record's place among the tile's
    // the tile's records go to LDS in record order and out by consecutive lanes: whole lines of the
    // three columns, not four 8-byte stores per thread 32 bytes apart
    __shared__ uint64_t s_off[kPwTile];
    __shared__ uint32_t s_len[kPwTile], s_src[kPwTile];
#pragma unroll
    for (uint32_t j = 0; j < kPwPer; j++) {
        if (!c[j]) continue;
        const uint32_t rb = (uint32_t)c[j];  // 16 + incl_len
        s_off[lk] = pos + 16;
        s_len[lk] = rb - 16u;
        s_src[lk] = (uint32_t)(i0 + j);
        // the window starts inside [pos, pos + rb)
        const uint64_t w0 = (pos + kPwWin - 1) / kPwWin, w1 = (pos + rb + kPwWin - 1) / kPwWin;
        for (uint64_t w = w0; w < w1 && w < nwin; w++) first[w] = (uint32_t)(kbase + lk);
        pos += rb;
        lk++;
    }
    __syncthreads();
    const uint32_t cnt = (uint32_t)(total >> 32);  // <= kPwTile
    for (uint32_t x = threadIdx.x; x < cnt; x += kPwBlock) {
        k_off[kbase + x] = s_off[x];
        if (rec_lens) rec_lens[kbase + x] = s_len[x];
        k_src[kbase + x] = s_src[x];
    }
}

__global__ __launch_bounds__(kPwBlock) void pw_copy_kernel(WSrc a, const uint64_t* __restrict__ tot, uint64_t dst_len,
                                                           const uint64_t* __restrict__ k_off,
                                                           const uint32_t* __restrict__ k_src,
                                                           const uint32_t* __restrict__ first, uint8_t* __restrict__ dst) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t w = (uint64_t)blockIdx.x * kPwWaves + wv;
    const uint64_t total = tot[0], nout = tot[1];
    if (total > dst_len) return;  // the capture does not fit: the host reports the size needed
    const uint64_t wa = w * kPwWin, we = wa + kPwWin;
    if (wa >= total) return;
    // slot r = record kb + r: where its header starts relative to the window, its source, incl_len |
    // orig_len << 16 and its time.  Slot 0 holds the window's first byte (for window 0 that is the
    // global header: a slot with nothing to give); later slots start inside the window.
    __shared__ int32_t s_rel[kPwWaves][kPwSlots];
    __shared__ uint64_t s_src[kPwWaves][kPwSlots];
    __shared__ uint32_t s_len[kPwWaves][kPwSlots];
    __shared__ uint32_t s_sec[kPwWaves][kPwSlots];
    __shared__ uint32_t s_usec[kPwWaves][kPwSlots];
    __shared__ uint32_t s_map[kPwWaves][kPwWin / 16 / 32];
    const int64_t kb = w == 0 ? -1 : (int64_t)first[w];
    if (lane < kPwWin / 16 / 32) s_map[wv][lane] = 0;
    wave_sync();
    for (uint32_t b = 0; b * 64u < kPwSlots; b++) {  // uniform
        const uint32_t r = 64u * b + lane;
        const int64_t k = kb + (int64_t)r;
        bool in = false;
        int32_t rel = -32;
        uint64_t src = 0;
        uint32_t len = 0, sec = 0, usec = 0;
        if (k < 0) {
            in = true;
        } else if ((uint64_t)k < nout && r < kPwSlots) {
            const uint64_t h = k_off[k] - 16;
            const uint64_t i = k_src[k];
            if (h < we) {
                in = true;
                src = pkt_off(a.b, i);
                const uint32_t orig = pkt_len(a.b, i, src);
                len = w_incl(a, orig) | orig << 16;
                sec = a.ts_sec ? a.ts_sec[i] : a.tv_sec;
                usec = a.ts_usec ? a.ts_usec[i] : a.tv_usec;
                rel = (int32_t)((int64_t)h - (int64_t)wa);
            }
        }
        if (in) {
            s_rel[wv][r] = rel;
            s_src[wv][r] = src;
            s_len[wv][r] = len;
            s_sec[wv][r] = sec;
            s_usec[wv][r] = usec;
            if (r > 0 && rel > 0 && rel < (int32_t)kPwWin) {  // starts in chunk rel / 16
                const uint32_t g = (uint32_t)rel >> 4;
                atomicOr(&s_map[wv][g >> 5], 1u << (g & 31u));
            }
        }
        if (!((__ballot(in) >> 63) & 1ull)) break;  // a record past the window (or the last one) was seen
    }
    wave_sync();
    const uint64_t last16 = a.b.slab_len ? ((a.b.slab_len + 15) & ~(uint64_t)15) - 16 : 0;
    constexpr uint32_t kQ = kPwWin / 16 / 64;  // chunks per lane
    Le128 o[kQ];
    uint4 v0[kQ], v1[kQ];
    uint32_t dsh[kQ], dlo[kQ], dhi[kQ];
    uint32_t run = 0;
    // the window's source loads go first, all in flight before the first store
#pragma unroll
    for (uint32_t q = 0; q < kQ; q++) {
        const uint32_t g = 64u * q + lane;
        const uint64_t ca = wa + 16u * g;
        const uint64_t word = (uint64_t)s_map[wv][2 * q] | (uint64_t)s_map[wv][2 * q + 1] << 32;
        const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(word >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)word, 0u));
        const uint32_t P = run + below;  // the last record starting before the chunk
        const bool bit = (word >> lane) & 1ull;
        run += (uint32_t)__builtin_popcountll(word);
        o[q] = Le128{0, 0};
        dlo[q] = dhi[q] = dsh[q] = 0;
        v0[q] = v1[q] = make_uint4(0, 0, 0, 0);
        if (ca >= total) continue;
        if (ca < 24) o[q] = ca == 0 ? Le128{0x00040002A1B2C3D4ull, 0} : Le128{0x000000010000FFFFull, 0};
        const int32_t relP = s_rel[wv][P] - (int32_t)(16u * g);  // its header's start, from the chunk's
        const uint32_t lenP = s_len[wv][P], inclP = lenP & 0xFFFFu;
        if (relP > -16) {  // the tail of its header
            const Le128 h = bytes_down(Le128{(uint64_t)s_sec[wv][P] | (uint64_t)s_usec[wv][P] << 32,
                                           (uint64_t)inclP | (uint64_t)(lenP >> 16) << 32},
                                      (uint32_t)(-relP));
            o[q].lo |= h.lo, o[q].hi |= h.hi;
        }
        if (bit) {  // the head of the next record's header
            const uint32_t lenQ = s_len[wv][P + 1];
            const int32_t relQ = s_rel[wv][P + 1] - (int32_t)(16u * g);
            const Le128 h = bytes_up(Le128{(uint64_t)s_sec[wv][P + 1] | (uint64_t)s_usec[wv][P + 1] << 32,
                                         (uint64_t)(lenQ & 0xFFFFu) | (uint64_t)(lenQ >> 16) << 32},
                                    (uint32_t)relQ & 15u);
            o[q].lo |= h.lo, o[q].hi |= h.hi;
        }
        // its data: the chunk's bytes [lo, hi)
        const int32_t d0 = relP + 16, d1 = d0 + (int32_t)inclP;
        const int32_t lo = d0 < 0 ? 0 : d0, hi = d1 > 16 ? 16 : d1;
        if (lo < hi) {
            dlo[q] = (uint32_t)lo, dhi[q] = (uint32_t)hi;
            // the source of the chunk's byte 0 (before the packet, even before the slab, when the
            // data starts inside the chunk: those bytes are masked off)
            const int64_t B = (int64_t)s_src[wv][P] - d0;
            const int64_t A = B & ~(int64_t)15;
            dsh[q] = (uint32_t)(B - A);
            const int64_t a0 = A < 0 ? 0 : A, a1 = A + 16;
            v0[q] = *reinterpret_cast<const uint4*>(a.b.slab + ((uint64_t)a0 > last16 ? last16 : (uint64_t)a0));
            v1[q] = *reinterpret_cast<const uint4*>(a.b.slab + ((uint64_t)a1 > last16 ? last16 : (uint64_t)a1));
        }
    }
#pragma unroll
    for (uint32_t q = 0; q < kQ; q++) {
        const uint64_t ca = wa + 16u * (64u * q + lane);
        if (ca >= total) continue;
        if (dlo[q] < dhi[q]) {
            const uint64_t x0 = (uint64_t)v0[q].x | (uint64_t)v0[q].y << 32, x1 = (uint64_t)v0[q].z | (uint64_t)v0[q].w << 32;
            const uint64_t x2 = (uint64_t)v1[q].x | (uint64_t)v1[q].y << 32, x3 = (uint64_t)v1[q].z | (uint64_t)v1[q].w << 32;
            const bool up = dsh[q] >= 8;
            const uint64_t y0 = up ? x1 : x0, y1 = up ? x2 : x1, y2 = up ? x3 : x2;
            const uint32_t s = 8u * (dsh[q] & 7u);
            const uint64_t lo = s ? y0 >> s | y1 << (64u - s) : y0, hi = s ? y1 >> s | y2 << (64u - s) : y1;
            const Le128 m1 = bytes_below(dhi[q]), m0 = bytes_below(dlo[q]);
            o[q].lo |= lo & m1.lo & ~m0.lo;
            o[q].hi |= hi & m1.hi & ~m0.hi;
        }
        const uint32_t d[4] = {(uint32_t)o[q].lo, (uint32_t)(o[q].lo >> 32), (uint32_t)o[q].hi, (uint32_t)(o[q].hi >> 32)};
        if (ca + 16 <= total) {
            *reinterpret_cast<uint4*>(dst + ca) = make_uint4(d[0], d[1], d[2], d[3]);
        } else {  // the file's last chunk: whole dwords, then a short, then a byte
            const uint32_t nbytes = (uint32_t)(total - ca);
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) {
                if (4 * j + 4 <= nbytes) {
                    *reinterpret_cast<uint32_t*>(dst + ca + 4 * j) = d[j];
                } else if (4 * j < nbytes) {
                    const uint32_t m = nbytes - 4 * j;  // 1..3
                    if (m & 2) *reinterpret_cast<uint16_t*>(dst + ca + 4 * j) = (uint16_t)d[j];
                    if (m & 1) dst[ca + 4 * j + (m & 2)] = (uint8_t)(d[j] >> (8 * (m & 2)));
                }
            }
        }
    }
}

// The four launches, queued on s.  The totals arrive in ctx->pw.ctl once the stream has passed them.
int pw_queue(pkt_ctx_t* ctx, const pkt_batch_t* b, const uint8_t* select, uint32_t snaplen, uint32_t tv_sec,
             uint32_t tv_usec, const uint32_t* ts_sec, const uint32_t* ts_usec, uint8_t* dst, uint64_t dst_len,
             uint64_t* rec_offsets, uint32_t* rec_lens, uint32_t* src_index, hipStream_t s) {
    if (!ctx || !b) return fail(ctx, PKT_ERR_INVALID_ARG, "null argument");
    if (b->n >= (1ull << 32)) return fail(ctx, PKT_ERR_INVALID_ARG, "pkt_pcap_write: n >= 2^32");
    if (dst_len && !dst) return fail(ctx, PKT_ERR_INVALID_ARG, "null dst");
    if ((uintptr_t)dst & 15) return fail(ctx, PKT_ERR_INVALID_ARG, "dst not 16-byte aligned");
    if (b->n) {
        int rc = check_batch_slab16(ctx, b);
        if (rc == PKT_SUCCESS) rc = check_batch_index(ctx, b);
        if (rc != PKT_SUCCESS) return rc;
    }
    PcapWriteScratch& pw = ctx->pw;
    if (pw.pending)
        return fail(ctx, PKT_ERR_INVALID_ARG, "a queued write's result has not been taken on this ctx (pkt_pcap_write_result)");
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    const uint64_t n = b->n;
    const uint32_t nb = (uint32_t)((n + kPwTile - 1) / kPwTile);
    // the windows the capture can reach: bounded by dst_len and by the longest record n packets can give
    uint64_t maxlen = b->lens ? 65535u : std::min<uint64_t>(b->stride, 65535u);
    if (snaplen) maxlen = std::min<uint64_t>(maxlen, snaplen);
    const uint64_t bound = std::min(dst_len, 24 + n * (16 + maxlen));
    const uint64_t nwin = (bound + kPwWin - 1) / kPwWin;
    if (nwin > (1ull << 32)) return fail(ctx, PKT_ERR_INVALID_ARG, "pkt_pcap_write: capture too large");
    // scratch: the two totals, the tile sums, the window table, and the record table's columns the
    // caller did not ask for
    const uint64_t o_bytes = 64, o_cnt = o_bytes + round16(8ull * nb), o_first = o_cnt + round16(4ull * nb);
    const uint64_t o_koff = o_first + round16(4 * nwin), o_ksrc = o_koff + (rec_offsets ? 0 : round16(8 * n));
    const uint64_t need = o_ksrc + (src_index ? 0 : round16(4 * n));
    if ((e = pw.reserve(need)) != hipSuccess) return hip_fail(ctx, e, "hipMalloc (pcap write)");
    if ((e = pw.ensure(64)) != hipSuccess) return hip_fail(ctx, e, "hipHostMalloc (pcap write)");
    char* p = static_cast<char*>(pw.buf);
    uint64_t* tot = reinterpret_cast<uint64_t*>(p);
    uint64_t* blk_bytes = reinterpret_cast<uint64_t*>(p + o_bytes);
    uint32_t* blk_cnt = reinterpret_cast<uint32_t*>(p + o_cnt);
    uint32_t* first = reinterpret_cast<uint32_t*>(p + o_first);
    uint64_t* k_off = rec_offsets ? rec_offsets : reinterpret_cast<uint64_t*>(p + o_koff);
    uint32_t* k_src = src_index ? src_index : reinterpret_cast<uint32_t*>(p + o_ksrc);
    WSrc a;
    a.b = batch_src(b);
    a.select = select;
    a.ts_sec = ts_sec;
    a.ts_usec = ts_usec;
    a.snaplen = snaplen;
    a.tv_sec = tv_sec;
    a.tv_usec = tv_usec;
    a.n = n;
    pw.ctl[0] = pw.ctl[1] = 0;
    pw.dst_len = dst_len;
    if (nb) hipLaunchKernelGGL(pw_reduce_kernel, dim3(nb), dim3(kPwBlock), 0, s, a, blk_bytes, blk_cnt);
    hipLaunchKernelGGL(pw_scan_kernel, dim3(1), dim3(kPwBlock), 0, s, blk_bytes, blk_cnt, nb, tot, pw.ctl_dev);
    if (nb && nwin)
        hipLaunchKernelGGL(pw_emit_kernel, dim3(nb), dim3(kPwBlock), 0, s, a, blk_bytes, blk_cnt, tot, dst_len, k_off,
                           rec_lens, k_src, first, nwin);
    if (nwin)
        hipLaunchKernelGGL(pw_copy_kernel, dim3((unsigned)((nwin + kPwWaves - 1) / kPwWaves)), dim3(kPwBlock), 0, s, a,
                           tot, dst_len, k_off, k_src, first, dst);
    if ((e = hipGetLastError()) != hipSuccess) return hip_fail(ctx, e, "pcap write launch");
    return PKT_SUCCESS;
}

// The outcome of the last pw_queue (the stream has passed it).
int pw_finish(pkt_ctx_t* ctx, uint64_t* bytes_out, uint64_t* n_out) {
    const PcapWriteScratch& pw = ctx->pw;
    if (bytes_out) *bytes_out = pw.ctl[0];
    if (n_out) *n_out = pw.ctl[1];
    if (pw.ctl[0] > pw.dst_len) return fail(ctx, PKT_ERR_INVALID_ARG, "pkt_pcap_write: the capture is larger than dst_len");
    return PKT_SUCCESS;
}

}  // namespace

extern "C" {

int pkt_pcap_write(pkt_ctx_t* ctx, const pkt_batch_t* batch, const uint8_t* select, uint32_t snaplen, uint32_t tv_sec,
                   uint32_t tv_usec, const uint32_t* ts_sec, const uint32_t* ts_usec, uint8_t* dst, uint64_t dst_len,
                   uint64_t* rec_offsets, uint32_t* rec_lens, uint32_t* src_index, uint64_t* bytes_out, uint64_t* n_out,
                   void* stream) {
    if (bytes_out) *bytes_out = 0;
    if (n_out) *n_out = 0;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int rc = pw_queue(ctx, batch, select, snaplen, tv_sec, tv_usec, ts_sec, ts_usec, dst, dst_len, rec_offsets,
                            rec_lens, src_index, s);
    if (rc != PKT_SUCCESS) return rc;
    const hipError_t e = hipStreamSynchronize(s);  // the one host wait, for the two totals
    if (e != hipSuccess) return hip_fail(ctx, e, "pkt_pcap_write");
    return pw_finish(ctx, bytes_out, n_out);
}

int pkt_pcap_write_async(pkt_ctx_t* ctx, const pkt_batch_t* batch, const uint8_t* select, uint32_t snaplen,
                         uint32_t tv_sec, uint32_t tv_usec, const uint32_t* ts_sec, const uint32_t* ts_usec, uint8_t* dst,
                         uint64_t dst_len, uint64_t* rec_offsets, uint32_t* rec_lens, uint32_t* src_index, void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int rc = pw_queue(ctx, batch, select, snaplen, tv_sec, tv_usec, ts_sec, ts_usec, dst, dst_len, rec_offsets,
                            rec_lens, src_index, s);
    if (rc != PKT_SUCCESS) return rc;
    ctx->pw.mark(s);
    return PKT_SUCCESS;
}

int pkt_pcap_write_result(pkt_ctx_t* ctx, uint64_t* bytes_out, uint64_t* n_out) {
    if (bytes_out) *bytes_out = 0;
    if (n_out) *n_out = 0;
    if (!ctx) return PKT_ERR_INVALID_ARG;
    PcapWriteScratch& pw = ctx->pw;
    if (!pw.pending) return fail(ctx, PKT_ERR_INVALID_ARG, "no write queued on this ctx");
    const hipError_t e = pw.take();
    if (e != hipSuccess) return hip_fail(ctx, e, "pkt_pcap_write_result");
    return pw_finish(ctx, bytes_out, n_out);
}

}  // extern "C"
