// pktgpu_frag.hip — pkt_frag_batch / _async / _result: IPv4 fragmentation of a batch to a per-packet MTU, one source
// packet to one or several output packets packed at 16-byte-aligned offsets of a second slab, in four launches with
// no waiting between blocks (pktgpu_pcapw.hip's shape):
//   fg_decide_kernel  a lane owns a source packet, a block a tile of 256 (or several where the launch caps the grid
//                     for the counters): offset, length, select byte, mtu and chain (the first four rows up front,
//                     chain_load), the IP entry (frag_find_step), the one or two aligned 16-byte slab chunks holding
//                     the IP header's bytes 0..11 (take16), the decision of pktgpu_frag.hpp.  Out: status / nfrag,
//                     the packet's plan (16 bytes of scratch: ip_off, per, P, status, chain rows, outputs, length),
//                     the tile's (outputs, rounded bytes), and the per-status counts merged in LDS and added once
//                     per block and non-zero status;
//   out_scan_kernel   (pktgpu_outbatch.hip, shared with reasm and icmp) one block: the exclusive prefix of the tile
//                     sums, the two totals and the overflow verdict to device words and to the ctx's pinned words:
//                     what does not fit is known on the device before anything is written;
//   fg_emit_kernel    per tile again: a block scan gives each packet's first output index and offset (first[]);
//                     then each wave spreads the rows of its 64 packets over its lanes (a search in the wave's
//                     prefix of the output counts), since a packet's rows are closed-form from per and P: out_off,
//                     out_len, src_index, frag_index and the out_chain rows.  A packet of 8190 fragments costs 128
//                     rounds of the wave, not 8190 turns of one lane;
//   fg_copy_kernel    a wave walks 64 outputs' 16-byte chunks together (pkt_reorder_batch's walk): lane r stages
//                     output r (destination, source, length, ip_off, the payload's shift j * per and the rebuilt
//                     header words) in LDS, the wave keeps the prefix of the chunk counts and its lanes take the
//                     chunks 64 at a time.  A chunk is built in registers: bytes below ip_off + 20 come from the
//                     source at the same place, bytes from there on from the source j * per further (a second pair
//                     of aligned loads only in the chunk the boundary falls in, when j > 0), the 12 rebuilt header
//                     bytes are laid over it, bytes past the output's length are zero, and the chunk is stored whole.
//                     Lanes past the last output write the empty tail of the per-output arrays.
// dst is never read; emit and copy exit when the outputs do not fit.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pktgpu_ctx.hpp"
#include "pktgpu_frag.hpp"

namespace {

constexpr uint32_t kGBlock = 256;
constexpr uint32_t kGWaves = kGBlock / 64;
constexpr uint32_t kCountBlocks = 1280;  // the counting launches' grid cap (fwd_kernel's, taken over, not measured again)
constexpr uint32_t kFitsIpo = 0x7FFFFF00u;  // a FITS output's staged ip_off: no header, no second source

struct GParams {
    BatchSrc src;
    uint64_t n;  // < 2^32
    const uint8_t* n_hdrs;
    const uint8_t* hdr_type;  // [PKT_MAX_HDRS][n]
    const uint16_t* hdr_off;  // [PKT_MAX_HDRS][n]
    uint32_t which, flags, mtu_all;
    const uint16_t* mtu;
    const uint8_t* select;
    uint8_t* status;
    uint32_t* nfrag;
    uint32_t* first;
    uint64_t* hits;
    uint4* plan;          // scratch, [n]
    uint64_t* blk_bytes;  // scratch, [tiles]
    uint64_t* blk_cnt;    // scratch, [tiles]
    uint64_t* tot;        // scratch: [bytes, outputs, overflow]
    // the outputs (not with NO_WRITE)
    uint8_t* dst;
    uint64_t dst_len, out_cap;
    uint64_t* out_off;
    uint32_t* out_len;
    uint32_t* src_index;   // the caller's, may be NULL
    uint16_t* frag_index;  // the caller's, may be NULL
    uint32_t* k_src;       // the caller's or scratch
    uint16_t* k_frag;      // the caller's or scratch
    uint8_t* oc_nh;
    uint8_t* oc_ty;
    uint16_t* oc_of;
};

__device__ __forceinline__ uint4 plan_pack(const FragPlan& p) {
    return make_uint4(p.ipo | p.per << 16, p.pay | p.st << 16 | p.nh << 24, p.nout, p.len);
}
__device__ __forceinline__ FragPlan plan_unpack(uint4 v) {
    FragPlan p;
    p.ipo = v.x & 0xFFFFu, p.per = v.x >> 16;
    p.pay = v.y & 0xFFFFu, p.st = v.y >> 16 & 0xFFu, p.nh = v.y >> 24;
    p.nout = v.z;
    p.len = v.w;
    return p;
}

// the IP header's bytes [S, S + 12) of the slab, which lie inside a packet: the aligned chunk of S, and the next one
// iff it holds a byte of them (so it lies at or below the slab's last chunk)
__device__ __forceinline__ void load_hdr12(const uint8_t* slab, uint64_t S, uint32_t h[4]) {
    const uint32_t sh = (uint32_t)S & 15u;
    const uint8_t* A = slab + (S & ~(uint64_t)15);
    const uint4 c0 = *reinterpret_cast<const uint4*>(A);
    const uint4 c1 = sh + 12u > 16u ? *reinterpret_cast<const uint4*>(A + 16) : make_uint4(0, 0, 0, 0);
    take16(c0, c1, sh, h);
}

__global__ __launch_bounds__(kGBlock) void fg_decide_kernel(GParams P) {
    __shared__ uint32_t s_hits[PKT_FRAG_STATUS_COUNT];
    __shared__ uint64_t s_w[kGWaves];
    const uint32_t t = threadIdx.x;
    if (P.hits) hits_zero<PKT_FRAG_STATUS_COUNT>(s_hits, t);
    const uint32_t ntiles = (uint32_t)((P.n + kGBlock - 1) / kGBlock);
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {  // uniform
        const uint64_t i = (uint64_t)tile * kGBlock + t;
        const bool act = i < P.n;
        FragPlan p{};
        p.st = PKT_FRAG_SKIPPED;
        if (act) {
            const uint64_t off = pkt_off(P.src, i);
            p.len = pkt_len(P.src, i, off);
            const ChainPre c = chain_load(P, i);
            const uint32_t sel = P.select ? P.select[i] : 1u;
            const uint32_t m = P.mtu ? P.mtu[i] : P.mtu_all;
            if (sel) {
                const uint32_t nh = c.nh > PKT_MAX_HDRS ? PKT_MAX_HDRS : c.nh;
                FragFind f;
#pragma unroll
                for (uint32_t j = 0; j < 4; j++)
                    if (j < nh) frag_find_step(f, P.which, j, c.ty[j], c.of[j]);
                for (uint32_t j = 4; j < nh; j++) {
                    const uint32_t ty = P.hdr_type[(uint64_t)j * P.n + i];
                    if (!fwd_is_ip(ty)) continue;
                    frag_find_step(f, P.which, j, ty, P.hdr_off[(uint64_t)j * P.n + i]);
                }
                p.st = frag_find_status(f, p.len);
                if (p.st == PKT_FRAG_FITS) {
                    uint32_t h[4];
                    load_hdr12(P.src.slab, off + f.ipo, h);
                    frag_decide(p, f.ipt, f.ipo, p.len, h, m);
                    frag_finish(p, f, nh, P.flags);
                }
            }
            P.plan[i] = plan_pack(p);
            if (P.status) P.status[i] = (uint8_t)p.st;
            if (P.nfrag) P.nfrag[i] = p.nout;
        }
        // the tile's sums: at most 256 * 8190 outputs
        uint64_t tc, tb;
        (void)block_excl_scan<kGWaves>(act ? p.nout : 0u, s_w, tc);
        (void)block_excl_scan<kGWaves>(act ? frag_out_bytes(p) : 0u, s_w, tb);
        if (t == 0) {
            P.blk_cnt[tile] = tc;
            P.blk_bytes[tile] = tb;
        }
        if (P.hits) hits_add<PKT_FRAG_STATUS_COUNT>(s_hits, t, act, p.st);
    }
    if (P.hits) hits_flush<PKT_FRAG_STATUS_COUNT>(s_hits, t, P.hits);
}

__global__ __launch_bounds__(kGBlock) void fg_emit_kernel(GParams P) {
    __shared__ uint64_t s_w[kGWaves];
    __shared__ uint32_t s_pre[kGWaves][65];
    __shared__ uint64_t s_q[kGWaves][64], s_o[kGWaves][64];
    __shared__ uint4 s_plan[kGWaves][64];
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
    const uint64_t i = (uint64_t)blockIdx.x * kGBlock + t;
    const bool act = i < P.n;
    const uint4 raw = act ? P.plan[i] : make_uint4(0, 0, 0, 0);
    const FragPlan p = plan_unpack(raw);
    uint64_t tc, tb;
    const uint64_t q0 = P.blk_cnt[blockIdx.x] + block_excl_scan<kGWaves>(p.nout, s_w, tc);
    const uint64_t o0 = P.blk_bytes[blockIdx.x] + block_excl_scan<kGWaves>(frag_out_bytes(p), s_w, tb);
    if (act && P.first) P.first[i] = p.nout ? (uint32_t)q0 : PKT_FRAG_NONE;
    if ((P.flags & PKT_FRAG_NO_WRITE) || P.tot[2]) return;  // (uniform) the sizing pass, or the outputs do not fit
    // the wave's rows: at most 64 * 8190
    const uint32_t incl = wave_incl_scan(p.nout, lane);
    s_pre[wv][lane + 1] = incl;
    if (lane == 0) s_pre[wv][0] = 0;
    s_q[wv][lane] = q0;
    s_o[wv][lane] = o0;
    s_plan[wv][lane] = raw;
    wave_sync();
    const uint32_t rows = s_pre[wv][64];
    const uint64_t ibase = i - lane;
    for (uint32_t f = lane; f < rows; f += 64) {
        // the packet holding row f: the number of prefix ends at or below f (locate()'s search, written out here and
        // in the copy kernel: a shared helper taking the prefix as a pointer moved both kernels' code)
        uint32_t s = 0;
#pragma unroll
        for (uint32_t st = 32; st; st >>= 1)
            if (s_pre[wv][s + st] <= f) s += st;
        const uint32_t j = f - s_pre[wv][s];
        const FragPlan r = plan_unpack(s_plan[wv][s]);
        const uint64_t q = s_q[wv][s] + j;  // < the outputs' total <= out_cap
        const uint64_t src = ibase + s;
        P.out_off[q] = s_o[wv][s] + frag_out_rel(r, j);
        P.out_len[q] = frag_out_len(r, j);
        P.k_src[q] = (uint32_t)src;
        P.k_frag[q] = (uint16_t)j;
        if (P.oc_nh) P.oc_nh[q] = (uint8_t)r.nh;
        for (uint32_t k = 0; k < r.nh; k++) {
            if (P.oc_ty) P.oc_ty[(uint64_t)k * P.out_cap + q] = P.hdr_type[(uint64_t)k * P.n + src];
            if (P.oc_of) P.oc_of[(uint64_t)k * P.out_cap + q] = P.hdr_off[(uint64_t)k * P.n + src];
        }
    }
}

__global__ __launch_bounds__(kGBlock) void fg_copy_kernel(GParams P) {
    __shared__ uint32_t s_pre[kGWaves][65];
    __shared__ uint64_t s_dst[kGWaves][64], s_src[kGWaves][64];
    __shared__ uint32_t s_len[kGWaves][64], s_ipo[kGWaves][64], s_delta[kGWaves][64];
    __shared__ uint32_t s_h[kGWaves][3][64];
    if (P.tot[2]) return;  // (uniform) the outputs do not fit: the host reports the capacity needed
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
    const uint64_t n_out = P.tot[1];
    const uint64_t q = (uint64_t)blockIdx.x * kGBlock + t;
    uint32_t chunks = 0;
    if (q < n_out) {
        const uint64_t i = P.k_src[q];
        const uint32_t j = P.k_frag[q];
        const FragPlan p = plan_unpack(P.plan[i]);
        const uint64_t off = pkt_off(P.src, i);
        const uint32_t ol = frag_out_len(p, j);
        uint32_t o[3] = {0, 0, 0};
        uint32_t ipo = kFitsIpo, delta = 0;
        if (p.st == PKT_FRAG_SPLIT) {
            uint32_t h[4];
            load_hdr12(P.src.slab, off + p.ipo, h);
            frag_header(p, j, h, o);
            ipo = p.ipo;
            delta = j * p.per;
        }
        s_dst[wv][lane] = P.out_off[q];
        s_src[wv][lane] = off;
        s_len[wv][lane] = ol;
        s_ipo[wv][lane] = ipo;
        s_delta[wv][lane] = delta;
        s_h[wv][0][lane] = o[0], s_h[wv][1][lane] = o[1], s_h[wv][2][lane] = o[2];
        chunks = (ol + 15u) >> 4;
    } else if (q < P.out_cap) {  // the empty tail
        P.out_off[q] = 0;
        P.out_len[q] = 0;
        if (P.src_index) P.src_index[q] = PKT_FRAG_NONE;
        if (P.frag_index) P.frag_index[q] = 0;
        if (P.oc_nh) P.oc_nh[q] = 0;
    }
    const uint32_t incl = wave_incl_scan(chunks, lane);
    s_pre[wv][lane + 1] = incl;
    if (lane == 0) s_pre[wv][0] = 0;
    wave_sync();
    const uint32_t total = s_pre[wv][64];  // at most 64 * 4096
    const uint64_t last16 = slab_last16(P.src);
    for (uint32_t f = lane; f < total; f += 64) {
        uint32_t s = 0;
#pragma unroll
        for (uint32_t st = 32; st; st >>= 1)
            if (s_pre[wv][s + st] <= f) s += st;
        const uint32_t B0 = 16u * (f - s_pre[wv][s]);  // the chunk's first byte within the output, < its length
        const uint32_t ol = s_len[wv][s], ipo = s_ipo[wv][s], delta = s_delta[wv][s];
        const uint64_t src = s_src[wv][s];
        const uint32_t he = ipo + 20u;
        // bytes [0, na) of the chunk come from the source at the same place, the rest from `delta` further on
        const uint32_t na = delta == 0 || he >= B0 + 16u ? 16u : he > B0 ? he - B0 : 0u;
        Le128 v{0, 0};
        if (na) v = load16(P.src.slab, src + B0, last16);
        if (na < 16u) {
            const Le128 c = load16(P.src.slab, src + delta + B0, last16);
            const Le128 m = bytes_below(na);
            v.lo = (v.lo & m.lo) | (c.lo & ~m.lo);
            v.hi = (v.hi & m.hi) | (c.hi & ~m.hi);
        }
        // the rebuilt header's bytes 0..11 at ipo - B0
        const int32_t rel = (int32_t)ipo - (int32_t)B0;
        if (rel > -12 && rel < 16) {
            const Le128 hv{(uint64_t)s_h[wv][0][s] | (uint64_t)s_h[wv][1][s] << 32, (uint64_t)s_h[wv][2][s]};
            const Le128 hm{~0ull, 0xFFFFFFFFull};
            const Le128 sv = rel >= 0 ? bytes_up(hv, (uint32_t)rel) : bytes_down(hv, (uint32_t)-rel);
            const Le128 sm = rel >= 0 ? bytes_up(hm, (uint32_t)rel) : bytes_down(hm, (uint32_t)-rel);
            v.lo = (v.lo & ~sm.lo) | sv.lo;
            v.hi = (v.hi & ~sm.hi) | sv.hi;
        }
        const Le128 keep = bytes_below(ol - B0 > 16u ? 16u : ol - B0);
        v.lo &= keep.lo;
        v.hi &= keep.hi;
        *reinterpret_cast<uint4*>(P.dst + s_dst[wv][s] + B0) =
            make_uint4((uint32_t)v.lo, (uint32_t)(v.lo >> 32), (uint32_t)v.hi, (uint32_t)(v.hi >> 32));
    }
}

constexpr OutEntry kFragEntry{&pkt_ctx::fr, "pkt_frag_batch", "pkt_frag_result"};

// The launches, queued on s.  The totals and the verdict arrive in ctx->fr.ctl once the stream has passed them.
int fg_queue(pkt_ctx_t* ctx, const pkt_batch_t* b, const pkt_chain_t* chain, uint32_t which_ip, uint32_t flags,
             const uint16_t* mtu, uint32_t mtu_all, const uint8_t* select, uint8_t* status, uint32_t* nfrag,
             uint32_t* first, uint8_t* dst, uint64_t dst_len, uint64_t out_cap, uint64_t* out_off, uint32_t* out_len,
             uint32_t* src_index, uint16_t* frag_index, const pkt_chain_t* out_chain, uint64_t* hits, hipStream_t s) {
    if (!ctx) return PKT_ERR_INVALID_ARG;
    if (const char* msg = frag_call_error(b, chain, which_ip, flags, mtu, mtu_all, dst, out_cap, out_off, out_len, hits, true))
        return pktgpu_out_refuse(ctx, kFragEntry, msg);
    OutScratch& fr = ctx->fr;
    if (fr.pending)
        return pktgpu_out_refuse(ctx, kFragEntry, "a queued call's result has not been taken on this ctx (pkt_frag_result)");
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    const bool write = !(flags & PKT_FRAG_NO_WRITE);
    if (!write) out_cap = 0;
    const uint64_t n = b->n;
    const uint32_t nb = (uint32_t)((n + kGBlock - 1) / kGBlock);
    const uint64_t o_bytes = 64, o_cnt = o_bytes + round16(8ull * nb), o_plan = o_cnt + round16(8ull * nb);
    const uint64_t o_ksrc = o_plan + 16 * n, o_kfrag = o_ksrc + (src_index || !write ? 0 : round16(4 * out_cap));
    const uint64_t need = o_kfrag + (frag_index || !write ? 0 : round16(2 * out_cap));
    if ((e = fr.reserve(need)) != hipSuccess) return hip_fail(ctx, e, "hipMalloc (pkt_frag_batch)");
    if ((e = fr.ensure(64)) != hipSuccess) return hip_fail(ctx, e, "hipHostMalloc (pkt_frag_batch)");
    char* p = static_cast<char*>(fr.buf);
    GParams P{};
    P.src = batch_src(b);
    P.n = n;
    P.n_hdrs = chain->n_hdrs;
    P.hdr_type = chain->hdr_type;
    P.hdr_off = chain->hdr_off;
    P.which = which_ip;
    P.flags = flags;
    P.mtu_all = mtu_all;
    P.mtu = mtu;
    P.select = select;
    P.status = status;
    P.nfrag = nfrag;
    P.first = first;
    P.hits = hits;
    P.tot = reinterpret_cast<uint64_t*>(p);
    P.blk_bytes = reinterpret_cast<uint64_t*>(p + o_bytes);
    P.blk_cnt = reinterpret_cast<uint64_t*>(p + o_cnt);
    P.plan = reinterpret_cast<uint4*>(p + o_plan);
    if (write) {
        P.dst = dst;
        P.dst_len = dst_len;
        P.out_cap = out_cap;
        P.out_off = out_off;
        P.out_len = out_len;
        P.src_index = src_index;
        P.frag_index = frag_index;
        P.k_src = src_index ? src_index : reinterpret_cast<uint32_t*>(p + o_ksrc);
        P.k_frag = frag_index ? frag_index : reinterpret_cast<uint16_t*>(p + o_kfrag);
        const OutChainCols oc = out_chain_cols(out_chain);
        P.oc_nh = oc.nh, P.oc_ty = oc.ty, P.oc_of = oc.of;
    }
    fr.ctl[0] = fr.ctl[1] = fr.ctl[2] = 0;
    if (nb) {
        const uint32_t grid = hits && nb > kCountBlocks ? kCountBlocks : nb;
        hipLaunchKernelGGL(fg_decide_kernel, dim3(grid), dim3(kGBlock), 0, s, P);
    }
    pktgpu_out_scan_launch(P.blk_bytes, P.blk_cnt, nb, !write, out_cap, dst_len, P.tot, fr.ctl_dev, s);
    if (nb && (write || first)) hipLaunchKernelGGL(fg_emit_kernel, dim3(nb), dim3(kGBlock), 0, s, P);
    if (write)
        hipLaunchKernelGGL(fg_copy_kernel, dim3((unsigned)((out_cap + kGBlock - 1) / kGBlock)), dim3(kGBlock), 0, s, P);
    if ((e = hipGetLastError()) != hipSuccess) return hip_fail(ctx, e, "pkt_frag_batch launch");
    return PKT_SUCCESS;
}

}  // namespace

extern "C" {

int pkt_frag_batch(pkt_ctx_t* ctx, const pkt_batch_t* batch, const pkt_chain_t* chain, uint32_t which_ip, uint32_t flags,
                   const uint16_t* mtu, uint32_t mtu_all, const uint8_t* select, uint8_t* status, uint32_t* nfrag,
                   uint32_t* first, uint8_t* dst, uint64_t dst_len, uint64_t out_cap, uint64_t* out_off, uint32_t* out_len,
                   uint32_t* src_index, uint16_t* frag_index, const pkt_chain_t* out_chain, uint64_t* hits,
                   uint64_t* bytes_out_total, uint64_t* n_out, void* stream) {
    const auto queue = [&](hipStream_t s) {
        return fg_queue(ctx, batch, chain, which_ip, flags, mtu, mtu_all, select, status, nfrag, first, dst, dst_len, out_cap,
                        out_off, out_len, src_index, frag_index, out_chain, hits, s);
    };
    return pktgpu_out_batch(ctx, kFragEntry, queue, stream, bytes_out_total, n_out);
}

int pkt_frag_batch_async(pkt_ctx_t* ctx, const pkt_batch_t* batch, const pkt_chain_t* chain, uint32_t which_ip,
                         uint32_t flags, const uint16_t* mtu, uint32_t mtu_all, const uint8_t* select, uint8_t* status,
                         uint32_t* nfrag, uint32_t* first, uint8_t* dst, uint64_t dst_len, uint64_t out_cap,
                         uint64_t* out_off, uint32_t* out_len, uint32_t* src_index, uint16_t* frag_index,
                         const pkt_chain_t* out_chain, uint64_t* hits, void* stream) {
    const auto queue = [&](hipStream_t s) {
        return fg_queue(ctx, batch, chain, which_ip, flags, mtu, mtu_all, select, status, nfrag, first, dst, dst_len, out_cap,
                        out_off, out_len, src_index, frag_index, out_chain, hits, s);
    };
    return pktgpu_out_batch_async(ctx, kFragEntry, queue, stream);
}

int pkt_frag_result(pkt_ctx_t* ctx, uint64_t* bytes_out_total, uint64_t* n_out) {
    return pktgpu_out_result(ctx, kFragEntry, bytes_out_total, n_out);
}

}  // extern "C"
