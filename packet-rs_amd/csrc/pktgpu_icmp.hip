// pktgpu_icmp.hip — pkt_icmp_err_batch / _async / _result: one ICMP / ICMPv6 error packet for every source packet
// that may be answered, packed at 16-byte-aligned offsets of a second slab (pkt_frag_batch's output contract), in
// three launches with no waiting between blocks:
//   ic_decide_kernel  a lane owns a source packet, a block a tile of 256 (or several where the launch caps the grid
//                     for the counters): offset, length, select byte, code (through the map that came with the
//                     launch), mtu and chain (the first four rows up front, chain_load; later rows only for chains
//                     that have them), the IP and the Ether entry (icmp_find_step), the aligned 16-byte slab chunks
//                     holding the IP header's bytes 0..31, the byte behind an IPv6 header and the Ether
//                     destination's first byte (take16), the decision of pktgpu_icmp.hpp.  Out: status, the packet's
//                     plan (32 bytes of scratch), the tile's (outputs, rounded bytes), and the per-status counts
//                     merged in LDS and added once per block and non-zero status;
//   out_scan_kernel   (pktgpu_outbatch.hip, shared with frag and reasm) one block: the exclusive prefix of the tile
//                     sums, the two totals and the overflow verdict to device words and to the ctx's pinned words;
//   ic_build_kernel   per tile again: a block scan gives each answered packet its output index and offset; the lane
//                     writes out_index and its output's row of the per-output arrays and stages the output in LDS
//                     (destination, source, offsets, Q and the 28 / 48 header bytes of icmp_headers, the ICMP
//                     checksum still zero).  Then the wave walks its 64 sources' 16-byte chunks together
//                     (fg_copy_kernel's walk): a chunk is built in registers from the swapped L2 prefix (the source
//                     at eth_off + B0), the header words (LDS) and the quote (the source at ip_off + B0 - P - H - 8:
//                     two aligned loads, shifted into the output's phase), bytes past the output's length are zero,
//                     and it is stored whole.  The quote bytes of a chunk are summed as eight native 16-bit words
//                     and added to the output's LDS word; all chunks of an output start at the same parity of the
//                     quote (P's), so the sum is byte-swapped once at the end when P is even.  The one or two
//                     chunks holding the ICMP checksum are not stored in the walk: once the wave's sums are
//                     complete, the owning lane finishes the checksum, lays it into the staged header and stores
//                     them.  Lanes past the last output write the empty tail of the per-output arrays.
// dst is never read; the build kernel stores nothing when the outputs do not fit.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pktgpu_ctx.hpp"
#include "pktgpu_icmp.hpp"

namespace {

constexpr uint32_t kIBlock = 256;
constexpr uint32_t kIWaves = kIBlock / 64;
constexpr uint32_t kCountBlocks = 1280;  // the counting launch's grid cap (fwd_kernel's, taken over, not measured again)

struct IParams {
    BatchSrc src;
    uint64_t n;  // < 2^32
    const uint8_t* n_hdrs;
    const uint8_t* hdr_type;  // [PKT_MAX_HDRS][n]
    const uint16_t* hdr_off;  // [PKT_MAX_HDRS][n]
    uint32_t which, flags, code_all, mtu_all;
    const uint8_t* code;
    const uint16_t* mtu;
    const uint8_t* select;
    uint8_t* status;
    uint32_t* out_index;
    uint64_t* hits;
    uint4* plan;          // scratch, [n][2]
    uint64_t* blk_bytes;  // scratch, [tiles]
    uint64_t* blk_cnt;    // scratch, [tiles]
    uint64_t* tot;        // scratch: [bytes, outputs, overflow]
    // the outputs (not with NO_WRITE)
    uint8_t* dst;
    uint64_t dst_len, out_cap;
    uint64_t* out_off;
    uint32_t* out_len;
    uint32_t* src_index;
    uint8_t* oc_nh;
    uint8_t* oc_ty;
    uint16_t* oc_of;
};

// what a launch takes: the parameters and the cfg with its map, by value
struct IArgs {
    IParams P;
    IcmpCfg cfg;
};

__device__ __forceinline__ void plan_pack(const IcmpPlan& p, uint4& a, uint4& b) {
    a = make_uint4(p.st | p.v4 << 8 | p.e_eth << 12 | p.e_ip << 16, p.eth | p.ipo << 16, p.q | p.type << 16 | p.code << 24,
                   p.mtu);
    b = make_uint4(p.sa[0], p.sa[1], p.sa[2], p.sa[3]);
}
__device__ __forceinline__ IcmpPlan plan_unpack(uint4 a, uint4 b) {
    IcmpPlan p;
    p.st = a.x & 0xFFu, p.v4 = a.x >> 8 & 1u, p.e_eth = a.x >> 12 & 15u, p.e_ip = a.x >> 16 & 15u;
    p.eth = a.y & 0xFFFFu, p.ipo = a.y >> 16;
    p.q = a.z & 0xFFFFu, p.type = a.z >> 16 & 0xFFu, p.code = a.z >> 24;
    p.mtu = a.w;
    p.sa[0] = b.x, p.sa[1] = b.y, p.sa[2] = b.z, p.sa[3] = b.w;
    return p;
}

// the slab byte at pos < slab_len, out of its aligned chunk
__device__ __forceinline__ uint32_t load_byte(const uint8_t* slab, uint64_t pos) {
    const uint4 v = *reinterpret_cast<const uint4*>(slab + (pos & ~(uint64_t)15));
    const uint32_t k = (uint32_t)pos >> 2 & 3u;
    const uint32_t w = k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w;
    return w >> (8u * ((uint32_t)pos & 3u)) & 0xFFu;
}

__global__ __launch_bounds__(kIBlock) void ic_decide_kernel(IArgs A) {
    const IParams& P = A.P;
    __shared__ uint32_t s_hits[PKT_ICMPE_STATUS_COUNT];
    __shared__ uint64_t s_w[kIWaves];
    const uint32_t t = threadIdx.x;
    if (P.hits) hits_zero<PKT_ICMPE_STATUS_COUNT>(s_hits, t);
    const uint32_t ntiles = (uint32_t)((P.n + kIBlock - 1) / kIBlock);
    const uint64_t last16 = slab_last16(P.src);
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {  // uniform
        const uint64_t i = (uint64_t)tile * kIBlock + t;
        const bool act = i < P.n;
        IcmpPlan p{};
        p.st = PKT_ICMPE_SKIPPED;
        if (act) {
            const uint64_t off = pkt_off(P.src, i);
            const uint32_t len = pkt_len(P.src, i, off);
            const ChainPre c = chain_load(P, i);
            const uint32_t sel = P.select ? P.select[i] : 1u;
            const uint32_t cd = P.code ? P.code[i] : P.code_all;
            const uint32_t m = P.mtu ? P.mtu[i] : P.mtu_all;
            const uint32_t r = A.cfg.has_map ? A.cfg.map[cd & 0xFFu] : cd;
            p.st = icmp_reason_status(sel, r);
            IcmpFind f;
            if (p.st == PKT_ICMPE_SENT) {
                const uint32_t nh = c.nh > PKT_MAX_HDRS ? PKT_MAX_HDRS : c.nh;
#pragma unroll
                for (uint32_t j = 0; j < 4; j++)
                    if (j < nh) icmp_find_step(f, P.which, j, c.ty[j], c.of[j]);
                for (uint32_t j = 4; j < nh; j++) {
                    const uint32_t ty = P.hdr_type[(uint64_t)j * P.n + i];
                    if (!fwd_wants(ty)) continue;
                    icmp_find_step(f, P.which, j, ty, P.hdr_off[(uint64_t)j * P.n + i]);
                }
                p.st = icmp_find_status(f, len);
            }
            if (p.st == PKT_ICMPE_SENT) {
                // the IP entry's bytes 0..31 (the first 20 / 40 lie inside the packet, so byte 16 does), the byte
                // behind an IPv6 header when the packet has it, the Ether destination's first byte
                const uint64_t S = off + f.ipo;
                const bool v4 = f.ipt == PKT_HDR_IPV4;
                uint32_t h[8];
                load16w(P.src.slab, S, last16, h);
                load16w(P.src.slab, S + 16, last16, h + 4);
                uint32_t tb = h[5];
                if (!v4 && f.ipo + 40u < len) tb = load_byte(P.src.slab, S + 40);
                const uint32_t ed0 = load_byte(P.src.slab, off + f.eth);
                icmp_decide(p, f, len, r, h, tb, ed0, m, A.cfg);
            }
            uint4 a, b;
            plan_pack(p, a, b);
            P.plan[2 * i] = a;
            P.plan[2 * i + 1] = b;
            if (P.status) P.status[i] = (uint8_t)p.st;
        }
        const bool sent = act && p.st == PKT_ICMPE_SENT;
        uint64_t tc, tb;
        (void)block_excl_scan<kIWaves>(sent ? 1u : 0u, s_w, tc);
        (void)block_excl_scan<kIWaves>(sent ? out_round16(icmp_out_len(p)) : 0u, s_w, tb);
        if (t == 0) {
            P.blk_cnt[tile] = tc;
            P.blk_bytes[tile] = tb;
        }
        if (P.hits) hits_add<PKT_ICMPE_STATUS_COUNT>(s_hits, t, act, p.st);
    }
    if (P.hits) hits_flush<PKT_ICMPE_STATUS_COUNT>(s_hits, t, P.hits);
}

__device__ __forceinline__ Le128 le_and(Le128 a, Le128 m) { return Le128{a.lo & m.lo, a.hi & m.hi}; }
__device__ __forceinline__ Le128 le_or(Le128 a, Le128 b) { return Le128{a.lo | b.lo, a.hi | b.hi}; }

// the eight native 16-bit words of c, added (at most 8 * 0xFFFF)
__device__ __forceinline__ uint32_t sum_words(Le128 c) {
    constexpr uint64_t kM = 0x0000FFFF0000FFFFull;
    const uint64_t a = (c.lo & kM) + (c.lo >> 16 & kM) + (c.hi & kM) + (c.hi >> 16 & kM);
    return (uint32_t)a + (uint32_t)(a >> 32);
}

// The output's bytes [B0, B0 + 16), B0 a multiple of 16 below its length P + H + 8 + Q, P = ipo - eth: the source's
// [eth, ipo) with the MACs swapped, the H + 8 header bytes (hdr[k * 64] = dword k of the staged header), the quote
// (source bytes from ipo on), zeros past the length.  quote = the chunk's quote bytes alone, for the sum.
__device__ __forceinline__ Le128 build_chunk(const uint8_t* slab, uint64_t last16, uint64_t src, uint32_t eth,
                                             uint32_t ipo, uint32_t H, uint32_t Q, const uint32_t* hdr, uint32_t B0,
                                             Le128& quote) {
    const uint32_t Pp = ipo - eth, HB = Pp + H + 8u;
    Le128 v{0, 0};
    quote = Le128{0, 0};
    if (B0 < Pp) {  // source byte eth + B0 < ipo lies inside the packet
        Le128 a = load16(slab, src + eth + B0, last16);
        if (B0 == 0) {  // bytes 0..5 <-> 6..11 (P >= 14)
            const uint64_t d = a.lo & 0xFFFFFFFFFFFFull, s = a.lo >> 48 | (a.hi & 0xFFFFFFFFull) << 16;
            a = Le128{s | d << 48, (a.hi & ~0xFFFFFFFFull) | d >> 16};
        }
        v = le_and(a, bytes_below(Pp - B0 > 16u ? 16u : Pp - B0));
    }
    if (B0 + 16u > Pp && B0 < HB) {  // header byte rel + c at chunk byte c; bytes outside [0, H + 8) are zero
        const int32_t rel = (int32_t)B0 - (int32_t)Pp, w0 = rel >> 2, nw = (int32_t)(H + 8u) >> 2;
        uint32_t d[5];
#pragma unroll
        for (int32_t k = 0; k < 5; k++) {
            const int32_t idx = w0 + k;
            d[k] = idx >= 0 && idx < nw ? hdr[idx * 64] : 0u;
        }
        const uint32_t r = (uint32_t)rel & 3u;
        uint32_t o[4];
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) o[k] = __builtin_amdgcn_alignbyte(d[k + 1], d[k], r);
        v = le_or(v, Le128{(uint64_t)o[0] | (uint64_t)o[1] << 32, (uint64_t)o[2] | (uint64_t)o[3] << 32});
    }
    if (B0 + 16u > HB) {  // quote byte qs + c at chunk byte c; qs < Q because B0 is below the length
        const int32_t qs = (int32_t)B0 - (int32_t)HB;
        const uint32_t lo = qs < 0 ? (uint32_t)-qs : 0u, k0 = qs < 0 ? 0u : (uint32_t)qs;
        Le128 c = load16(slab, src + ipo + k0, last16);  // k0 < Q: inside the packet
        c = bytes_up(c, lo);
        const uint32_t end = (uint32_t)((int32_t)Q - qs);  // the chunk byte behind the quote's last
        quote = le_and(c, bytes_below(end > 16u ? 16u : end));
        v = le_or(v, quote);
    }
    return v;
}

__device__ __forceinline__ void store_chunk(uint8_t* p, Le128 v) {
    *reinterpret_cast<uint4*>(p) = make_uint4((uint32_t)v.lo, (uint32_t)(v.lo >> 32), (uint32_t)v.hi, (uint32_t)(v.hi >> 32));
}

__global__ __launch_bounds__(kIBlock) void ic_build_kernel(IArgs A) {
    const IParams& P = A.P;
    __shared__ uint64_t s_w[kIWaves];
    __shared__ uint32_t s_pre[kIWaves][65];
    __shared__ uint64_t s_dst[kIWaves][64], s_src[kIWaves][64];
    __shared__ uint32_t s_geo[kIWaves][64], s_q[kIWaves][64], s_sum[kIWaves][64];
    __shared__ uint32_t s_hdr[kIWaves][12][64];
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
    const uint32_t nb = (uint32_t)((P.n + kIBlock - 1) / kIBlock);
    const bool write = !(P.flags & PKT_ICMPE_NO_WRITE) && !P.tot[2];  // (uniform) not the sizing pass, and the outputs fit
    const uint64_t i = (uint64_t)blockIdx.x * kIBlock + t;
    if (write && i >= P.tot[1] && i < P.out_cap) {  // the empty tail
        P.out_off[i] = 0;
        P.out_len[i] = 0;
        if (P.src_index) P.src_index[i] = PKT_ICMPE_NONE;
        if (P.oc_nh) P.oc_nh[i] = 0;
    }
    if (blockIdx.x >= nb) return;  // (uniform) a block of the tail alone
    const bool act = i < P.n;
    const uint4 ra = act ? P.plan[2 * i] : make_uint4(PKT_ICMPE_SKIPPED, 0, 0, 0);
    const uint4 rb = act ? P.plan[2 * i + 1] : make_uint4(0, 0, 0, 0);
    const IcmpPlan p = plan_unpack(ra, rb);
    const bool sent = act && p.st == PKT_ICMPE_SENT;
    const uint32_t ol = sent ? icmp_out_len(p) : 0u;
    uint64_t tc, tb;
    const uint64_t q = P.blk_cnt[blockIdx.x] + block_excl_scan<kIWaves>(sent ? 1u : 0u, s_w, tc);
    const uint64_t o0 = P.blk_bytes[blockIdx.x] + block_excl_scan<kIWaves>(out_round16(ol), s_w, tb);
    if (act && P.out_index) P.out_index[i] = sent ? (uint32_t)q : PKT_ICMPE_NONE;
    if (!write) return;  // (uniform)
    const uint32_t H = icmp_hlen(p), Pp = p.ipo - p.eth;
    uint32_t part = 0;
    if (sent) {  // q < the outputs' total <= out_cap
        const uint64_t off = pkt_off(P.src, i);
        P.out_off[q] = o0;
        P.out_len[q] = ol;
        if (P.src_index) P.src_index[q] = (uint32_t)i;
        const uint32_t rows = p.e_ip - p.e_eth + 1u;  // 2..16
        if (P.oc_nh) P.oc_nh[q] = (uint8_t)(rows + 1u > PKT_MAX_HDRS ? PKT_MAX_HDRS : rows + 1u);
        for (uint32_t k = 0; k < rows; k++) {
            if (P.oc_ty) P.oc_ty[(uint64_t)k * P.out_cap + q] = P.hdr_type[(uint64_t)(p.e_eth + k) * P.n + i];
            if (P.oc_of) P.oc_of[(uint64_t)k * P.out_cap + q] = (uint16_t)(P.hdr_off[(uint64_t)(p.e_eth + k) * P.n + i] - p.eth);
        }
        if (rows < PKT_MAX_HDRS) {
            if (P.oc_ty) P.oc_ty[(uint64_t)rows * P.out_cap + q] = PKT_HDR_ICMP;
            if (P.oc_of) P.oc_of[(uint64_t)rows * P.out_cap + q] = (uint16_t)(Pp + H);
        }
        uint32_t w[12];
        part = icmp_headers(p, q, A.cfg, w);
#pragma unroll
        for (uint32_t k = 0; k < 12; k++) s_hdr[wv][k][lane] = w[k];
        s_dst[wv][lane] = o0;
        s_src[wv][lane] = off;
        s_geo[wv][lane] = p.eth | p.ipo << 16;
        s_q[wv][lane] = p.q | H << 16;
        s_sum[wv][lane] = 0;
    }
    const uint32_t chunks = (ol + 15u) >> 4;
    const uint32_t incl = wave_incl_scan(chunks, lane);
    s_pre[wv][lane + 1] = incl;
    if (lane == 0) s_pre[wv][0] = 0;
    wave_sync();
    const uint32_t total = s_pre[wv][64];  // at most 64 * 8192
    const uint64_t last16 = slab_last16(P.src);
    for (uint32_t f = lane; f < total; f += 64) {
        // the output holding chunk f: the number of prefix ends at or below f (locate()'s search, written out: a
        // shared helper taking the prefix as a pointer moved this kernel's code)
        uint32_t s = 0;
#pragma unroll
        for (uint32_t st = 32; st; st >>= 1)
            if (s_pre[wv][s + st] <= f) s += st;
        const uint32_t k = f - s_pre[wv][s];
        const uint32_t geo = s_geo[wv][s], qh = s_q[wv][s];
        const uint32_t eth = geo & 0xFFFFu, ipo = geo >> 16, sQ = qh & 0xFFFFu, sH = qh >> 16;
        Le128 quote;
        const Le128 v = build_chunk(P.src.slab, last16, s_src[wv][s], eth, ipo, sH, sQ, &s_hdr[wv][0][s], 16u * k, quote);
        if (quote.lo | quote.hi) atomicAdd(&s_sum[wv][s], sum_words(quote));
        const uint32_t cs = ipo - eth + sH + 2u;  // the ICMP checksum's first byte
        if (cs >> 4 != k && (cs + 1u) >> 4 != k) store_chunk(P.dst + s_dst[wv][s] + 16u * k, v);
    }
    wave_sync();
    if (sent) {
        // the quote's sum: its byte 0 sits at the parity of P in every chunk, the low byte of a native word when P is even
        const uint32_t n16 = icmp_fold(s_sum[wv][lane]);
        const uint32_t qsum = Pp & 1u ? n16 : (n16 >> 8 | (n16 & 0xFFu) << 8);
        const uint32_t c = icmp_csum(p, part, qsum);
        s_hdr[wv][H >> 2][lane] |= (c >> 8) << 16 | (c & 0xFFu) << 24;  // the ICMP header's bytes 2..3
        const uint32_t cs = Pp + H + 2u, k0 = cs >> 4, k1 = (cs + 1u) >> 4;
        const uint64_t off = s_src[wv][lane];
        Le128 quote;
        store_chunk(P.dst + o0 + 16u * k0,
                    build_chunk(P.src.slab, last16, off, p.eth, p.ipo, H, p.q, &s_hdr[wv][0][lane], 16u * k0, quote));
        if (k1 != k0)
            store_chunk(P.dst + o0 + 16u * k1,
                        build_chunk(P.src.slab, last16, off, p.eth, p.ipo, H, p.q, &s_hdr[wv][0][lane], 16u * k1, quote));
    }
}

constexpr OutEntry kIcmpEntry{&pkt_ctx::ic, "pkt_icmp_err_batch", "pkt_icmp_err_result"};

// The launches, queued on s.  The totals and the verdict arrive in ctx->ic.ctl once the stream has passed them.
int ic_queue(pkt_ctx_t* ctx, const pkt_batch_t* b, const pkt_chain_t* chain, uint32_t which_ip, uint32_t flags,
             const pkt_icmp_cfg_t* cfg, const uint8_t* code, uint32_t code_all, const uint8_t* map, const uint16_t* mtu,
             uint32_t mtu_all, const uint8_t* select, uint8_t* status, uint32_t* out_index, uint8_t* dst, uint64_t dst_len,
             uint64_t out_cap, uint64_t* out_off, uint32_t* out_len, uint32_t* src_index, const pkt_chain_t* out_chain,
             uint64_t* hits, hipStream_t s) {
    if (!ctx) return PKT_ERR_INVALID_ARG;
    if (const char* msg = icmp_call_error(b, chain, which_ip, flags, cfg, code_all, mtu, mtu_all, dst, out_cap, out_off,
                                          out_len, hits, true))
        return pktgpu_out_refuse(ctx, kIcmpEntry, msg);
    OutScratch& ic = ctx->ic;
    if (ic.pending)
        return pktgpu_out_refuse(ctx, kIcmpEntry, "a queued call's result has not been taken on this ctx (pkt_icmp_err_result)");
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    const bool write = !(flags & PKT_ICMPE_NO_WRITE);
    if (!write) out_cap = 0;
    const uint64_t n = b->n;
    const uint32_t nb = (uint32_t)((n + kIBlock - 1) / kIBlock);
    const uint64_t o_bytes = 64, o_cnt = o_bytes + round16(8ull * nb), o_plan = o_cnt + round16(8ull * nb);
    const uint64_t need = o_plan + 32 * n;
    if ((e = ic.reserve(need)) != hipSuccess) return hip_fail(ctx, e, "hipMalloc (pkt_icmp_err_batch)");
    if ((e = ic.ensure(64)) != hipSuccess) return hip_fail(ctx, e, "hipHostMalloc (pkt_icmp_err_batch)");
    char* p = static_cast<char*>(ic.buf);
    IArgs A{};
    A.cfg = icmp_cfg(*cfg, map);
    IParams& P = A.P;
    P.src = batch_src(b);
    P.n = n;
    P.n_hdrs = chain->n_hdrs;
    P.hdr_type = chain->hdr_type;
    P.hdr_off = chain->hdr_off;
    P.which = which_ip;
    P.flags = flags;
    P.code_all = code_all;
    P.mtu_all = mtu_all;
    P.code = code;
    P.mtu = mtu;
    P.select = select;
    P.status = status;
    P.out_index = out_index;
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
        const OutChainCols oc = out_chain_cols(out_chain);
        P.oc_nh = oc.nh, P.oc_ty = oc.ty, P.oc_of = oc.of;
    }
    ic.ctl[0] = ic.ctl[1] = ic.ctl[2] = 0;
    if (nb) {
        const uint32_t grid = hits && nb > kCountBlocks ? kCountBlocks : nb;
        hipLaunchKernelGGL(ic_decide_kernel, dim3(grid), dim3(kIBlock), 0, s, A);
    }
    pktgpu_out_scan_launch(P.blk_bytes, P.blk_cnt, nb, !write, out_cap, dst_len, P.tot, ic.ctl_dev, s);
    // a block per tile of sources, and enough blocks for the empty tail of the per-output arrays
    const uint64_t tail_blocks = (out_cap + kIBlock - 1) / kIBlock;
    const uint32_t grid = (uint32_t)(write && tail_blocks > nb ? tail_blocks : nb);
    if (grid && (write || out_index)) hipLaunchKernelGGL(ic_build_kernel, dim3(grid), dim3(kIBlock), 0, s, A);
    if ((e = hipGetLastError()) != hipSuccess) return hip_fail(ctx, e, "pkt_icmp_err_batch launch");
    return PKT_SUCCESS;
}

}  // namespace

extern "C" {

int pkt_icmp_err_batch(pkt_ctx_t* ctx, const pkt_batch_t* batch, const pkt_chain_t* chain, uint32_t which_ip,
                       uint32_t flags, const pkt_icmp_cfg_t* cfg, const uint8_t* code, uint32_t code_all,
                       const uint8_t* map, const uint16_t* mtu, uint32_t mtu_all, const uint8_t* select, uint8_t* status,
                       uint32_t* out_index, uint8_t* dst, uint64_t dst_len, uint64_t out_cap, uint64_t* out_off,
                       uint32_t* out_len, uint32_t* src_index, const pkt_chain_t* out_chain, uint64_t* hits,
                       uint64_t* bytes_out_total, uint64_t* n_out, void* stream) {
    const auto queue = [&](hipStream_t s) {
        return ic_queue(ctx, batch, chain, which_ip, flags, cfg, code, code_all, map, mtu, mtu_all, select, status, out_index,
                        dst, dst_len, out_cap, out_off, out_len, src_index, out_chain, hits, s);
    };
    return pktgpu_out_batch(ctx, kIcmpEntry, queue, stream, bytes_out_total, n_out);
}

int pkt_icmp_err_batch_async(pkt_ctx_t* ctx, const pkt_batch_t* batch, const pkt_chain_t* chain, uint32_t which_ip,
                             uint32_t flags, const pkt_icmp_cfg_t* cfg, const uint8_t* code, uint32_t code_all,
                             const uint8_t* map, const uint16_t* mtu, uint32_t mtu_all, const uint8_t* select,
                             uint8_t* status, uint32_t* out_index, uint8_t* dst, uint64_t dst_len, uint64_t out_cap,
                             uint64_t* out_off, uint32_t* out_len, uint32_t* src_index, const pkt_chain_t* out_chain,
                             uint64_t* hits, void* stream) {
    const auto queue = [&](hipStream_t s) {
        return ic_queue(ctx, batch, chain, which_ip, flags, cfg, code, code_all, map, mtu, mtu_all, select, status, out_index,
                        dst, dst_len, out_cap, out_off, out_len, src_index, out_chain, hits, s);
    };
    return pktgpu_out_batch_async(ctx, kIcmpEntry, queue, stream);
}

int pkt_icmp_err_result(pkt_ctx_t* ctx, uint64_t* bytes_out_total, uint64_t* n_out) {
    return pktgpu_out_result(ctx, kIcmpEntry, bytes_out_total, n_out);
}

}  // extern "C"
