// pktgpu_tunnel.hip — pkt_tunnel_create and pkt_tunnel_encap_batch / pkt_tunnel_decap_batch with their _async /
// _result forms: one output packet for every source packet that goes into (comes out of) a tunnel, packed at
// 16-byte-aligned offsets of a second slab (pkt_frag_batch's output contract), in three launches per call with no
// waiting between blocks:
//   tn_encap_decide_kernel / tn_decap_decide_kernel
//                     a lane owns a source packet, a block a tile of 256 (or several where the launch caps the grid
//                     for the counters): offset, length, select byte and chain (the first four rows up front,
//                     chain_load; later rows only for chains that have them), the search of pktgpu_tunnel.hpp, the
//                     table entry (encap: four 16-byte loads) or the lookup (decap), the aligned 16-byte slab chunks
//                     holding the header bytes the tests need (take16), the decision.  Out: status (decap: tunnel_out),
//                     the packet's plan (32 bytes of scratch), the tile's (outputs, rounded bytes), and the per-status
//                     counts merged in LDS and added once per block and non-zero status;
//   out_scan_kernel   (pktgpu_outbatch.hip, shared with frag, reasm and icmp_err) one block: the exclusive prefix of
//                     the tile sums, the two totals and the overflow verdict to device words and the ctx's pinned words;
//   tn_build_kernel   (both calls) per tile again: a block scan gives each OK packet its output index and offset; the
//                     lane writes out_index, its output's row of the per-output arrays and its out_chain rows
//                     (tun_out_row), and stages the output in LDS (destination, source, P, S, I, the header length and,
//                     for encap, the up to 70 header bytes of tun_headers with the UDP checksum still zero).  Then the
//                     wave walks its 64 sources' 16-byte chunks together (fg_copy_kernel's walk): a chunk is built in
//                     registers from the prefix (the source at B0, the ethertype bytes before P set), the header words
//                     (LDS) and the payload (the source at P + S + B0 - P - hl: two aligned loads, shifted into the
//                     output's phase), bytes past the output's length are zero, and it is stored whole.  With UDP_CSUM
//                     the payload bytes of a chunk are summed as eight native 16-bit words into the output's LDS word
//                     (the payload starts at an even output byte, 50 or 70, so the sum is byte-swapped once at the end);
//                     the chunk holding the UDP checksum is not stored in the walk: once the wave's sums are complete
//                     the owning lane finishes the checksum, lays it into the staged header and stores that chunk.
//                     Lanes past the last output write the empty tail of the per-output arrays.
// dst is never read; the build kernel stores nothing when the outputs do not fit.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pktgpu_ctx.hpp"
#include "pktgpu_tunnel.hpp"

namespace {

constexpr uint32_t kTBlock = 256;
constexpr uint32_t kTWaves = kTBlock / 64;
constexpr uint32_t kCountBlocks = 1280;  // the counting launch's grid cap (fwd_kernel's, taken over, not measured again)
constexpr uint32_t kHdrWords = 18;

struct TParams {
    BatchSrc src;
    uint64_t n;  // < 2^32
    const uint8_t* n_hdrs;
    const uint8_t* hdr_type;  // [PKT_MAX_HDRS][n]
    const uint16_t* hdr_off;  // [PKT_MAX_HDRS][n]
    uint32_t which, flags, tunnel_all, ident;
    const uint32_t* tunnel;
    const uint32_t* entropy;
    const uint8_t* select;
    TunView v;
    uint8_t* status;
    uint32_t* out_index;
    uint32_t* tunnel_out;
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

// entry t by four aligned 16-byte loads
__device__ __forceinline__ TunEnt load_entry(const TunEnt* ent, uint32_t t) {
    const uint4* p = reinterpret_cast<const uint4*>(ent + t);
    TunEnt e;
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
        const uint4 v = p[k];
        e.w[4 * k] = v.x, e.w[4 * k + 1] = v.y, e.w[4 * k + 2] = v.z, e.w[4 * k + 3] = v.w;
    }
    return e;
}

__device__ __forceinline__ void plan_store(uint4* plan, uint64_t i, const TunPlan& p) {
    uint32_t a[4], b[4];
    tun_plan_pack(p, a, b);
    plan[2 * i] = make_uint4(a[0], a[1], a[2], a[3]);
    plan[2 * i + 1] = make_uint4(b[0], b[1], b[2], b[3]);
}

// the search over packet i's chain: the first four rows from the registers, the rest for the chains that have them
__device__ __forceinline__ TunFind chain_search(const TParams& P, uint64_t i, const ChainPre& c, uint32_t nh) {
    TunFind f;
#pragma unroll
    for (uint32_t j = 0; j < 4; j++)
        if (j < nh) tun_find_step(f, P.which, j, c.ty[j], c.of[j]);
    for (uint32_t j = 4; j < nh; j++)
        tun_find_step(f, P.which, j, P.hdr_type[(uint64_t)j * P.n + i], P.hdr_off[(uint64_t)j * P.n + i]);
    return f;
}

// what both decision kernels end a tile with: the tile's sums and the counts
template <uint32_t NST>
__device__ __forceinline__ void tile_end(const TParams& P, uint32_t tile, bool act, const TunPlan& p, uint64_t* s_w,
                                         uint32_t* s_hits) {
    const bool sent = act && p.st == 0;
    uint64_t tc, tb;
    (void)block_excl_scan<kTWaves>(sent ? 1u : 0u, s_w, tc);
    (void)block_excl_scan<kTWaves>(sent ? out_round16(tun_out_len(p)) : 0u, s_w, tb);
    if (threadIdx.x == 0) {
        P.blk_cnt[tile] = tc;
        P.blk_bytes[tile] = tb;
    }
    if (P.hits) hits_add<NST>(s_hits, threadIdx.x, act, p.st);
}

static_assert(PKT_TUNE_OK == 0 && PKT_TUND_OK == 0, "tile_end and the build kernel take status 0 for an output");

__global__ __launch_bounds__(kTBlock) void tn_encap_decide_kernel(TParams P) {
    __shared__ uint32_t s_hits[PKT_TUNE_STATUS_COUNT];
    __shared__ uint64_t s_w[kTWaves];
    const uint32_t t = threadIdx.x;
    if (P.hits) hits_zero<PKT_TUNE_STATUS_COUNT>(s_hits, t);
    const uint32_t ntiles = (uint32_t)((P.n + kTBlock - 1) / kTBlock);
    const uint64_t last16 = slab_last16(P.src);
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {  // uniform
        const uint64_t i = (uint64_t)tile * kTBlock + t;
        const bool act = i < P.n;
        TunPlan p{};
        p.st = PKT_TUNE_SKIPPED;
        if (act) {
            const uint64_t off = pkt_off(P.src, i);
            const uint32_t len = pkt_len(P.src, i, off);
            const ChainPre c = chain_load(P, i);
            const uint32_t sel = P.select ? P.select[i] : 1u;
            const uint32_t tn = P.tunnel ? P.tunnel[i] : P.tunnel_all;
            const uint32_t ent = P.entropy ? P.entropy[i] : 0u;
            if (sel) p.st = tn >= P.v.n ? PKT_TUNE_NO_TUNNEL : PKT_TUNE_OK;
            if (p.st == PKT_TUNE_OK) {
                const TunEnt e = load_entry(P.v.ent, tn);
                const uint32_t nh = c.nh > PKT_MAX_HDRS ? PKT_MAX_HDRS : c.nh;
                const TunFind f = chain_search(P, i, c, nh);
                uint32_t rd;
                p.st = tun_encap_find_status(f, e, len, rd);
                if (p.st == PKT_TUNE_OK) {
                    uint32_t h[4] = {0, 0, 0, 0};
                    if (rd != kTunNoRead) load16w(P.src.slab, off + rd, last16, h);  // rd + 2 <= len: inside the slab
                    tun_encap_decide(p, f, e, tn, nh, len, rd, h, ent);
                }
            }
            plan_store(P.plan, i, p);
            if (P.status) P.status[i] = (uint8_t)p.st;
        }
        tile_end<PKT_TUNE_STATUS_COUNT>(P, tile, act, p, s_w, s_hits);
    }
    if (P.hits) hits_flush<PKT_TUNE_STATUS_COUNT>(s_hits, t, P.hits);
}

__global__ __launch_bounds__(kTBlock) void tn_decap_decide_kernel(TParams P) {
    __shared__ uint32_t s_hits[PKT_TUND_STATUS_COUNT];
    __shared__ uint64_t s_w[kTWaves];
    const uint32_t t = threadIdx.x;
    if (P.hits) hits_zero<PKT_TUND_STATUS_COUNT>(s_hits, t);
    const uint32_t ntiles = (uint32_t)((P.n + kTBlock - 1) / kTBlock);
    const uint64_t last16 = slab_last16(P.src);
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {  // uniform
        const uint64_t i = (uint64_t)tile * kTBlock + t;
        const bool act = i < P.n;
        TunPlan p{};
        p.st = PKT_TUND_SKIPPED;
        if (act) {
            const uint64_t off = pkt_off(P.src, i);
            const uint32_t len = pkt_len(P.src, i, off);
            const ChainPre c = chain_load(P, i);
            const uint32_t sel = P.select ? P.select[i] : 1u;
            uint32_t tout = PKT_TUN_NONE;
            if (sel) {
                const uint32_t nh = c.nh > PKT_MAX_HDRS ? PKT_MAX_HDRS : c.nh;
                const TunFind f = chain_search(P, i, c, nh);
                p.st = tun_decap_find_status(f, len);
                if (p.st == PKT_TUND_OK) {
                    // the IP header's 20 / 40 bytes lie inside the packet, so every chunk start below is inside the slab;
                    // the 16 bytes behind the header only if the packet has a byte there
                    const uint64_t S = off + f.ipo;
                    const bool v4 = f.ipt == PKT_HDR_IPV4;
                    const uint32_t H = v4 ? 20u : 40u;
                    uint32_t ip[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, th[4] = {0, 0, 0, 0};
                    load16w(P.src.slab, S, last16, ip);
                    load16w(P.src.slab, S + 16, last16, ip + 4);
                    if (!v4) load16w(P.src.slab, S + 32, last16, ip + 8);
                    if (f.ipo + H < len) load16w(P.src.slab, S + H, last16, th);
                    tun_decap_decide(p, f, nh, len, ip, th, P.v, tout);
                }
            }
            plan_store(P.plan, i, p);
            if (P.status) P.status[i] = (uint8_t)p.st;
            if (P.tunnel_out) P.tunnel_out[i] = tout;
        }
        tile_end<PKT_TUND_STATUS_COUNT>(P, tile, act, p, s_w, s_hits);
    }
    if (P.hits) hits_flush<PKT_TUND_STATUS_COUNT>(s_hits, t, P.hits);
}

__device__ __forceinline__ Le128 le_and(Le128 a, Le128 m) { return Le128{a.lo & m.lo, a.hi & m.hi}; }
__device__ __forceinline__ Le128 le_or(Le128 a, Le128 b) { return Le128{a.lo | b.lo, a.hi | b.hi}; }

// v with byte idx set to val when idx is in 0..15
__device__ __forceinline__ Le128 le_put(Le128 v, int32_t idx, uint32_t val) {
    if (idx < 0 || idx > 15) return v;
    const uint32_t s = 8u * ((uint32_t)idx & 7u);
    const uint64_t m = ~(0xFFull << s), b = (uint64_t)val << s;
    return idx < 8 ? Le128{(v.lo & m) | b, v.hi} : Le128{v.lo, (v.hi & m) | b};
}

// the eight native 16-bit words of c, added (at most 8 * 0xFFFF)
__device__ __forceinline__ uint32_t sum_words(Le128 c) {
    constexpr uint64_t kM = 0x0000FFFF0000FFFFull;
    const uint64_t a = (c.lo & kM) + (c.lo >> 16 & kM) + (c.hi & kM) + (c.hi >> 16 & kM);
    return (uint32_t)a + (uint32_t)(a >> 32);
}

// a staged output's numbers: P | S << 16, and I | hl << 16 | patch << 23 | et6 << 24 | cs << 25 | csw << 26
__device__ __forceinline__ uint32_t meta_pack(const TunPlan& p, uint32_t csw) {
    return p.I | p.hl << 16 | p.patch << 23 | p.et6 << 24 | p.cs << 25 | csw << 26;
}

// The output's bytes [B0, B0 + 16), B0 a multiple of 16 below its length Pp + hl + I: the source's [0, Pp) with the
// ethertype before Pp set when `patch`, the hl header bytes (hdr[k * 64] = dword k of the staged header, zero past hl),
// the payload (source bytes from Pp + S on), zeros past the length.  pay = the chunk's payload bytes alone, for the sum.
__device__ __forceinline__ Le128 build_chunk(const uint8_t* slab, uint64_t last16, uint64_t src, uint32_t Pp, uint32_t S,
                                             uint32_t meta, const uint32_t* hdr, uint32_t B0, Le128& pay) {
    const uint32_t I = meta & 0xFFFFu, hl = meta >> 16 & 127u, HB = Pp + hl;
    Le128 v{0, 0};
    pay = Le128{0, 0};
    if (B0 < Pp) {  // source byte B0 < Pp lies inside the packet
        Le128 a = load16(slab, src + B0, last16);
        a = le_and(a, bytes_below(Pp - B0 > 16u ? 16u : Pp - B0));
        if (meta >> 23 & 1u) {  // Pp >= 2
            const bool v6 = meta >> 24 & 1u;
            a = le_put(a, (int32_t)(Pp - 2u) - (int32_t)B0, v6 ? 0x86u : 0x08u);
            a = le_put(a, (int32_t)(Pp - 1u) - (int32_t)B0, v6 ? 0xDDu : 0x00u);
        }
        v = a;
    }
    if (hl && B0 + 16u > Pp && B0 < HB) {  // header byte rel + c at chunk byte c; bytes outside [0, hl) are zero
        const int32_t rel = (int32_t)B0 - (int32_t)Pp, w0 = rel >> 2;
        uint32_t d[5];
#pragma unroll
        for (int32_t k = 0; k < 5; k++) {
            const int32_t idx = w0 + k;
            d[k] = idx >= 0 && idx < (int32_t)kHdrWords ? hdr[idx * 64] : 0u;
        }
        const uint32_t r = (uint32_t)rel & 3u;
        uint32_t o[4];
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) o[k] = __builtin_amdgcn_alignbyte(d[k + 1], d[k], r);
        v = le_or(v, Le128{(uint64_t)o[0] | (uint64_t)o[1] << 32, (uint64_t)o[2] | (uint64_t)o[3] << 32});
    }
    if (B0 + 16u > HB) {  // payload byte qs + c at chunk byte c; qs < I because B0 is below the length
        const int32_t qs = (int32_t)B0 - (int32_t)HB;
        const uint32_t lo = qs < 0 ? (uint32_t)-qs : 0u, k0 = qs < 0 ? 0u : (uint32_t)qs;
        if (k0 < I) {
            Le128 c = load16(slab, src + Pp + S + k0, last16);  // inside the packet: Pp + S + I <= its length
            c = bytes_up(c, lo);
            const uint32_t end = (uint32_t)((int32_t)I - qs);  // the chunk byte behind the payload's last
            pay = le_and(c, bytes_below(end > 16u ? 16u : end));
            v = le_or(v, pay);
        }
    }
    return v;
}

__device__ __forceinline__ void store_chunk(uint8_t* p, Le128 v) {
    *reinterpret_cast<uint4*>(p) = make_uint4((uint32_t)v.lo, (uint32_t)(v.lo >> 32), (uint32_t)v.hi, (uint32_t)(v.hi >> 32));
}

__global__ __launch_bounds__(kTBlock) void tn_build_kernel(TParams P) {
    __shared__ uint64_t s_w[kTWaves];
    __shared__ uint32_t s_pre[kTWaves][65];
    __shared__ uint64_t s_dst[kTWaves][64], s_src[kTWaves][64];
    __shared__ uint32_t s_geo[kTWaves][64], s_meta[kTWaves][64], s_sum[kTWaves][64];
    __shared__ uint32_t s_hdr[kTWaves][kHdrWords][64];
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
    const uint32_t nb = (uint32_t)((P.n + kTBlock - 1) / kTBlock);
    const bool write = !(P.flags & PKT_TUN_NO_WRITE) && !P.tot[2];  // (uniform) not the sizing pass, and the outputs fit
    const uint64_t i = (uint64_t)blockIdx.x * kTBlock + t;
    if (write && i >= P.tot[1] && i < P.out_cap) {  // the empty tail
        P.out_off[i] = 0;
        P.out_len[i] = 0;
        if (P.src_index) P.src_index[i] = PKT_TUN_NONE;
        if (P.oc_nh) P.oc_nh[i] = 0;
    }
    if (blockIdx.x >= nb) return;  // (uniform) a block of the tail alone
    const bool act = i < P.n;
    const uint4 ra = act ? P.plan[2 * i] : make_uint4(1u, 0, 0, 0);  // status 1: SKIPPED in both calls
    const uint4 rb = act ? P.plan[2 * i + 1] : make_uint4(0, 0, 0, 0);
    const uint32_t pa[4] = {ra.x, ra.y, ra.z, ra.w}, pb[4] = {rb.x, rb.y, rb.z, rb.w};
    const TunPlan p = tun_plan_unpack(pa, pb);
    const bool sent = act && p.st == 0;
    const uint32_t ol = sent ? tun_out_len(p) : 0u;
    uint64_t tc, tb;
    const uint64_t q = P.blk_cnt[blockIdx.x] + block_excl_scan<kTWaves>(sent ? 1u : 0u, s_w, tc);
    const uint64_t o0 = P.blk_bytes[blockIdx.x] + block_excl_scan<kTWaves>(out_round16(ol), s_w, tb);
    if (act && P.out_index) P.out_index[i] = sent ? (uint32_t)q : PKT_TUN_NONE;
    if (!write) return;  // (uniform)
    uint32_t part = 0, csw = 0;
    if (sent) {  // q < the outputs' total <= out_cap
        const uint64_t off = pkt_off(P.src, i);
        P.out_off[q] = o0;
        P.out_len[q] = ol;
        if (P.src_index) P.src_index[q] = (uint32_t)i;
        TunEnt e{};
        if (p.hl) {  // encap: p.t is below the table's size
            e = load_entry(P.v.ent, p.t);
            uint32_t w[kHdrWords];
            part = tun_headers(p, e, q, P.ident, w);
            csw = tun_csum_word(e);
#pragma unroll
            for (uint32_t k = 0; k < kHdrWords; k++) s_hdr[wv][k][lane] = w[k];
        }
        const uint32_t rows = tun_out_rows(p);  // at most PKT_MAX_HDRS
        if (P.oc_nh) P.oc_nh[q] = (uint8_t)rows;
        if (P.oc_ty || P.oc_of)
            for (uint32_t r = 0; r < rows; r++) {
                uint32_t ty = 0, of = 0, j = 0;
                int32_t delta = 0;
                if (!tun_out_row(p, &e, r, ty, of, j, delta)) {
                    ty = P.hdr_type[(uint64_t)j * P.n + i];
                    of = (uint32_t)((int32_t)P.hdr_off[(uint64_t)j * P.n + i] + delta);
                }
                if (P.oc_ty) P.oc_ty[(uint64_t)r * P.out_cap + q] = (uint8_t)ty;
                if (P.oc_of) P.oc_of[(uint64_t)r * P.out_cap + q] = (uint16_t)of;
            }
        s_dst[wv][lane] = o0;
        s_src[wv][lane] = off;
        s_geo[wv][lane] = p.P | p.S << 16;
        s_meta[wv][lane] = meta_pack(p, csw);
        s_sum[wv][lane] = 0;
    }
    const uint32_t chunks = (ol + 15u) >> 4;
    const uint32_t incl = wave_incl_scan(chunks, lane);
    s_pre[wv][lane + 1] = incl;
    if (lane == 0) s_pre[wv][0] = 0;
    wave_sync();
    const uint32_t total = s_pre[wv][64];  // at most 64 * 4101
    const uint64_t last16 = slab_last16(P.src);
    for (uint32_t f = lane; f < total; f += 64) {
        // the output holding chunk f: the number of prefix ends at or below f
        uint32_t s = 0;
#pragma unroll
        for (uint32_t st = 32; st; st >>= 1)
            if (s_pre[wv][s + st] <= f) s += st;
        const uint32_t k = f - s_pre[wv][s];
        const uint32_t geo = s_geo[wv][s], meta = s_meta[wv][s];
        Le128 pay;
        const Le128 v = build_chunk(P.src.slab, last16, s_src[wv][s], geo & 0xFFFFu, geo >> 16, meta, &s_hdr[wv][0][s], 16u * k, pay);
        const bool cs = meta >> 25 & 1u;
        if (cs && (pay.lo | pay.hi)) atomicAdd(&s_sum[wv][s], sum_words(pay));
        // the UDP checksum's chunk (VXLAN: P = 0, header dword csw) waits for the sums
        if (!(cs && (meta >> 26) >> 2 == k)) store_chunk(P.dst + s_dst[wv][s] + 16u * k, v);
    }
    wave_sync();
    if (sent && p.cs) {
        // the payload's byte 0 sits at an even output byte (50 or 70): the low byte of a native word
        const uint32_t n16 = tun_fold(s_sum[wv][lane]);
        const uint32_t c = tun_udp_csum(part, n16 >> 8 | (n16 & 0xFFu) << 8);
        s_hdr[wv][csw][lane] |= c >> 8 | (c & 0xFFu) << 8;  // the UDP header's bytes 6..7
        Le128 pay;
        store_chunk(P.dst + o0 + 16u * (csw >> 2),
                    build_chunk(P.src.slab, last16, s_src[wv][lane], p.P, p.S, s_meta[wv][lane], &s_hdr[wv][0][lane],
                                16u * (csw >> 2), pay));
    }
}

constexpr OutEntry kEncapEntry{&pkt_ctx::te, "pkt_tunnel_encap_batch", "pkt_tunnel_encap_result"};
constexpr OutEntry kDecapEntry{&pkt_ctx::td, "pkt_tunnel_decap_batch", "pkt_tunnel_decap_result"};

// The launches of either call, queued on s.  The totals and the verdict arrive in the scratch's ctl words once the
// stream has passed them.
int tn_queue(pkt_ctx_t* ctx, bool encap, const pkt_batch_t* b, const pkt_chain_t* chain, uint32_t which_ip, uint32_t flags,
             const pkt_tunnel_t* tun, const uint32_t* tunnel, uint32_t tunnel_all, const uint32_t* entropy, uint32_t ident,
             const uint8_t* select, uint8_t* status, uint32_t* out_index, uint32_t* tunnel_out, uint8_t* dst,
             uint64_t dst_len, uint64_t out_cap, uint64_t* out_off, uint32_t* out_len, uint32_t* src_index,
             const pkt_chain_t* out_chain, uint64_t* hits, hipStream_t s) {
    if (!ctx) return PKT_ERR_INVALID_ARG;
    const OutEntry& en = encap ? kEncapEntry : kDecapEntry;
    if (const char* msg = tun_call_error(b, chain, which_ip, flags, tun, encap ? tunnel : tunnel_out, entropy, dst, out_cap,
                                         out_off, out_len, hits, true, ctx->device))
        return pktgpu_out_refuse(ctx, en, msg);
    OutScratch& sc = ctx->*en.scratch;
    if (sc.pending)
        return pktgpu_out_refuse(ctx, en, encap ? "a queued call's result has not been taken on this ctx (pkt_tunnel_encap_result)"
                                                : "a queued call's result has not been taken on this ctx (pkt_tunnel_decap_result)");
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    const bool write = !(flags & PKT_TUN_NO_WRITE);
    if (!write) out_cap = 0;
    const uint64_t n = b->n;
    const uint32_t nb = (uint32_t)((n + kTBlock - 1) / kTBlock);
    const uint64_t o_bytes = 64, o_cnt = o_bytes + round16(8ull * nb), o_plan = o_cnt + round16(8ull * nb);
    const uint64_t need = o_plan + 32 * n;
    if ((e = sc.reserve(need)) != hipSuccess) return hip_fail(ctx, e, "hipMalloc (pkt_tunnel)");
    if ((e = sc.ensure(64)) != hipSuccess) return hip_fail(ctx, e, "hipHostMalloc (pkt_tunnel)");
    char* p = static_cast<char*>(sc.buf);
    TParams P{};
    P.src = batch_src(b);
    P.n = n;
    P.n_hdrs = chain->n_hdrs;
    P.hdr_type = chain->hdr_type;
    P.hdr_off = chain->hdr_off;
    P.which = which_ip;
    P.flags = flags;
    P.tunnel_all = tunnel_all;
    P.ident = ident;
    P.tunnel = tunnel;
    P.entropy = entropy;
    P.select = select;
    P.v = tun->v;
    P.status = status;
    P.out_index = out_index;
    P.tunnel_out = tunnel_out;
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
    sc.ctl[0] = sc.ctl[1] = sc.ctl[2] = 0;
    if (nb) {
        const uint32_t grid = hits && nb > kCountBlocks ? kCountBlocks : nb;
        if (encap)
            hipLaunchKernelGGL(tn_encap_decide_kernel, dim3(grid), dim3(kTBlock), 0, s, P);
        else
            hipLaunchKernelGGL(tn_decap_decide_kernel, dim3(grid), dim3(kTBlock), 0, s, P);
    }
    pktgpu_out_scan_launch(P.blk_bytes, P.blk_cnt, nb, !write, out_cap, dst_len, P.tot, sc.ctl_dev, s);
    // a block per tile of sources, and enough blocks for the empty tail of the per-output arrays
    const uint64_t tail_blocks = (out_cap + kTBlock - 1) / kTBlock;
    const uint32_t grid = (uint32_t)(write && tail_blocks > nb ? tail_blocks : nb);
    if (grid && (write || out_index)) hipLaunchKernelGGL(tn_build_kernel, dim3(grid), dim3(kTBlock), 0, s, P);
    if ((e = hipGetLastError()) != hipSuccess) return hip_fail(ctx, e, "pkt_tunnel launch");
    return PKT_SUCCESS;
}

int tn_destroy(pkt_tunnel* t) {
    if (hipSetDevice(t->device_id) != hipSuccess) return PKT_ERR_HIP;
    return hipFree(t->dev_buf) == hipSuccess ? PKT_SUCCESS : PKT_ERR_HIP;
}

}  // namespace

extern "C" {

int pkt_tunnel_create(pkt_ctx_t* ctx, const pkt_tunnel_entry_t* entries, uint32_t count, pkt_tunnel_t** out) {
    if (!ctx || !out) return fail(ctx, PKT_ERR_INVALID_ARG, "pkt_tunnel_create: null argument");
    *out = nullptr;
    pkt_tunnel* t = new pkt_tunnel;
    int rc = tun_compile(entries, count, t->img, ctx->err);
    if (rc != PKT_SUCCESS) {
        delete t;
        return rc;
    }
    const uint64_t eb = (uint64_t)count * sizeof(TunEnt), sb = t->img.slots.size() * sizeof(uint32_t);
    hipError_t e = hipSetDevice(ctx->device);
    if (e == hipSuccess) e = hipMalloc(&t->dev_buf, eb + sb);
    if (e == hipSuccess) e = hipMemcpy(t->dev_buf, t->img.ent.data(), eb, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(static_cast<char*>(t->dev_buf) + eb, t->img.slots.data(), sb, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(t->dev_buf);
        delete t;
        return hip_fail(ctx, e, "pkt_tunnel_create");
    }
    t->device = true;
    t->device_id = ctx->device;
    t->destroy = tn_destroy;
    t->v = TunView{static_cast<const TunEnt*>(t->dev_buf),
                   reinterpret_cast<const uint32_t*>(static_cast<char*>(t->dev_buf) + eb), count,
                   (uint32_t)t->img.slots.size() - 1u};
    *out = t;
    return PKT_SUCCESS;
}

int pkt_tunnel_encap_batch(pkt_ctx_t* ctx, const pkt_batch_t* batch, const pkt_chain_t* chain, uint32_t which_ip,
                           uint32_t flags, const pkt_tunnel_t* tun, const uint32_t* tunnel, uint32_t tunnel_all,
                           const uint32_t* entropy, uint32_t ident, const uint8_t* select, uint8_t* status,
                           uint32_t* out_index, uint8_t* dst, uint64_t dst_len, uint64_t out_cap, uint64_t* out_off,
                           uint32_t* out_len, uint32_t* src_index, const pkt_chain_t* out_chain, uint64_t* hits,
                           uint64_t* bytes_out_total, uint64_t* n_out, void* stream) {
    const auto queue = [&](hipStream_t s) {
        return tn_queue(ctx, true, batch, chain, which_ip, flags, tun, tunnel, tunnel_all, entropy, ident, select, status,
                        out_index, nullptr, dst, dst_len, out_cap, out_off, out_len, src_index, out_chain, hits, s);
    };
    return pktgpu_out_batch(ctx, kEncapEntry, queue, stream, bytes_out_total, n_out);
}

int pkt_tunnel_encap_batch_async(pkt_ctx_t* ctx, const pkt_batch_t* batch, const pkt_chain_t* chain, uint32_t which_ip,
                                 uint32_t flags, const pkt_tunnel_t* tun, const uint32_t* tunnel, uint32_t tunnel_all,
                                 const uint32_t* entropy, uint32_t ident, const uint8_t* select, uint8_t* status,
                                 uint32_t* out_index, uint8_t* dst, uint64_t dst_len, uint64_t out_cap, uint64_t* out_off,
                                 uint32_t* out_len, uint32_t* src_index, const pkt_chain_t* out_chain, uint64_t* hits,
                                 void* stream) {
    const auto queue = [&](hipStream_t s) {
        return tn_queue(ctx, true, batch, chain, which_ip, flags, tun, tunnel, tunnel_all, entropy, ident, select, status,
                        out_index, nullptr, dst, dst_len, out_cap, out_off, out_len, src_index, out_chain, hits, s);
    };
    return pktgpu_out_batch_async(ctx, kEncapEntry, queue, stream);
}

int pkt_tunnel_encap_result(pkt_ctx_t* ctx, uint64_t* bytes_out_total, uint64_t* n_out) {
    return pktgpu_out_result(ctx, kEncapEntry, bytes_out_total, n_out);
}

int pkt_tunnel_decap_batch(pkt_ctx_t* ctx, const pkt_batch_t* batch, const pkt_chain_t* chain, uint32_t which_ip,
                           uint32_t flags, const pkt_tunnel_t* tun, const uint8_t* select, uint8_t* status,
                           uint32_t* out_index, uint32_t* tunnel_out, uint8_t* dst, uint64_t dst_len, uint64_t out_cap,
                           uint64_t* out_off, uint32_t* out_len, uint32_t* src_index, const pkt_chain_t* out_chain,
                           uint64_t* hits, uint64_t* bytes_out_total, uint64_t* n_out, void* stream) {
    const auto queue = [&](hipStream_t s) {
        return tn_queue(ctx, false, batch, chain, which_ip, flags, tun, nullptr, 0, nullptr, 0, select, status, out_index,
                        tunnel_out, dst, dst_len, out_cap, out_off, out_len, src_index, out_chain, hits, s);
    };
    return pktgpu_out_batch(ctx, kDecapEntry, queue, stream, bytes_out_total, n_out);
}

int pkt_tunnel_decap_batch_async(pkt_ctx_t* ctx, const pkt_batch_t* batch, const pkt_chain_t* chain, uint32_t which_ip,
                                 uint32_t flags, const pkt_tunnel_t* tun, const uint8_t* select, uint8_t* status,
                                 uint32_t* out_index, uint32_t* tunnel_out, uint8_t* dst, uint64_t dst_len,
                                 uint64_t out_cap, uint64_t* out_off, uint32_t* out_len, uint32_t* src_index,
                                 const pkt_chain_t* out_chain, uint64_t* hits, void* stream) {
    const auto queue = [&](hipStream_t s) {
        return tn_queue(ctx, false, batch, chain, which_ip, flags, tun, nullptr, 0, nullptr, 0, select, status, out_index,
                        tunnel_out, dst, dst_len, out_cap, out_off, out_len, src_index, out_chain, hits, s);
    };
    return pktgpu_out_batch_async(ctx, kDecapEntry, queue, stream);
}

int pkt_tunnel_decap_result(pkt_ctx_t* ctx, uint64_t* bytes_out_total, uint64_t* n_out) {
    return pktgpu_out_result(ctx, kDecapEntry, bytes_out_total, n_out);
}

}  // extern "C"
