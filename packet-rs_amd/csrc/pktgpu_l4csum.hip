// pktgpu_l4csum.hip — pkt_l4_checksum_batch: the RFC 1071 checksum of every packet's TCP / UDP / ICMP segment
// with its pseudo-header, verified and (PKT_L4_UPDATE) stored, in one launch:
//   l4_kernel<UPD>   a wave owns 64 consecutive packets.  Lane p reads packet p's offset, length and chain (the
//                    first four rows up front, chain_load; later rows only when n_hdrs > 4), finds the L4 and
//                    IP slots, reads the IP header's length and fragment bytes and the stored field, decides the
//                    status and the segment [s, e) and counts the aligned 16-byte slab chunks that cover the
//                    summed span (0 for a packet that is not summed): the segment and, in front of it, the IP
//                    header's address bytes, which are the pseudo-header's (read per lane instead where a chain
//                    puts the L4 header anywhere but right behind its IP header).  A wave prefix sum of the counts goes to LDS
//                    and the wave walks the FLATTENED chunk list, 64 chunks per step and kL4Q steps' loads in
//                    flight: a lane finds its (packet, chunk) in the prefix, loads ONE aligned chunk, masks it
//                    to the bytes inside the span less the two checksum bytes, sums its eight native 16-bit
//                    words and adds them to the packet's LDS slot.  Chunks are 16-aligned, so word parity
//                    inside a chunk is address parity and no byte ever moves.  A 65535-byte packet among
//                    64-byte ones costs its bytes, not 64 times its length.  Lane p then folds its slot, swaps
//                    the bytes when the segment starts at an even address (the native words are little-endian:
//                    RFC 1071 2(B)), adds the pseudo-header, and writes the three outputs (coalesced) and,
//                    UPD, the field's two bytes.
// The read-only form (UPD = false) is compiled separately and holds no store to the slab.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pktgpu_ctx.hpp"

namespace {

constexpr uint32_t kL4Block = 256;
constexpr uint32_t kL4Waves = kL4Block / 64;
constexpr uint32_t kL4Q = 4;  // steps of 64 chunks whose loads are issued before the first use (cmp_kernel's depth)

struct LParams {
    BatchSrc src;
    uint64_t n;  // < 2^32
    const uint8_t* n_hdrs;
    const uint8_t* hdr_type;   // [PKT_MAX_HDRS][n]
    const uint16_t* hdr_off;   // [PKT_MAX_HDRS][n]
    uint16_t* calc;
    uint16_t* stored;
    uint8_t* status;
    uint32_t which;
    uint32_t keep_zero;
};

__device__ __forceinline__ bool is_l4(uint32_t t) { return t == PKT_HDR_TCP || t == PKT_HDR_UDP || t == PKT_HDR_ICMP; }

__device__ __forceinline__ uint32_t be16(const uint8_t* p) { return (uint32_t)p[0] << 8 | p[1]; }

__device__ __forceinline__ uint32_t fold16(uint32_t x) {
    x = (x & 0xFFFFu) + (x >> 16);
    return (x & 0xFFFFu) + (x >> 16);
}

// the sum of the eight 16-bit words of v's bytes [lo, hi), the bytes [f0, f1) taken as zero (all in 0..16)
__device__ __forceinline__ uint32_t chunk_sum(uint4 v, uint32_t lo, uint32_t hi, uint32_t f0, uint32_t f1) {
    const Le128 h = bytes_below(hi), l = bytes_below(lo), g1 = bytes_below(f1), g0 = bytes_below(f0);
    const uint64_t mlo = h.lo & ~l.lo & ~(g1.lo & ~g0.lo), mhi = h.hi & ~l.hi & ~(g1.hi & ~g0.hi);
    const uint32_t d0 = v.x & (uint32_t)mlo, d1 = v.y & (uint32_t)(mlo >> 32);
    const uint32_t d2 = v.z & (uint32_t)mhi, d3 = v.w & (uint32_t)(mhi >> 32);
    return (d0 & 0xFFFFu) + (d0 >> 16) + (d1 & 0xFFFFu) + (d1 >> 16) + (d2 & 0xFFFFu) + (d2 >> 16) + (d3 & 0xFFFFu) +
           (d3 >> 16);
}

template <bool UPD>
__global__ __launch_bounds__(kL4Block) void l4_kernel(LParams P) {
    __shared__ uint32_t s_pre[kL4Waves][65];  // exclusive prefix of the packets' chunk counts
    __shared__ uint64_t s_at[kL4Waves][64];   // the segment's first byte in the slab
    __shared__ uint32_t s_seg[kL4Waves][64];  // e - s | the checksum field's offset in the segment << 16
    __shared__ uint32_t s_sum[kL4Waves][64];  // the native words' sum so far (< 2^31 for 65535 bytes)
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t i = (uint64_t)blockIdx.x * kL4Block + threadIdx.x;
    const bool in = i < P.n;
    // the L4 slot and the one before it
    uint32_t l4t = 0, l4o = 0, ipt = 0, ipo = 0;
    uint64_t off = 0;
    uint32_t len = 0;
    if (in) {
        off = pkt_off(P.src, i);
        len = pkt_len(P.src, i, off);
        const ChainPre c = chain_load(P, i);
        const uint32_t nh = c.nh > PKT_MAX_HDRS ? PKT_MAX_HDRS : c.nh;
        uint32_t seen = 0, pt = 0, po = 0;
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            const bool hit = j < nh && is_l4(c.ty[j]);
            const bool take = hit && (P.which == PKT_L4_LAST || seen == P.which);
            l4t = take ? c.ty[j] : l4t;
            l4o = take ? c.of[j] : l4o;
            ipt = take ? pt : ipt;
            ipo = take ? po : ipo;
            seen += hit ? 1u : 0u;
            pt = c.ty[j];
            po = c.of[j];
        }
        for (uint32_t j = 4; j < nh; j++) {
            const uint32_t t = P.hdr_type[(uint64_t)j * P.n + i], o = P.hdr_off[(uint64_t)j * P.n + i];
            if (is_l4(t)) {
                if (P.which == PKT_L4_LAST || seen == P.which) {
                    l4t = t;
                    l4o = o;
                    ipt = pt;
                    ipo = po;
                }
                seen++;
            }
            pt = t;
            po = o;
        }
    }
    // the status, the segment and the pseudo-header's sum (big-endian words)
    uint32_t st = PKT_L4_ABSENT, seg = 0, fo = 0, ph = 0, sv = 0, chunks = 0;
    const uint8_t* pkt = P.src.slab + off;
    const bool v4 = ipt == PKT_HDR_IPV4;
    if (l4t) {
        if (!v4 && ipt != PKT_HDR_IPV6) {
            st = PKT_L4_NO_IP;
        } else if (ipo + (v4 ? 20u : 40u) > len) {
            st = PKT_L4_SPAN;
        } else if (v4 && (be16(pkt + ipo + 6) & 0x3FFFu)) {
            st = PKT_L4_FRAGMENT;
        } else {
            const uint32_t e = v4 ? ipo + be16(pkt + ipo + 2) : ipo + 40u + be16(pkt + ipo + 4);
            const uint32_t hs = l4t == PKT_HDR_TCP ? 20u : l4t == PKT_HDR_UDP ? 8u : 4u;
            if (e > len || e < l4o + hs) {
                st = PKT_L4_SPAN;
            } else {
                st = PKT_L4_OK;  // OK, BAD or UNCHECKED: decided once the sum is known
                seg = e - l4o;   // >= hs: the field's two bytes lie inside the segment, and it inside the packet
                                 // (l4o, seg, fo: from here on the SUMMED span, which may start at the addresses)
                fo = l4t == PKT_HDR_TCP ? 16u : l4t == PKT_HDR_UDP ? 6u : 2u;
                sv = be16(pkt + l4o + fo);
                if (!v4 || l4t != PKT_HDR_ICMP) {
                    // The pseudo-header: length and protocol here.  The addresses are the IP header's last 8 / 32
                    // bytes: where the L4 header follows it at once (every parse's chain) they are summed by
                    // the walk, as bytes in front of the segment (an even count: the words' parity holds);
                    // a chain that puts the L4 header elsewhere has them read here.
                    ph = seg + (l4t == PKT_HDR_TCP ? 6u : l4t == PKT_HDR_UDP ? 17u : 58u);
                    const uint32_t a0 = v4 ? 12u : 8u, a1 = v4 ? 20u : 40u;
                    if (l4o == ipo + a1) {
                        l4o -= a1 - a0;
                        seg += a1 - a0;
                        fo += a1 - a0;
                    } else {
                        for (uint32_t k = a0; k < a1; k += 2) ph += be16(pkt + ipo + k);
                    }
                }
                const uint64_t S = off + l4o;
                chunks = (uint32_t)(((S + seg + 15) >> 4) - (S >> 4));
            }
        }
    }
    const uint32_t incl = wave_incl_scan(chunks, lane);
    if (lane == 0) s_pre[wv][0] = 0;
    s_pre[wv][lane + 1] = incl;
    s_at[wv][lane] = off + l4o;
    s_seg[wv][lane] = seg | fo << 16;
    s_sum[wv][lane] = 0;
    wave_sync();
    const uint32_t total = __builtin_amdgcn_readfirstlane(s_pre[wv][64]);  // <= 64 * 4097
    const FlatWalk walk = flat_walk(chunks);
    for (uint32_t base = 0; base < total; base += 64u * kL4Q) {  // uniform
        uint4 v[kL4Q];
        uint32_t pr[kL4Q], lo[kL4Q], hi[kL4Q], f0[kL4Q], f1[kL4Q];
#pragma unroll
        for (uint32_t q = 0; q < kL4Q; q++) {
            const uint32_t f = base + 64u * q + lane;
            pr[q] = 64;  // no chunk
            lo[q] = hi[q] = f0[q] = f1[q] = 0;
            v[q] = make_uint4(0, 0, 0, 0);
            if (f >= total) continue;
            const FlatAt at = locate(walk, s_pre[wv], f);
            const uint32_t p = at.p;
            // Chunk k of the segment's aligned chunks: it holds at least one byte of [S, S + seg), which lies
            // inside the slab, so it is at or below the slab's last aligned chunk.
            const uint64_t S = s_at[wv][p], A = (S & ~(uint64_t)15) + 16ull * at.k;
            const uint32_t sg = s_seg[wv][p];
            const int64_t b = (int64_t)(S - A), e = b + (sg & 0xFFFFu), g = b + (sg >> 16);  // relative to the chunk
            pr[q] = p;
            lo[q] = b < 0 ? 0u : (uint32_t)b;                  // b <= 15
            hi[q] = e > 16 ? 16u : (uint32_t)e;                // e >= 1
            f0[q] = g < 0 ? 0u : g > 16 ? 16u : (uint32_t)g;   // the checksum field's bytes [g, g + 2)
            f1[q] = g + 2 < 0 ? 0u : g + 2 > 16 ? 16u : (uint32_t)(g + 2);
            v[q] = *reinterpret_cast<const uint4*>(P.src.slab + A);
        }
#pragma unroll
        for (uint32_t q = 0; q < kL4Q; q++) {
            if (pr[q] >= 64) continue;
            const uint32_t part = chunk_sum(v[q], lo[q], hi[q], f0[q], f1[q]);
            if (part) atomicAdd(&s_sum[wv][pr[q]], part);
        }
    }
    wave_sync();
    uint32_t c = 0;
    if (st == PKT_L4_OK) {
        // The slot holds the sum of the words as the machine reads them, low byte first.  A segment that starts
        // at an odd address has its big-endian high bytes in the native words' high bytes already; at an even
        // address the two are swapped, and so is the folded sum (RFC 1071 2(B)).
        uint32_t x = fold16(s_sum[wv][lane]);
        if (((off + l4o) & 1u) == 0) x = (x >> 8 | x << 8) & 0xFFFFu;
        c = ~fold16(x + ph) & 0xFFFFu;
        const bool udp = l4t == PKT_HDR_UDP;
        if (udp && c == 0) c = 0xFFFFu;
        if (udp && sv == 0)
            st = v4 ? PKT_L4_UNCHECKED : PKT_L4_BAD;
        else
            st = sv == c || (sv == 0xFFFFu && c == 0) ? PKT_L4_OK : PKT_L4_BAD;
        if (UPD && !(st == PKT_L4_UNCHECKED && P.keep_zero)) {
            uint8_t* w = const_cast<uint8_t*>(pkt) + l4o + fo;
            if (((uintptr_t)w & 1u) == 0) {  // one 16-bit store where the field is aligned
                *reinterpret_cast<uint16_t*>(w) = (uint16_t)(c >> 8 | c << 8);
            } else {
                w[0] = (uint8_t)(c >> 8);
                w[1] = (uint8_t)c;
            }
        }
    }
    if (in) {
        if (P.calc) P.calc[i] = (uint16_t)c;
        if (P.stored) P.stored[i] = (uint16_t)sv;
        if (P.status) P.status[i] = (uint8_t)st;
    }
}

}  // namespace

extern "C" int pkt_l4_checksum_batch(pkt_ctx_t* ctx, const pkt_batch_t* b, const pkt_chain_t* chain, uint32_t which,
                                     uint32_t flags, uint16_t* calc, uint16_t* stored, uint8_t* l4_status, void* stream) {
    if (!ctx || !b || !chain) return fail(ctx, PKT_ERR_INVALID_ARG, "null argument");
    if (b->n >= (1ull << 32)) return fail(ctx, PKT_ERR_INVALID_ARG, "pkt_l4_checksum_batch: n >= 2^32");
    if (flags & ~(PKT_L4_UPDATE | PKT_L4_KEEP_ZERO_UDP)) return fail(ctx, PKT_ERR_INVALID_ARG, "pkt_l4_checksum_batch: unknown flag bits");
    if ((flags & PKT_L4_KEEP_ZERO_UDP) && !(flags & PKT_L4_UPDATE))
        return fail(ctx, PKT_ERR_INVALID_ARG, "pkt_l4_checksum_batch: KEEP_ZERO_UDP without UPDATE");
    if (which >= PKT_MAX_HDRS && which != PKT_L4_LAST)
        return fail(ctx, PKT_ERR_INVALID_ARG, "pkt_l4_checksum_batch: which is neither below 16 nor PKT_L4_LAST");
    if (b->n == 0) return PKT_SUCCESS;
    if (!chain->n_hdrs || !chain->hdr_type || !chain->hdr_off)
        return fail(ctx, PKT_ERR_INVALID_ARG, "pkt_l4_checksum_batch: null chain column");
    int rc = check_batch_slab16(ctx, b);
    if (rc == PKT_SUCCESS) rc = check_batch_index(ctx, b);
    if (rc != PKT_SUCCESS) return rc;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    LParams P{};
    P.src = batch_src(b);
    P.n = b->n;
    P.n_hdrs = chain->n_hdrs;
    P.hdr_type = chain->hdr_type;
    P.hdr_off = chain->hdr_off;
    P.calc = calc;
    P.stored = stored;
    P.status = l4_status;
    P.which = which;
    P.keep_zero = flags & PKT_L4_KEEP_ZERO_UDP;
    const dim3 grid((unsigned)((b->n + kL4Block - 1) / kL4Block));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (flags & PKT_L4_UPDATE)
        hipLaunchKernelGGL(l4_kernel<true>, grid, dim3(kL4Block), 0, s, P);
    else
        hipLaunchKernelGGL(l4_kernel<false>, grid, dim3(kL4Block), 0, s, P);
    if ((e = hipGetLastError()) != hipSuccess) return hip_fail(ctx, e, "l4 checksum launch");
    return PKT_SUCCESS;
}
