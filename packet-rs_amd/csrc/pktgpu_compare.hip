// pktgpu_compare.hip — pkt_compare_batch: Packet::compare (packet.rs:326-358) of packet i of batch a
// against packet i of batch b, for every i, in two launches:
//   cmp_kernel<IGN>   a wave owns 64 consecutive pairs.  Lane p reads pair p's offsets and lengths
//                     (m = the common length, chunks = ceil(m / 16)) and, with ignores, resolves every
//                     spec against its chain into a packet-relative bit range in LDS.  A wave prefix sum
//                     of the chunk counts goes to LDS and the wave walks the FLATTENED chunk list, 64
//                     chunks per step and kCmpQ steps' loads in flight: a lane finds its (pair, chunk) in
//                     the prefix, builds its 16 packet-relative bytes of a and of b from two aligned
//                     16-byte loads each (the two sides differ in alignment), and adds the
//                     chunk's matching bytes / takes the minimum of its first differing byte in the
//                     pair's LDS slot.  A 65535-byte pair among 64-byte ones costs its bytes, not 64
//                     times its length.  Lane p then writes pair p's three outputs (coalesced) and the
//                     block adds its counts to one of 256 slots of four device words (three adds and
//                     one max per block; one slot for every block costs 30 us of queueing at the L2).
//   cmp_fin_kernel    one block: the slots summed to the ctx's pinned words, and back to zero.
// The nignore == 0 case is compiled separately (IGN = false) and pays nothing for the masks.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pktgpu_ctx.hpp"

namespace {

constexpr uint32_t kCmpBlock = 256;
constexpr uint32_t kCmpWaves = kCmpBlock / 64;
constexpr uint32_t kCmpQ = 4;          // steps of 64 chunks whose loads are issued before the first use
constexpr uint32_t kCmpMaxIgnore = 16;
constexpr uint32_t kCmpSlots = 256;     // summary slots the blocks spread their atomics over
constexpr uint32_t kCmpSlotWords = 16;  // a slot: [n_equal, n_len, n_bytes, ~first_bad] on 128 bytes of its own

struct CParams {
    BatchSrc a, b;
    uint64_t n;  // < 2^32
    const uint8_t* n_hdrs;
    const uint8_t* hdr_type;   // [PKT_MAX_HDRS][n]
    const uint16_t* hdr_off;   // [PKT_MAX_HDRS][n]
    uint8_t* result;
    uint32_t* matching;
    uint32_t* first_diff;
    uint64_t* acc;  // [kCmpSlots][kCmpSlotWords]
    uint32_t nignore;
    pkt_field_spec_t ign[kCmpMaxIgnore];
};

// bit 7 of every byte of x that is not zero
__device__ __forceinline__ uint32_t nonzero_bytes(uint32_t x) {
    return (((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;
}

// The ignore ranges of a wave's pairs: [spec][64] first and last ignored bit, packet-relative (first >
// last: nothing).  Dynamic LDS, sized by nignore: [kCmpWaves][nignore][2][64] words.
extern __shared__ uint32_t s_ign[];

template <bool IGN>
__global__ __launch_bounds__(kCmpBlock) void cmp_kernel(CParams P) {
    __shared__ uint32_t s_pre[kCmpWaves][65];   // exclusive prefix of the pairs' chunk counts
    __shared__ uint64_t s_ao[kCmpWaves][64], s_bo[kCmpWaves][64];
    __shared__ uint32_t s_m[kCmpWaves][64];
    __shared__ uint32_t s_cnt[kCmpWaves][64];   // matching bytes so far
    __shared__ uint32_t s_fd[kCmpWaves][64];    // lowest differing byte so far
    __shared__ unsigned long long s_sum[4];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t i = (uint64_t)blockIdx.x * kCmpBlock + threadIdx.x;
    const bool in = i < P.n;
    if (threadIdx.x < 4) s_sum[threadIdx.x] = threadIdx.x == 3 ? ~0ull : 0ull;
    uint64_t ao = 0, bo = 0;
    uint32_t la = 0, lb = 0;
    if (in) {
        ao = pkt_off(P.a, i);
        bo = pkt_off(P.b, i);
        la = pkt_len(P.a, i, ao);
        lb = pkt_len(P.b, i, bo);
    }
    const uint32_t m = la < lb ? la : lb;
    const uint32_t chunks = (m + 15u) >> 4;
    const uint32_t incl = wave_incl_scan(chunks, lane);
    if (lane == 0) s_pre[wv][0] = 0;
    s_pre[wv][lane + 1] = incl;
    s_ao[wv][lane] = ao;
    s_bo[wv][lane] = bo;
    s_m[wv][lane] = m;
    s_cnt[wv][lane] = 0;
    s_fd[wv][lane] = m;
    uint32_t* ig = nullptr;
    if (IGN) {
        // lane p resolves every spec against its own chain (slot-major, coalesced reads): the chain's
        // first four slots in registers, later ones read again per spec
        ig = s_ign + (size_t)wv * P.nignore * 128u;
        uint32_t nh = in ? P.n_hdrs[i] : 0;
        nh = nh > PKT_MAX_HDRS ? PKT_MAX_HDRS : nh;
        uint32_t ty[4], ho[4];
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            ty[j] = j < nh ? P.hdr_type[(uint64_t)j * P.n + i] : 0u;
            ho[j] = j < nh ? P.hdr_off[(uint64_t)j * P.n + i] : 0u;
        }
        for (uint32_t s = 0; s < P.nignore; s++) {  // uniform
            const uint32_t type = P.ign[s].hdr_type, occ = P.ign[s].occurrence;
            uint32_t seen = 0, at = ~0u;
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) {
                const bool hit = j < nh && ty[j] == type;
                at = hit && seen == occ ? ho[j] : at;
                seen += hit ? 1u : 0u;
            }
            for (uint32_t j = 4; j < nh; j++) {
                if (P.hdr_type[(uint64_t)j * P.n + i] != type) continue;
                if (seen++ == occ) at = P.hdr_off[(uint64_t)j * P.n + i];
            }
            ig[s * 128u + lane] = at != ~0u ? 8u * at + P.ign[s].start : 1u;
            ig[s * 128u + 64u + lane] = at != ~0u ? 8u * at + P.ign[s].end : 0u;
        }
    }
    __syncthreads();  // (also orders s_sum's first values before the atomics at the end)
    const uint32_t total = __builtin_amdgcn_readfirstlane(s_pre[wv][64]);  // <= 64 * 4096
    const FlatWalk walk = flat_walk(chunks);
    // an aligned chunk at or past the slab's last one is not loaded again: its bytes are not needed
    const uint64_t a_last = P.a.slab_len ? ((P.a.slab_len + 15) & ~(uint64_t)15) - 16 : 0;
    const uint64_t b_last = P.b.slab_len ? ((P.b.slab_len + 15) & ~(uint64_t)15) - 16 : 0;
    for (uint32_t base = 0; base < total; base += 64u * kCmpQ) {  // uniform
        uint4 a0[kCmpQ], a1[kCmpQ], b0[kCmpQ], b1[kCmpQ];
        uint32_t pr[kCmpQ], ck[kCmpQ], sha[kCmpQ], shb[kCmpQ];
#pragma unroll
        for (uint32_t q = 0; q < kCmpQ; q++) {
            const uint32_t f = base + 64u * q + lane;
            pr[q] = 64;  // no chunk
            ck[q] = sha[q] = shb[q] = 0;
            a0[q] = a1[q] = b0[q] = b1[q] = make_uint4(0, 0, 0, 0);
            if (f >= total) continue;
            const FlatAt at = locate(walk, s_pre[wv], f);
            const uint32_t p = at.p, k = at.k;
            pr[q] = p;
            ck[q] = k;
            // Bytes [16 k, min(16 k + 16, m)) of both packets lie inside their slabs, so the first aligned
            // chunk is at or below the slab's last one; the second is needed only when it is too, and is
            // the first one again (a load that is not used) when the first is the slab's last.
            const uint64_t A = s_ao[wv][p] + 16u * k, B = s_bo[wv][p] + 16u * k;
            const uint64_t A0 = A & ~(uint64_t)15, B0 = B & ~(uint64_t)15;
            sha[q] = (uint32_t)A & 15u;
            shb[q] = (uint32_t)B & 15u;
            a0[q] = *reinterpret_cast<const uint4*>(P.a.slab + A0);
            a1[q] = *reinterpret_cast<const uint4*>(P.a.slab + A0 + (A0 >= a_last ? 0u : 16u));
            b0[q] = *reinterpret_cast<const uint4*>(P.b.slab + B0);
            b1[q] = *reinterpret_cast<const uint4*>(P.b.slab + B0 + (B0 >= b_last ? 0u : 16u));
        }
#pragma unroll
        for (uint32_t q = 0; q < kCmpQ; q++) {
            const uint32_t p = pr[q], k = ck[q];
            if (p >= 64) continue;
            uint32_t va[4], vb[4], d[4];
            take16(a0[q], a1[q], sha[q], va);
            take16(b0[q], b1[q], shb[q], vb);
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) d[j] = va[j] ^ vb[j];
            const uint32_t left = s_m[wv][p] - 16u * k;  // >= 1
            const uint32_t valid = left > 16u ? 16u : left;
            if (IGN && (d[0] | d[1] | d[2] | d[3])) {  // a chunk without a difference needs no mask
                // the ranges that touch the chunk's bits [128 k, 128 k + 127], MSB-first: bit t of the
                // chunk is bit 127 - t of a 128-bit word, whose bytes are then reversed into memory order
                const uint32_t c0 = 128u * k;
                Le128 g{0, 0};
                for (uint32_t s = 0; s < P.nignore; s++) {
                    const uint32_t lo = ig[s * 128u + p], hi = ig[s * 128u + 64u + p];
                    if (lo > hi || hi < c0 || lo > c0 + 127u) continue;
                    const uint32_t l = lo > c0 ? lo - c0 : 0u, h = hi < c0 + 127u ? hi - c0 : 127u;
                    const Le128 up = bits_below(128u - l), dn = bits_below(127u - h);
                    g.lo |= up.lo & ~dn.lo;
                    g.hi |= up.hi & ~dn.hi;
                }
                const uint64_t glo = __builtin_bswap64(g.hi), ghi = __builtin_bswap64(g.lo);
                d[0] &= ~(uint32_t)glo;
                d[1] &= ~(uint32_t)(glo >> 32);
                d[2] &= ~(uint32_t)ghi;
                d[3] &= ~(uint32_t)(ghi >> 32);
            }
            // z: bit 8 i + j = byte i of dword j (the chunk's byte 4 j + i) differs; vz: the same bits of
            // the chunk's first `valid` bytes (jf whole dwords, then rem bytes of dword jf)
            const uint32_t y0 = nonzero_bytes(d[0]), y1 = nonzero_bytes(d[1]), y2 = nonzero_bytes(d[2]), y3 = nonzero_bytes(d[3]);
            const uint32_t z = y0 >> 7 | y1 >> 6 | y2 >> 5 | y3 >> 4;
            const uint32_t jf = valid >> 2, rem = valid & 3u;
            const uint32_t vz = ((1u << jf) - 1u) * 0x01010101u | (0x00010101u & ((1u << (8u * rem)) - 1u)) << jf;
            const uint32_t bad = (uint32_t)__builtin_popcount(z & vz);
            atomicAdd(&s_cnt[wv][p], valid - bad);
            if (bad) {
                // the lowest differing byte of all 16: below `valid`, since one of the valid bytes differs
                const uint32_t ys = y0 ? y0 : y1 ? y1 : y2 ? y2 : y3;
                const uint32_t js = y0 ? 0u : y1 ? 4u : y2 ? 8u : 12u;
                atomicMin(&s_fd[wv][p], 16u * k + js + ((uint32_t)__builtin_ctz(ys) >> 3));
            }
        }
    }
    wave_sync();
    const uint32_t cnt = s_cnt[wv][lane];
    const uint32_t res = la != lb ? PKT_CMP_LEN : cnt != la ? PKT_CMP_BYTES : PKT_CMP_EQUAL;
    if (in) {
        if (P.result) P.result[i] = (uint8_t)res;
        if (P.matching) P.matching[i] = cnt;
        if (P.first_diff) P.first_diff[i] = s_fd[wv][lane];
    }
    // the summary: ballots per wave, one LDS atomic per wave and word, one device atomic per block and word
    const uint64_t e = __ballot(in && res == PKT_CMP_EQUAL), l = __ballot(in && res == PKT_CMP_LEN);
    const uint64_t y = __ballot(in && res == PKT_CMP_BYTES);
    if (lane == 0) {
        if (e) atomicAdd(&s_sum[0], (unsigned long long)__builtin_popcountll(e));
        if (l) atomicAdd(&s_sum[1], (unsigned long long)__builtin_popcountll(l));
        if (y) atomicAdd(&s_sum[2], (unsigned long long)__builtin_popcountll(y));
        if (l | y)
            atomicMin(&s_sum[3], (unsigned long long)((uint64_t)blockIdx.x * kCmpBlock + 64u * wv +
                                                      (uint32_t)__builtin_ctzll(l | y)));
    }
    __syncthreads();
    // Atomics of every block on one address take their turn at the L2 (4096 blocks: 30 us, measured), so
    // a block adds to one of kCmpSlots slots, each on a line of its own.  The lowest bad index is kept as
    // the maximum of its complement: every word rests at 0.
    unsigned long long* slot = reinterpret_cast<unsigned long long*>(P.acc) + (blockIdx.x % kCmpSlots) * kCmpSlotWords;
    if (threadIdx.x < 3 && s_sum[threadIdx.x]) atomicAdd(slot + threadIdx.x, s_sum[threadIdx.x]);
    if (threadIdx.x == 3 && s_sum[3] != ~0ull) atomicMax(slot + 3, ~s_sum[3]);
}

// One block of kCmpSlots threads: the slots' sums to the host's pinned words (first_bad: ~0 = none, the
// host makes it n), and every slot back to 0 for the next call.
__global__ __launch_bounds__(kCmpSlots) void cmp_fin_kernel(uint64_t* __restrict__ acc, uint64_t* __restrict__ host) {
    __shared__ uint64_t s_part[kCmpSlots / 64][4];
    uint64_t v[4];
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
        v[k] = acc[threadIdx.x * kCmpSlotWords + k];
        acc[threadIdx.x * kCmpSlotWords + k] = 0;
    }
#pragma unroll
    for (uint32_t d = 32; d; d >>= 1) {
#pragma unroll
        for (uint32_t k = 0; k < 3; k++) v[k] += __shfl_xor(v[k], d, 64);
        const uint64_t o = __shfl_xor(v[3], d, 64);
        v[3] = o > v[3] ? o : v[3];
    }
    if ((threadIdx.x & 63u) == 0) {
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) s_part[threadIdx.x >> 6][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        uint64_t r = 0;
        for (uint32_t w = 0; w < kCmpSlots / 64; w++) {
            const uint64_t x = s_part[w][threadIdx.x];
            r = threadIdx.x < 3 ? r + x : (x > r ? x : r);
        }
        host[threadIdx.x] = threadIdx.x < 3 ? r : (r ? ~r : ~0ull);
    }
}

int side(pkt_ctx_t* ctx, const pkt_batch_t* b, BatchSrc& s) {
    s = batch_src(b);
    if (!b->n) return PKT_SUCCESS;
    const int rc = check_batch_slab16(ctx, b);
    return rc != PKT_SUCCESS ? rc : check_batch_index(ctx, b);
}

// The two launches, queued on s.  The summary arrives in ctx->cmp.ctl once the stream has passed them.
int cmp_queue(pkt_ctx_t* ctx, const pkt_batch_t* a, const pkt_batch_t* b, const pkt_chain_t* chain,
              const pkt_field_spec_t* ignore, uint32_t nignore, uint8_t* result, uint32_t* matching,
              uint32_t* first_diff, hipStream_t s) {
    if (!ctx || !a || !b) return fail(ctx, PKT_ERR_INVALID_ARG, "null argument");
    if (a->n != b->n) return fail(ctx, PKT_ERR_INVALID_ARG, "pkt_compare_batch: the batches differ in n");
    if (a->n >= (1ull << 32)) return fail(ctx, PKT_ERR_INVALID_ARG, "pkt_compare_batch: n >= 2^32");
    if (nignore > kCmpMaxIgnore) return fail(ctx, PKT_ERR_INVALID_ARG, "pkt_compare_batch: more than 16 ignores");
    if (nignore && (!ignore || !chain || !chain->n_hdrs || !chain->hdr_type || !chain->hdr_off))
        return fail(ctx, PKT_ERR_INVALID_ARG, "pkt_compare_batch: ignores without specs or chain columns");
    for (uint32_t k = 0; k < nignore; k++)
        if (ignore[k].end < ignore[k].start) return fail(ctx, PKT_ERR_INVALID_ARG, "pkt_compare_batch: a spec with end < start");
    CParams P{};
    int rc = side(ctx, a, P.a);
    if (rc == PKT_SUCCESS) rc = side(ctx, b, P.b);
    if (rc != PKT_SUCCESS) return rc;
    CompareScratch& c = ctx->cmp;
    if (c.pending)
        return fail(ctx, PKT_ERR_INVALID_ARG, "a queued compare's result has not been taken on this ctx (pkt_compare_result)");
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    if ((e = c.ensure(64)) != hipSuccess) return hip_fail(ctx, e, "hipHostMalloc (compare)");
    if (!c.acc) {
        const size_t bytes = (size_t)kCmpSlots * kCmpSlotWords * sizeof(uint64_t);
        if ((e = hipMalloc(reinterpret_cast<void**>(&c.acc), bytes)) != hipSuccess) return hip_fail(ctx, e, "hipMalloc (compare)");
        if ((e = hipMemset(c.acc, 0, bytes)) != hipSuccess) {
            (void)hipFree(c.acc);
            c.acc = nullptr;
            return hip_fail(ctx, e, "hipMemset (compare)");
        }
    }
    c.n = a->n;
    c.ctl[0] = c.ctl[1] = c.ctl[2] = 0;
    c.ctl[3] = ~0ull;
    if (a->n == 0) return PKT_SUCCESS;
    P.n = a->n;
    if (nignore) {
        P.n_hdrs = chain->n_hdrs;
        P.hdr_type = chain->hdr_type;
        P.hdr_off = chain->hdr_off;
        for (uint32_t k = 0; k < nignore; k++) P.ign[k] = ignore[k];
    }
    P.nignore = nignore;
    P.result = result;
    P.matching = matching;
    P.first_diff = first_diff;
    P.acc = c.acc;
    const dim3 grid((unsigned)((a->n + kCmpBlock - 1) / kCmpBlock));
    if (nignore)
        hipLaunchKernelGGL(cmp_kernel<true>, grid, dim3(kCmpBlock), kCmpWaves * nignore * 128u * sizeof(uint32_t), s, P);
    else
        hipLaunchKernelGGL(cmp_kernel<false>, grid, dim3(kCmpBlock), 0, s, P);
    hipLaunchKernelGGL(cmp_fin_kernel, dim3(1), dim3(kCmpSlots), 0, s, c.acc, c.ctl_dev);
    if ((e = hipGetLastError()) != hipSuccess) return hip_fail(ctx, e, "compare launch");
    return PKT_SUCCESS;
}

// The outcome of the last cmp_queue (the stream has passed it).
void cmp_finish(pkt_ctx_t* ctx, pkt_cmp_summary_t* summary) {
    const CompareScratch& c = ctx->cmp;
    if (!summary) return;
    summary->n_equal = c.ctl[0];
    summary->n_len = c.ctl[1];
    summary->n_bytes = c.ctl[2];
    summary->first_bad = c.ctl[3] == ~0ull ? c.n : c.ctl[3];
}

}  // namespace

extern "C" {

int pkt_compare_batch(pkt_ctx_t* ctx, const pkt_batch_t* a, const pkt_batch_t* b, const pkt_chain_t* chain_a,
                      const pkt_field_spec_t* ignore, uint32_t nignore, uint8_t* result, uint32_t* matching,
                      uint32_t* first_diff, pkt_cmp_summary_t* summary, void* stream) {
    if (summary) *summary = pkt_cmp_summary_t{0, 0, 0, 0};
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int rc = cmp_queue(ctx, a, b, chain_a, ignore, nignore, result, matching, first_diff, s);
    if (rc != PKT_SUCCESS) return rc;
    if (a->n) {
        const hipError_t e = hipStreamSynchronize(s);  // the one host wait, for the summary
        if (e != hipSuccess) return hip_fail(ctx, e, "pkt_compare_batch");
    }
    cmp_finish(ctx, summary);
    return PKT_SUCCESS;
}

int pkt_compare_batch_async(pkt_ctx_t* ctx, const pkt_batch_t* a, const pkt_batch_t* b, const pkt_chain_t* chain_a,
                            const pkt_field_spec_t* ignore, uint32_t nignore, uint8_t* result, uint32_t* matching,
                            uint32_t* first_diff, void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int rc = cmp_queue(ctx, a, b, chain_a, ignore, nignore, result, matching, first_diff, s);
    if (rc != PKT_SUCCESS) return rc;
    ctx->cmp.mark(s);
    return PKT_SUCCESS;
}

int pkt_compare_result(pkt_ctx_t* ctx, pkt_cmp_summary_t* summary) {
    if (summary) *summary = pkt_cmp_summary_t{0, 0, 0, 0};
    if (!ctx) return PKT_ERR_INVALID_ARG;
    CompareScratch& c = ctx->cmp;
    if (!c.pending) return fail(ctx, PKT_ERR_INVALID_ARG, "no compare queued on this ctx");
    const hipError_t e = c.take();
    if (e != hipSuccess) return hip_fail(ctx, e, "pkt_compare_result");
    cmp_finish(ctx, summary);
    return PKT_SUCCESS;
}

}  // extern "C"
