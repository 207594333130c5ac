// pktgpu_match.hip — pkt_match_create / _destroy / _batch: first-match rule tables over a parsed batch.
//   match_kernel<NCH>  a lane owns a packet, a block 256 of them.  Prologue as extract_kernel's (pktgpu_rewrite.hip):
//                      the wave's windows (the packets' first NCH aligned 16-byte chunks) loaded cooperatively
//                      into LDS at an odd dword stride, chain_load and the compiled program's loads issued with
//                      them, one barrier.  The program (pktgpu_match.hpp) is uniform across the wave: its terms are
//                      read from the read-only device buffer at uniform addresses (scalar loads, 32 bytes a term,
//                      through the scalar cache: no vector-memory round trip per packet), its rules and header
//                      references from LDS (a lane reads its own rule's action).  Each of the program's first
//                      kRefLds distinct (hdr_type, occurrence) references is resolved once per packet into an
//                      LDS column (0xFFFF = absent or not wholly inside the packet); later ones when a term
//                      first names them.  Rules in order,
//                      terms in the compiled order; a rule stops at the term after which no lane of the wave still
//                      holds, and without `matched` the wave stops at the first rule by which every active lane
//                      has matched.  Fields past the window come from global memory (PacketView::le: aligned
//                      dwords clamped to round_up(slab_len, 16)); only bytes of a header that lies wholly inside
//                      the packet are ever interpreted.  Counters: a wave's lanes with the same first rule add
//                      once to the block's LDS counters (its first four groups; the rest a lane at a time), and
//                      after a barrier thread r adds rule r's non-zero count and bytes to the caller's arrays
//                      with one agent-scope vector atomic each.  No lane waits for another.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "pktgpu_ctx.hpp"
#include "pktgpu_device.hpp"
#include "pktgpu_match.hpp"

using namespace pktgpu;

struct pkt_match {
    pkt_ctx* ctx;
    int device;
    MatchCompiled* prog;  // device
    uint32_t nterms, nrules, nrefs, default_action;
};

namespace {

constexpr uint32_t kMBlock = 256;
constexpr uint32_t kRefLds = 16;     // header references resolved up front into LDS
constexpr uint32_t kAbsent = 0xFFFFu;
constexpr uint32_t kWaveGroups = 4;  // distinct first rules a wave adds for as groups
// A launch that counts with a small program is bound by the counters' adds (4096 blocks adding to the same line:
// + 40 us per 2^20 packets), so its grid is capped and a block loops over tiles; a program of many terms hides
// the adds behind its arithmetic and loses more to the coarser tail of looping blocks, so it keeps one tile a
// block (one run, 2^20 packets, all outputs: 1 term 58.9 -> 31.4 us; 16 x 5 terms 169.1 -> 180.8 us, 64 x 4
// 401.2 -> 438.7 us; profiles/ab/match_count_grid.txt).  Only those three programs (1, 80 and 256 compiled terms)
// were measured: kLoopMaxTerms lies between the first two and was not searched, and kCountBlocks is the number
// of blocks resident at once (LDS allows 5 a CU), not a measured optimum.
constexpr uint32_t kCountBlocks = 1280;   // 5 blocks a CU on 256 CUs
constexpr uint32_t kLoopMaxTerms = 16;

struct MParams {
    BatchSrc src;
    uint64_t n;  // < 2^32
    const uint8_t* n_hdrs;
    const uint8_t* hdr_type;   // [PKT_MAX_HDRS][n]
    const uint16_t* hdr_off;   // [PKT_MAX_HDRS][n]
    const MatchCompiled* prog;
    uint32_t nterms, nrules, nrefs, default_action;
    uint8_t* rule;
    uint32_t* action;
    uint8_t* select;
    uint64_t* matched;
    uint64_t* hits;
    uint64_t* bytes;
};

__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// offset of the occurrence-th header of `type` in packet i's chain, or -1: the first 4 slots from registers
// (find_pre's selects, pktgpu_rewrite.hip), deeper ones from the chain columns.  (The selects are written here a
// second time: with them in a helper of pktgpu_batch.hpp that find_pre calls too, extract_kernel's and
// set_fields_kernel's listings came out different (registers, operand order, two instructions), and those
// kernels are kept as they were measured.)
__device__ __forceinline__ int32_t find_hdr(const ChainPre& c, const MParams& P, uint64_t i, uint32_t nh, uint32_t type,
                                            uint32_t occ) {
    int32_t r = -1;
    uint32_t cnt = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) {
        const bool m = j < nh && c.ty[j] == type;
        r = (m && cnt == occ && r < 0) ? (int32_t)c.of[j] : r;
        cnt += m ? 1u : 0u;
    }
    if (r < 0 && nh > 4) {
        for (uint32_t j = 4; j < nh; j++) {
            if (P.hdr_type[(uint64_t)j * P.n + i] != type) continue;
            if (cnt == occ) return (int32_t)P.hdr_off[(uint64_t)j * P.n + i];
            cnt++;
        }
    }
    return r;
}

template <int NCH>
__global__ __launch_bounds__(kMBlock) void match_kernel(MParams P, const uint4* __restrict__ gt) {
    constexpr uint32_t kStride = 4 * NCH + 1;  // dwords
    __shared__ uint32_t win[kMBlock * kStride];
    __shared__ __align__(8) pkt_match_rule_t s_rules[PKT_MATCH_MAX_RULES];
    __shared__ MatchRef s_refs[PKT_MATCH_MAX_TERMS];
    __shared__ uint16_t s_ho[kRefLds][kMBlock];
    __shared__ uint32_t s_hits[PKT_MATCH_MAX_RULES + 1];
    __shared__ unsigned long long s_bytes[PKT_MATCH_MAX_RULES + 1];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave0 = t & ~63u;
    // ---- the program's rules and references into LDS, the block's counters zeroed
    // (gt = the program's terms, read below at uniform addresses; a kernel argument of its own so that it can
    // be __restrict__: the tile loop's output stores then do not stop the compiler from using scalar loads)
    uint2 pr = make_uint2(0, 0);
    uint32_t pf = 0;
    if (t < P.nrules) pr = reinterpret_cast<const uint2*>(P.prog->rules)[t];
    if (t < P.nrefs) pf = reinterpret_cast<const uint32_t*>(P.prog->refs)[t];
    if (t < P.nrules) reinterpret_cast<uint2*>(s_rules)[t] = pr;
    if (t < P.nrefs) reinterpret_cast<uint32_t*>(s_refs)[t] = pf;
    if (t <= PKT_MATCH_MAX_RULES) {
        s_hits[t] = 0;
        s_bytes[t] = 0;
    }
    const bool counting = P.hits || P.bytes;  // uniform over the grid
    const uint64_t up = (P.src.slab_len + 15) & ~(uint64_t)15;
    const uint64_t last16 = up ? up - 16 : 0;
    // A block takes the tiles of 256 packets blockIdx.x, blockIdx.x + gridDim.x, ..: one tile, or several where
    // the launch caps the grid (kCountBlocks), so that the counters cost one add per block, rule and counter.
    const uint32_t ntiles = (uint32_t)((P.n + kMBlock - 1) / kMBlock);
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {  // uniform
    const uint64_t i = (uint64_t)tile * kMBlock + t;
    const bool act = i < P.n;  // no early exit: the wave loads its windows together
    uint64_t off = 0;
    uint32_t len = 0;
    if (act) {
        off = pkt_off(P.src, i);
        len = pkt_len(P.src, i, off);
    }
    // ---- every load first: the windows (pair 64k + lane in load k, as extract_kernel) and the chain
    uint4 v[NCH];
#pragma unroll
    for (uint32_t k = 0; k < (uint32_t)NCH; k++) {
        const uint32_t pid = 64u * k + lane, r = pid / (uint32_t)NCH, c = pid % (uint32_t)NCH;
        const uint64_t offr = ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(off >> 32), (int)r, 64) << 32) |
                              (uint32_t)__shfl((int)(uint32_t)off, (int)r, 64);
        uint64_t a = (offr & ~(uint64_t)15) + 16u * c;
        a = a > last16 ? last16 : a;
        v[k] = up ? *reinterpret_cast<const uint4*>(P.src.slab + a) : make_uint4(0, 0, 0, 0);  // (an empty slab: no load)
    }
    ChainPre cp{};
    if (act) cp = chain_load(P, i);
    // ---- the LDS stores
#pragma unroll
    for (uint32_t k = 0; k < (uint32_t)NCH; k++) {
        const uint32_t pid = 64u * k + lane, r = pid / (uint32_t)NCH, c = pid % (uint32_t)NCH;
        uint32_t* wr = win + (wave0 + r) * kStride + 4 * c;
        wr[0] = v[k].x, wr[1] = v[k].y, wr[2] = v[k].z, wr[3] = v[k].w;
    }
    // the block's first tile: the rules, references and counters (a barrier); every tile: the wave's windows
    if (tile == blockIdx.x) __syncthreads();  // uniform
    else wave_sync();
    const uint32_t nh = act ? (cp.nh > PKT_MAX_HDRS ? PKT_MAX_HDRS : cp.nh) : 0u;
    const uint32_t* w = win + t * kStride;
    PacketView pv;
    pv.lw = reinterpret_cast<const uint8_t*>(w);
    pv.slab = P.src.slab;
    pv.off = off;
    pv.last4 = up - 4;  // (used only for a header inside the packet: up > 0)
    pv.shift = (uint32_t)(off & 15);
    pv.win_lo = 0;
    pv.win_end = 16u * NCH - pv.shift;
    pv.len = len;
    // a reference's header: its offset when it is present (listed, and wholly inside the packet), else kAbsent
    auto resolve = [&](uint32_t ref) -> uint32_t {
        const uint32_t rf = uni(reinterpret_cast<const uint32_t*>(s_refs)[ref]);  // type | occ << 8 | size << 16
        const int32_t ho = find_hdr(cp, P, i, nh, rf & 0xFFu, (rf >> 8) & 0xFFu);
        return (ho >= 0 && (uint32_t)ho + ((rf >> 16) & 0xFFu) <= len) ? (uint32_t)ho : kAbsent;
    };
    const uint32_t nrl = P.nrefs < kRefLds ? P.nrefs : kRefLds;
    for (uint32_t r = 0; r < nrl; r++) s_ho[r][t] = (uint16_t)resolve(r);  // read back by this lane alone
    // ---- the rules
    const bool full = P.matched != nullptr;
    uint64_t bits = 0;
    uint32_t first = PKT_MATCH_NONE;
    for (uint32_t r = 0; r < P.nrules; r++) {  // uniform
        bool ok = act && (full || first == PKT_MATCH_NONE);
        if (!full && !__ballot(ok)) break;  // every active lane of the wave has its first match
        const uint32_t rr = uni(reinterpret_cast<const uint32_t*>(s_rules)[2 * r]);
        const uint32_t t0 = rr & 0xFFFFu, t1 = t0 + (rr >> 16);
        uint32_t cur = 0xFFFFFFFFu, ho = kAbsent;
        for (uint32_t k = t0; k < t1; k++) {  // uniform
            if (!__ballot(ok)) break;         // no lane of the wave still holds
            // the term's 32 bytes through one scalar load: k is uniform, and nothing the kernel has stored by
            // now can alias the program (13 % faster than the terms staged in LDS at 16 x 5 and 64 x 4 terms,
            // profiles/ab/match_program_lds.txt).  A reference past the first kRefLds is looked up here, once per
            // run of consecutive terms that name it, in every rule that does: `cur` starts anew with each rule.
            const uint4 q0 = gt[2 * k];
            const uint4 q1 = gt[2 * k + 1];
            const uint64_t a = (uint64_t)uni(q0.y) << 32 | uni(q0.x), b = (uint64_t)uni(q0.w) << 32 | uni(q0.z);
            const uint32_t m0 = uni(q1.x), m1 = uni(q1.y), width = uni(q1.z);
            const uint32_t ref = m0 & 0xFFFFu, b0 = m0 >> 16, op = m1 & 0xFFu, neg = (m1 >> 8) & 1u;
            const uint32_t nb = (m1 >> 16) & 0xFFu, rsh = m1 >> 24;
            bool raw;
            if (op == PKT_MATCH_LEN) {
                raw = a <= len && len <= b;
            } else {
                if (ref != cur) {  // consecutive terms of one header: one lookup
                    ho = ref < kRefLds ? (uint32_t)s_ho[ref][t] : resolve(ref);
                    cur = ref;
                }
                const bool pres = ho != kAbsent;
                raw = pres;
                if (op != PKT_MATCH_HAS) {
                    // the field's <= 9 bytes from rel on, as extract_kernel reads them: three LDS dwords when
                    // every lane that has the header holds bytes rel .. rel + 11 in its window, else le()
                    const uint32_t rel = pres ? ho + b0 : 0u;
                    uint32_t x0, x1, x8;
                    if (!__ballot(pres && rel + 12u > pv.win_end)) {  // uniform
                        const uint32_t wb = rel + pv.shift, kk = wb >> 2, sh = wb & 3;
                        const uint32_t d0 = w[kk], d1 = w[kk + 1], d2 = w[kk + 2];
                        x0 = __builtin_amdgcn_alignbyte(d1, d0, sh);
                        x1 = __builtin_amdgcn_alignbyte(d2, d1, sh);
                        x8 = d2 >> (8u * sh);
                    } else {
                        x0 = pres ? pv.le(rel, 4) : 0u;
                        x1 = pres && nb > 4 ? pv.le(rel + 4, 4) : 0u;
                        x8 = (pres && nb == 9) ? pv.le(rel + 8, 1) : 0u;
                    }
                    // bytes b0.. as a big-endian integer, shifted right by the trailing bits, cut to the width
                    const uint64_t hi = ((uint64_t)__builtin_bswap32(x0) << 32) | __builtin_bswap32(x1);
                    uint64_t acc, top;
                    if (nb == 9) {
                        acc = (hi << 8) | (x8 & 0xFFu);
                        top = hi >> 56;
                    } else {
                        acc = hi >> (8 * (8 - nb));
                        top = 0;
                    }
                    uint64_t val = rsh ? ((acc >> rsh) | (top << (64 - rsh))) : acc;
                    if (width < 64) val &= (1ull << width) - 1;
                    raw = pres && (op == PKT_MATCH_EQ ? ((val ^ a) & b) == 0 : (a <= val && val <= b));
                }
            }
            ok = ok && (raw != (neg != 0));
        }
        if (ok) {
            bits |= 1ull << r;
            first = first == PKT_MATCH_NONE ? r : first;
        }
    }
    // ---- outputs (non-temporal, as the getter columns)
    if (act) {
        const uint32_t av = first == PKT_MATCH_NONE ? P.default_action : s_rules[first].action;
        if (P.rule) __builtin_nontemporal_store((uint8_t)first, P.rule + i);
        if (P.action) __builtin_nontemporal_store(av, P.action + i);
        if (P.select) __builtin_nontemporal_store((uint8_t)(av != 0 ? 1 : 0), P.select + i);
        if (P.matched) __builtin_nontemporal_store(bits, P.matched + i);
    }
    // ---- counters
    if (counting) {
    const uint32_t idx = first == PKT_MATCH_NONE ? P.nrules : first;
    uint64_t todo = __ballot(act);
    for (uint32_t g = 0; g < kWaveGroups && todo; g++) {  // uniform
        const uint32_t lead = (uint32_t)__ffsll((unsigned long long)todo) - 1u;
        const uint32_t il = (uint32_t)__builtin_amdgcn_readlane((int)idx, (int)uni(lead));
        const bool mine = act && idx == il;
        const uint64_t m = __ballot(mine);
        uint32_t sum = mine ? len : 0u;
#pragma unroll
        for (uint32_t x = 32; x; x >>= 1) sum += (uint32_t)__shfl_xor((int)sum, (int)x, 64);
        if (lane == lead) {
            atomicAdd(&s_hits[il], (uint32_t)__popcll((unsigned long long)m));
            atomicAdd(&s_bytes[il], (unsigned long long)sum);
        }
        todo &= ~m;
    }
    if ((todo >> lane) & 1ull) {
        atomicAdd(&s_hits[idx], 1u);
        atomicAdd(&s_bytes[idx], (unsigned long long)len);
    }
    }
    wave_sync();  // the wave has read its windows (and its lanes' s_ho) before the next tile's are stored
    }
    if (!counting) return;
    __syncthreads();
    if (t <= P.nrules) {
        const uint32_t h = s_hits[t];
        const uint64_t bsum = s_bytes[t];
        if (P.hits && h) __hip_atomic_fetch_add(P.hits + t, (uint64_t)h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (P.bytes && bsum) __hip_atomic_fetch_add(P.bytes + t, bsum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// Fixed-stride batches of <= 64-byte, 16-byte-aligned slots: 4-chunk windows (the packet) instead of 5.
bool narrow_slots(const pkt_batch_t* b) { return !b->offsets && b->stride <= 64 && b->stride % 16 == 0; }

}  // namespace

extern "C" int pkt_match_create(pkt_ctx_t* ctx, const pkt_match_term_t* terms, uint32_t nterms,
                                const pkt_match_rule_t* rules, uint32_t nrules, uint32_t default_action,
                                pkt_match_t** out) {
    if (!ctx || !out) return fail(ctx, PKT_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (const char* msg = match_program_error(terms, nterms, rules, nrules)) return fail(ctx, PKT_ERR_INVALID_ARG, msg);
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    MatchCompiled* c = new MatchCompiled;
    match_compile(terms, nterms, rules, nrules, *c);
    pkt_match* m = new pkt_match{ctx, ctx->device, nullptr, c->nterms, c->nrules, c->nrefs, default_action};
    e = hipMalloc(reinterpret_cast<void**>(&m->prog), sizeof(MatchCompiled));
    if (e == hipSuccess) e = hipMemcpy(m->prog, c, sizeof(MatchCompiled), hipMemcpyHostToDevice);
    delete c;
    if (e != hipSuccess) {
        if (m->prog) (void)hipFree(m->prog);
        delete m;
        return hip_fail(ctx, e, "pkt_match_create");
    }
    *out = m;
    return PKT_SUCCESS;
}

extern "C" int pkt_match_destroy(pkt_match_t* m) {
    if (!m) return PKT_ERR_INVALID_ARG;
    (void)hipSetDevice(m->device);
    const hipError_t e = hipFree(m->prog);
    delete m;
    return e == hipSuccess ? PKT_SUCCESS : PKT_ERR_HIP;
}

extern "C" int pkt_match_batch(pkt_match_t* m, const pkt_batch_t* b, const pkt_chain_t* chain, uint8_t* rule,
                               uint32_t* action, uint8_t* select, uint64_t* matched, uint64_t* hits, uint64_t* bytes,
                               void* stream) {
    if (!m) return PKT_ERR_INVALID_ARG;
    pkt_ctx* ctx = m->ctx;
    if (!b || !chain) return fail(ctx, PKT_ERR_INVALID_ARG, "null argument");
    if (b->n >= (1ull << 32)) return fail(ctx, PKT_ERR_INVALID_ARG, "pkt_match_batch: n >= 2^32");
    if ((uintptr_t)matched & 7) return fail(ctx, PKT_ERR_INVALID_ARG, "pkt_match_batch: matched not 8-byte aligned");
    if (((uintptr_t)hits | (uintptr_t)bytes) & 7)
        return fail(ctx, PKT_ERR_INVALID_ARG, "pkt_match_batch: hits / bytes not 8-byte aligned");
    if (b->n == 0) return PKT_SUCCESS;
    if (!chain->n_hdrs || !chain->hdr_type || !chain->hdr_off)
        return fail(ctx, PKT_ERR_INVALID_ARG, "pkt_match_batch: null chain column");
    int rc = check_batch_slab16(ctx, b);
    if (rc == PKT_SUCCESS) rc = check_batch_index(ctx, b);
    if (rc != PKT_SUCCESS) return rc;
    if (!rule && !action && !select && !matched && !hits && !bytes) return PKT_SUCCESS;
    hipError_t e = hipSetDevice(m->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    MParams P{};
    P.src = batch_src(b);
    P.n = b->n;
    P.n_hdrs = chain->n_hdrs;
    P.hdr_type = chain->hdr_type;
    P.hdr_off = chain->hdr_off;
    P.prog = m->prog;
    P.nterms = m->nterms;
    P.nrules = m->nrules;
    P.nrefs = m->nrefs;
    P.default_action = m->default_action;
    P.rule = rule;
    P.action = action;
    P.select = select;
    P.matched = matched;
    P.hits = hits;
    P.bytes = bytes;
    const uint64_t tiles = (b->n + kMBlock - 1) / kMBlock;
    const bool loop = (hits || bytes) && m->nterms <= kLoopMaxTerms && tiles > kCountBlocks;
    const dim3 grid((unsigned)(loop ? kCountBlocks : tiles));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const uint4* gt = reinterpret_cast<const uint4*>(reinterpret_cast<const uint8_t*>(m->prog) + offsetof(MatchCompiled, terms));
    if (narrow_slots(b))
        hipLaunchKernelGGL(match_kernel<4>, grid, dim3(kMBlock), 0, s, P, gt);
    else
        hipLaunchKernelGGL(match_kernel<5>, grid, dim3(kMBlock), 0, s, P, gt);
    if ((e = hipGetLastError()) != hipSuccess) return hip_fail(ctx, e, "match_kernel launch");
    return PKT_SUCCESS;
}
