// pktgpu_reasm.hip — pkt_reasm_batch / _async / _result: IPv4 reassembly of a batch's fragments, the inverse of
// pktgpu_frag.hip.  Members of one datagram are found through an open-addressed table, never by a loop over a
// datagram: every kernel gives a lane one source packet (or one 16-byte chunk), so the cost is linear in n whatever
// the grouping, also when all n packets share one key or one datagram has thousands of fragments.
//   rs_classify_kernel  a lane owns a source packet: offset, length, select byte, chain (chain_load), the IP entry
//                       (frag_find_step), the aligned 16-byte slab chunks holding the IP header's 20 bytes, the
//                       classification of pktgpu_reasm.hpp.  Out: the status (members: PENDING for now), a 16-byte
//                       record (key, s, len, MF) and 8 more bytes (ip_off, chain rows, length);
//   rs_group_kernel     a member probes the group table (>= 2 n slots of 32 bits, cleared per call) from its key's home
//                       slot: one compare-and-swap of i + 1 into an empty slot; an occupied slot's key is the record of
//                       the packet named there, which rs_classify_kernel wrote: read-only here.  The packet named in
//                       the member's slot is the datagram's representative; the datagram's words (RAcc, indexed by the
//                       representative) take one 64-bit add (payload bytes), two 32-bit adds (members, finals), a max
//                       (the owner) and plain stores of E and of the s = 0 member.  A run of adjacent lanes with one
//                       representative (fragments in arrival order, a wave inside one datagram) makes those adds
//                       once, from the wave's prefix sums and lane masks.  Then (representative, s) goes into the
//                       second table, a set of fragment starts (64-bit compare-and-swap);
//   rs_link_kernel      every MF-set member looks (representative, e) up in the set; a miss sets the hole flag;
//   rs_count_kernel     the verdict (reasm_verdict) from the datagram's words, the final status, each packet's
//                       output length (WHOLE, or the owner of a JOINED datagram; else 0), the tile's (outputs,
//                       rounded bytes), and the per-status counts merged in LDS and added once per block;
//   out_scan_kernel     (pktgpu_outbatch.hip, shared with frag and icmp) one block: the exclusive prefix of the tile
//                       sums, the totals and the overflow verdict;
//   rs_emit_kernel      per tile: a block scan gives each emitting packet its output index and offset; it writes the
//                       output's row (out_off, out_len, src_index, nfrag, out_chain) and where the output lies (ROut,
//                       by representative) for the members;
//   rs_copy_kernel      source-driven: a wave walks its 64 source packets' destination chunks together (flat_walk).
//                       A packet's bytes go to [D0, D0 + dlen) of dst; a chunk is an aligned 16-byte piece of that
//                       range, built in registers from the two aligned source chunks holding its bytes and stored
//                       whole; the ragged first and last chunks of a member, which it shares with its neighbours, go
//                       as aligned 8 / 4 / 2 / 1-byte stores of its own bytes only.  The s = 0 member also carries
//                       the prefix and lays the rebuilt header over it, the final member the zero fill;
//   rs_index_kernel     out_index, when asked for.
// No lane waits for another: every atomic is one attempt; the probe loops are bounded by the slot count.  dst is never
// read, and every byte of it below the total is written exactly once.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pktgpu_ctx.hpp"
#include "pktgpu_reasm.hpp"

namespace {

constexpr uint32_t kRBlock = 256;
constexpr uint32_t kRWaves = kRBlock / 64;
constexpr uint32_t kCountBlocks = 1280;  // the counting launch's grid cap (pktgpu_frag.hip's)
constexpr uint32_t kNoHdr = 0x7FFFFF00u;  // a staged packet without a header to rebuild

// A datagram's words, indexed by its representative packet, all zero before rs_group_kernel.
struct RAcc {
    unsigned long long sum;  // the members' payload bytes
    uint32_t cnt, finals;    // members; those with MF clear
    uint32_t owner;          // the largest member index
    uint32_t E;              // the final member's end
    uint32_t s0;             // 1 + the index of a member with s = 0 (0: none)
    uint32_t hole;           // nonzero: an MF-set member's end is no member's start
};
static_assert(sizeof(RAcc) == 32, "two 16-byte loads");

// Where an output lies: indexed by the packet itself (WHOLE) or by the datagram's representative (JOINED).
struct ROut {
    uint64_t off;   // out_off[q]
    uint32_t q;
    uint32_t ipoE;  // JOINED: the s = 0 member's ip_off | E << 16
};
static_assert(sizeof(ROut) == 16, "one 16-byte load");

struct RParams {
    BatchSrc src;
    uint64_t n;  // < 2^32
    const uint8_t* n_hdrs;
    const uint8_t* hdr_type;  // [PKT_MAX_HDRS][n]
    const uint16_t* hdr_off;  // [PKT_MAX_HDRS][n]
    uint32_t which, flags;
    const uint8_t* select;
    uint8_t* st;  // the caller's status, or scratch
    uint32_t* out_index;
    uint64_t* hits;
    // scratch
    uint4* rec;      // [n]: src, dst, id | proto << 16 | MF << 24 | member << 25, len | (s / 8) << 16
    uint2* aux;      // [n]: ip_off | chain rows << 16, the packet's length
    uint32_t* grp;   // [n]: a member's representative
    uint32_t* olen;  // [n]: the output's length where the packet emits one, else 0
    ROut* gout;      // [n]
    RAcc* acc;       // [n]
    uint32_t* tab1;  // [slots]: 1 + the packet that claimed the slot
    unsigned long long* tab2;  // [slots]: (representative + 1) << 32 | s
    uint64_t mask;   // slots - 1
    uint64_t* blk_bytes;  // [tiles]
    uint64_t* blk_cnt;    // [tiles]
    uint64_t* tot;        // [bytes, outputs, overflow]
    // the outputs (not with NO_WRITE)
    uint8_t* dst;
    uint64_t dst_len, out_cap;
    uint64_t* out_off;
    uint32_t* out_len;
    uint32_t* src_index;  // may be NULL
    uint32_t* nfrag;      // may be NULL
    uint8_t* oc_nh;
    uint8_t* oc_ty;
    uint16_t* oc_of;
};

struct Member {
    uint32_t src, dst, idp, mf, s, len;
    bool member;
};
__device__ __forceinline__ uint4 rec_pack(const ReasmRec& r) {
    return make_uint4(r.src, r.dst, r.idp | r.mf << 24 | r.member << 25, r.len | (r.s >> 3) << 16);
}
__device__ __forceinline__ Member rec_unpack(uint4 v) {
    return Member{v.x, v.y, v.z & 0xFFFFFFu, v.z >> 24 & 1u, (v.w >> 16) << 3, v.w & 0xFFFFu, (v.z >> 25 & 1u) != 0};
}

__device__ __forceinline__ bool emits_whole(uint32_t st, uint32_t flags) {
    return st == PKT_REASM_WHOLE && !(flags & PKT_REASM_ONLY_JOINED);
}

// the slab bytes [S, S + 4 * W), W = 3 or 5 dwords, which lie inside a packet: the aligned chunk of S and the next
// ones iff they hold a byte of them (so each lies at or below the slab's last chunk)
template <uint32_t W>
__device__ __forceinline__ void load_hdr(const uint8_t* slab, uint64_t S, uint32_t h[W]) {
    const uint32_t sh = (uint32_t)S & 15u;
    const uint8_t* A = slab + (S & ~(uint64_t)15);
    const uint4 z = make_uint4(0, 0, 0, 0);
    const uint4 c0 = *reinterpret_cast<const uint4*>(A);
    const uint4 c1 = sh + 4u * W > 16u ? *reinterpret_cast<const uint4*>(A + 16) : z;
    uint32_t o[4];
    take16(c0, c1, sh, o);
    h[0] = o[0], h[1] = o[1], h[2] = o[2];
    if constexpr (W > 3) {
        const uint4 c2 = sh + 4u * W > 32u ? *reinterpret_cast<const uint4*>(A + 32) : z;
        uint32_t p[4];
        take16(c1, c2, sh, p);
        h[3] = o[3], h[W - 1] = p[0];
    }
}

__global__ __launch_bounds__(kRBlock) void rs_classify_kernel(RParams P) {
    const uint64_t i = (uint64_t)blockIdx.x * kRBlock + threadIdx.x;
    if (i >= P.n) return;
    const uint64_t off = pkt_off(P.src, i);
    ReasmRec r{};
    r.plen = pkt_len(P.src, i, off);
    r.st = PKT_REASM_SKIPPED;
    const ChainPre c = chain_load(P, i);
    const uint32_t sel = P.select ? P.select[i] : 1u;
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
        r.st = reasm_find_status(f, r.plen);
        if (r.st == PKT_REASM_WHOLE) {
            uint32_t h[5];
            load_hdr<5>(P.src.slab, off + f.ipo, h);
            reasm_classify(r, f, nh, h);
        }
    }
    P.rec[i] = rec_pack(r);
    P.aux[i] = make_uint2(r.ipo | r.nh << 16, r.plen);
    P.st[i] = (uint8_t)r.st;
}

__global__ __launch_bounds__(kRBlock) void rs_group_kernel(RParams P) {
    const uint64_t i = (uint64_t)blockIdx.x * kRBlock + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const Member m = i < P.n ? rec_unpack(P.rec[i]) : Member{};
    const bool mem = m.member;  // (no lane leaves before the wave's shuffles below)
    const uint32_t me = (uint32_t)i;
    uint32_t rep = me;
    uint64_t slot = 0;
    if (mem) {
        slot = reasm_key_hash(m.src, m.dst, m.idp) & P.mask;
        for (uint64_t k = 0; k <= P.mask; k++, slot = (slot + 1) & P.mask) {  // at most n slots are ever taken
            uint32_t occ = __hip_atomic_load(P.tab1 + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (!occ) occ = atomicCAS(P.tab1 + slot, 0u, me + 1u);
            if (!occ) break;  // claimed: this packet represents its datagram
            const uint4 o = P.rec[occ - 1u];
            if (reasm_same_key(m.src, m.dst, m.idp, o.x, o.y, o.z & 0xFFFFFFu)) {
                rep = occ - 1u;
                break;
            }
        }
        P.grp[i] = rep;
    }
    // A run of adjacent lanes with one representative (fragments that arrive in order; a wave of one datagram) adds
    // once, by its first lane: the run's payload bytes from the wave's prefix sums, its members and finals from the
    // lane masks, its largest index from its last lane.  Shuffled members form runs of one.
    const uint32_t run_key = mem ? rep : 0xFFFFFFFFu;  // (a representative is below 2^32 - 1)
    const uint32_t prev = __shfl_up(run_key, 1, 64);
    const bool head = lane == 0 || prev != run_key;
    const uint64_t heads = __ballot(head), finals = __ballot(mem && !m.mf);
    const uint32_t incl = wave_incl_scan(mem ? m.len : 0u, lane);
    const uint64_t above = lane == 63 ? 0ull : heads >> (lane + 1u);
    const uint32_t end = above ? lane + (uint32_t)__builtin_ctzll(above) : 63u;  // the run is lanes [lane, end]
    const uint32_t incl_end = __shfl(incl, end, 64);
    if (!mem) return;
    RAcc* a = P.acc + rep;
    if (head) {
        const uint64_t run = (end == 63u ? ~0ull : (1ull << (end + 1u)) - 1ull) & ~((1ull << lane) - 1ull);
        const uint32_t f = (uint32_t)__popcll((unsigned long long)(finals & run));
        atomicAdd(&a->sum, (unsigned long long)(incl_end - (incl - m.len)));
        atomicAdd(&a->cnt, end - lane + 1u);
        atomicMax(&a->owner, me + (end - lane));
        if (f) atomicAdd(&a->finals, f);
    }
    if (!m.mf) a->E = m.s + m.len;  // two finals: either store; the datagram is PENDING
    if (m.s == 0) a->s0 = me + 1u;  // two members at 0: either store; the datagram is PENDING
    const unsigned long long key = (unsigned long long)(rep + 1u) << 32 | m.s;
    slot = flow_mix64(key) & P.mask;
    for (uint64_t k = 0; k <= P.mask; k++, slot = (slot + 1) & P.mask) {
        const unsigned long long old = atomicCAS(P.tab2 + slot, 0ull, key);
        if (old == 0 || old == key) break;  // (a duplicate start: the set keeps one, the sum tells)
    }
}

__global__ __launch_bounds__(kRBlock) void rs_link_kernel(RParams P) {
    const uint64_t i = (uint64_t)blockIdx.x * kRBlock + threadIdx.x;
    if (i >= P.n) return;
    const Member m = rec_unpack(P.rec[i]);
    if (!m.member || !m.mf) return;
    const uint32_t rep = P.grp[i];
    const unsigned long long key = (unsigned long long)(rep + 1u) << 32 | (m.s + m.len);
    uint64_t slot = flow_mix64(key) & P.mask;
    bool found = false;
    for (uint64_t k = 0; k <= P.mask; k++, slot = (slot + 1) & P.mask) {
        const unsigned long long v = P.tab2[slot];  // the previous launch filled the set
        found = v == key;
        if (found || v == 0) break;
    }
    if (!found) P.acc[rep].hole = 1u;
}

__global__ __launch_bounds__(kRBlock) void rs_count_kernel(RParams P) {
    __shared__ uint32_t s_hits[PKT_REASM_STATUS_COUNT];
    __shared__ uint64_t s_w[kRWaves];
    const uint32_t t = threadIdx.x;
    if (P.hits) hits_zero<PKT_REASM_STATUS_COUNT>(s_hits, t);
    const uint32_t ntiles = (uint32_t)((P.n + kRBlock - 1) / kRBlock);
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {  // uniform
        const uint64_t i = (uint64_t)tile * kRBlock + t;
        const bool act = i < P.n;
        uint32_t st = PKT_REASM_SKIPPED, ol = 0;
        if (act) {
            st = P.st[i];
            if (st == PKT_REASM_PENDING) {  // a member
                const uint4* ap = reinterpret_cast<const uint4*>(P.acc + P.grp[i]);
                const uint4 a0 = ap[0], a1 = ap[1];  // sum, cnt, finals | owner, E, s0, hole
                const uint64_t sum = (uint64_t)a0.x | (uint64_t)a0.y << 32;
                st = reasm_verdict(a0.w, a1.z != 0, a1.w != 0, sum, a1.y);
                if (st != PKT_REASM_PENDING) P.st[i] = (uint8_t)st;
                if (st == PKT_REASM_JOINED && a1.x == (uint32_t)i) ol = (P.aux[a1.z - 1u].x & 0xFFFFu) + 20u + a1.y;
            } else if (emits_whole(st, P.flags)) {
                ol = P.aux[i].y;
            }
            P.olen[i] = ol;
        }
        uint64_t tc, tb;
        (void)block_excl_scan<kRWaves>(ol ? 1u : 0u, s_w, tc);
        (void)block_excl_scan<kRWaves>(out_round16(ol), s_w, tb);
        if (t == 0) {
            P.blk_cnt[tile] = tc;
            P.blk_bytes[tile] = tb;
        }
        if (P.hits) hits_add<PKT_REASM_STATUS_COUNT>(s_hits, t, act, st);
    }
    if (P.hits) hits_flush<PKT_REASM_STATUS_COUNT>(s_hits, t, P.hits);
}

__global__ __launch_bounds__(kRBlock) void rs_emit_kernel(RParams P) {
    __shared__ uint64_t s_w[kRWaves];
    const uint64_t i = (uint64_t)blockIdx.x * kRBlock + threadIdx.x;
    const bool act = i < P.n;
    const uint32_t ol = act ? P.olen[i] : 0u;
    uint64_t tc, tb;
    const uint64_t q = P.blk_cnt[blockIdx.x] + block_excl_scan<kRWaves>(ol ? 1u : 0u, s_w, tc);
    const uint64_t o = P.blk_bytes[blockIdx.x] + block_excl_scan<kRWaves>(out_round16(ol), s_w, tb);
    if (!ol) return;
    // an emitting packet is WHOLE, or the owner of a JOINED datagram
    uint64_t rows_of = i, g = i;
    uint32_t members = 1, ipoE = 0;
    if (P.st[i] == PKT_REASM_JOINED) {
        g = P.grp[i];
        const uint4* ap = reinterpret_cast<const uint4*>(P.acc + g);
        const uint4 a0 = ap[0], a1 = ap[1];
        members = a0.z;
        rows_of = a1.z - 1u;
        ipoE = (P.aux[rows_of].x & 0xFFFFu) | a1.y << 16;  // JOINED: E <= 65515
    }
    P.gout[g] = ROut{o, (uint32_t)q, ipoE};
    if ((P.flags & PKT_REASM_NO_WRITE) || P.tot[2]) return;  // the sizing pass, or the outputs do not fit
    P.out_off[q] = o;  // q < the outputs' total <= out_cap
    P.out_len[q] = ol;
    if (P.src_index) P.src_index[q] = (uint32_t)i;
    if (P.nfrag) P.nfrag[q] = members;
    const uint32_t nh = P.aux[rows_of].x >> 16;  // at most PKT_MAX_HDRS
    if (P.oc_nh) P.oc_nh[q] = (uint8_t)nh;
    for (uint32_t k = 0; k < nh; k++) {
        if (P.oc_ty) P.oc_ty[(uint64_t)k * P.out_cap + q] = P.hdr_type[(uint64_t)k * P.n + rows_of];
        if (P.oc_of) P.oc_of[(uint64_t)k * P.out_cap + q] = P.hdr_off[(uint64_t)k * P.n + rows_of];
    }
}

__global__ __launch_bounds__(kRBlock) void rs_copy_kernel(RParams P) {
    __shared__ uint32_t s_pre[kRWaves][65];
    __shared__ uint64_t s_dst[kRWaves][64], s_src[kRWaves][64];
    __shared__ uint32_t s_lo[kRWaves][64], s_dend[kRWaves][64], s_hend[kRWaves][64], s_ipo[kRWaves][64];
    __shared__ uint32_t s_h[kRWaves][3][64];
    if (P.tot[2]) return;  // (uniform) the outputs do not fit: the host reports the capacity needed
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
    const uint64_t n_out = P.tot[1];
    const uint64_t i = (uint64_t)blockIdx.x * kRBlock + t;
    if (i >= n_out && i < P.out_cap) {  // the empty tail
        P.out_off[i] = 0;
        P.out_len[i] = 0;
        if (P.src_index) P.src_index[i] = PKT_REASM_NONE;
        if (P.nfrag) P.nfrag[i] = 0;
        if (P.oc_nh) P.oc_nh[i] = 0;
    }
    // this source packet's bytes go to dst [D0, D0 + dlen), from the slab at S0 on
    uint32_t chunks = 0;
    const uint32_t st = i < P.n ? P.st[i] : PKT_REASM_SKIPPED;
    if (st == PKT_REASM_JOINED || emits_whole(st, P.flags)) {
        const uint64_t off = pkt_off(P.src, i);
        uint64_t D0, S0 = off;
        uint32_t dlen, ipo = kNoHdr, o[3] = {0, 0, 0};
        bool last = true;  // the zero fill up to the output's rounded end is this packet's
        if (st == PKT_REASM_WHOLE) {
            D0 = P.gout[i].off;
            dlen = P.aux[i].y;
        } else {
            const Member m = rec_unpack(P.rec[i]);
            const ROut g = P.gout[P.grp[i]];
            const uint32_t ipo0 = g.ipoE & 0xFFFFu, my_ipo = P.aux[i].x & 0xFFFFu;
            last = !m.mf;
            if (m.s == 0) {  // the prefix and the header go with the first payload
                uint32_t h[3];
                load_hdr<3>(P.src.slab, off + my_ipo, h);
                reasm_header(g.ipoE >> 16, h, o);
                ipo = my_ipo;
                D0 = g.off;
                dlen = my_ipo + 20u + m.len;
            } else {
                D0 = g.off + ipo0 + 20u + m.s;
                dlen = m.len;
                S0 = off + my_ipo + 20u;
            }
        }
        const uint32_t lo = (uint32_t)D0 & 15u, dend = lo + dlen;
        s_dst[wv][lane] = D0 - lo;
        s_src[wv][lane] = S0 - lo;  // S0 >= 20 where lo > 0: a member's payload lies behind its IP header
        s_lo[wv][lane] = lo;
        s_dend[wv][lane] = dend;
        s_hend[wv][lane] = last ? out_round16(dend) : dend;
        s_ipo[wv][lane] = ipo;
        s_h[wv][0][lane] = o[0], s_h[wv][1][lane] = o[1], s_h[wv][2][lane] = o[2];
        chunks = (dend + 15u) >> 4;  // at most 4096
    }
    const uint32_t incl = wave_incl_scan(chunks, lane);
    s_pre[wv][lane + 1] = incl;
    if (lane == 0) s_pre[wv][0] = 0;
    wave_sync();
    const uint32_t total = s_pre[wv][64];  // at most 64 * 4096
    const FlatWalk w = flat_walk(chunks);
    const uint64_t last16 = slab_last16(P.src);
    for (uint32_t f = lane; f < total; f += 64) {
        const FlatAt at = locate(w, s_pre[wv], f);
        const uint32_t s = at.p, B0 = 16u * at.k;  // the chunk's first byte, counted from the packet's aligned start
        const uint32_t dend = s_dend[wv][s], hend = s_hend[wv][s], ipo = s_ipo[wv][s];
        const uint32_t lo = at.k ? 0u : s_lo[wv][s];              // the chunk's bytes [lo, hi) are this packet's,
        const uint32_t hi = hend - B0 > 16u ? 16u : hend - B0;    // those from dend - B0 on zero
        Le128 v = load16(P.src.slab, s_src[wv][s] + B0, last16);
        const int32_t rel = (int32_t)ipo - (int32_t)B0;  // the rebuilt header's bytes 0..11 (lo is 0 for its packet)
        if (rel > -12 && rel < 16) {
            const Le128 hv{(uint64_t)s_h[wv][0][s] | (uint64_t)s_h[wv][1][s] << 32, (uint64_t)s_h[wv][2][s]};
            const Le128 hm{~0ull, 0xFFFFFFFFull};
            const Le128 sv = rel >= 0 ? bytes_up(hv, (uint32_t)rel) : bytes_down(hv, (uint32_t)-rel);
            const Le128 sm = rel >= 0 ? bytes_up(hm, (uint32_t)rel) : bytes_down(hm, (uint32_t)-rel);
            v.lo = (v.lo & ~sm.lo) | sv.lo;
            v.hi = (v.hi & ~sm.hi) | sv.hi;
        }
        const Le128 keep = bytes_below(dend - B0 > 16u ? 16u : dend - B0);
        v.lo &= keep.lo;
        v.hi &= keep.hi;
        uint8_t* d = P.dst + s_dst[wv][s] + B0;
        if (lo == 0 && hi == 16u) {
            *reinterpret_cast<uint4*>(d) = make_uint4((uint32_t)v.lo, (uint32_t)(v.lo >> 32), (uint32_t)v.hi, (uint32_t)(v.hi >> 32));
            continue;
        }
        // a ragged chunk: the largest aligned pieces inside [lo, hi), at most seven
        for (uint32_t p = lo; p < hi;) {
            uint32_t sz = p & 1u ? 1u : p & 2u ? 2u : p & 4u ? 4u : 8u;
            while (p + sz > hi) sz >>= 1;
            const uint64_t x = bytes_down(v, p).lo;
            if (sz == 8u) *reinterpret_cast<uint64_t*>(d + p) = x;
            else if (sz == 4u) *reinterpret_cast<uint32_t*>(d + p) = (uint32_t)x;
            else if (sz == 2u) *reinterpret_cast<uint16_t*>(d + p) = (uint16_t)x;
            else d[p] = (uint8_t)x;
            p += sz;
        }
    }
}

__global__ __launch_bounds__(kRBlock) void rs_index_kernel(RParams P) {
    const uint64_t i = (uint64_t)blockIdx.x * kRBlock + threadIdx.x;
    if (i >= P.n) return;
    const uint32_t st = P.st[i];
    uint32_t q = PKT_REASM_NONE;
    if (st == PKT_REASM_JOINED) q = P.gout[P.grp[i]].q;
    else if (emits_whole(st, P.flags)) q = P.gout[i].q;
    P.out_index[i] = q;
}

constexpr OutEntry kReasmEntry{&pkt_ctx::rs, "pkt_reasm_batch", "pkt_reasm_result"};

// The launches, queued on s.  The totals and the verdict arrive in ctx->rs.ctl once the stream has passed them.
int rs_queue(pkt_ctx_t* ctx, const pkt_batch_t* b, const pkt_chain_t* chain, uint32_t which_ip, uint32_t flags,
             const uint8_t* select, uint8_t* status, uint32_t* out_index, uint8_t* dst, uint64_t dst_len, uint64_t out_cap,
             uint64_t* out_off, uint32_t* out_len, uint32_t* src_index, uint32_t* nfrag, const pkt_chain_t* out_chain,
             uint64_t* hits, hipStream_t s) {
    if (!ctx) return PKT_ERR_INVALID_ARG;
    if (const char* msg = reasm_call_error(b, chain, which_ip, flags, dst, out_cap, out_off, out_len, hits, true))
        return pktgpu_out_refuse(ctx, kReasmEntry, msg);
    OutScratch& rs = ctx->rs;
    if (rs.pending)
        return pktgpu_out_refuse(ctx, kReasmEntry, "a queued call's result has not been taken on this ctx (pkt_reasm_result)");
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    const bool write = !(flags & PKT_REASM_NO_WRITE);
    if (!write) out_cap = 0;
    const uint64_t n = b->n;
    const uint32_t nb = (uint32_t)((n + kRBlock - 1) / kRBlock);
    uint64_t slots = 16;  // a power of two >= 2 n
    while (slots < 2 * n) slots <<= 1;
    // per packet: 16 (rec) + 8 (aux) + 1 (status) + 4 (grp) + 4 (olen) + 16 (gout) + 32 (acc) and 12 per slot
    const uint64_t o_bytes = 64, o_cnt = o_bytes + round16(8ull * nb), o_rec = o_cnt + round16(8ull * nb);
    const uint64_t o_gout = o_rec + 16 * n, o_aux = o_gout + 16 * n, o_grp = o_aux + round16(8 * n);
    const uint64_t o_olen = o_grp + round16(4 * n), o_st = o_olen + round16(4 * n), o_acc = o_st + round16(n);
    const uint64_t o_tab2 = o_acc + 32 * n, o_tab1 = o_tab2 + 8 * slots, need = o_tab1 + 4 * slots;
    if ((e = rs.reserve(need)) != hipSuccess) return hip_fail(ctx, e, "hipMalloc (pkt_reasm_batch)");
    if ((e = rs.ensure(64)) != hipSuccess) return hip_fail(ctx, e, "hipHostMalloc (pkt_reasm_batch)");
    char* p = static_cast<char*>(rs.buf);
    RParams P{};
    P.src = batch_src(b);
    P.n = n;
    P.n_hdrs = chain->n_hdrs;
    P.hdr_type = chain->hdr_type;
    P.hdr_off = chain->hdr_off;
    P.which = which_ip;
    P.flags = flags;
    P.select = select;
    P.st = status ? status : reinterpret_cast<uint8_t*>(p + o_st);
    P.out_index = out_index;
    P.hits = hits;
    P.tot = reinterpret_cast<uint64_t*>(p);
    P.blk_bytes = reinterpret_cast<uint64_t*>(p + o_bytes);
    P.blk_cnt = reinterpret_cast<uint64_t*>(p + o_cnt);
    P.rec = reinterpret_cast<uint4*>(p + o_rec);
    P.gout = reinterpret_cast<ROut*>(p + o_gout);
    P.aux = reinterpret_cast<uint2*>(p + o_aux);
    P.grp = reinterpret_cast<uint32_t*>(p + o_grp);
    P.olen = reinterpret_cast<uint32_t*>(p + o_olen);
    P.acc = reinterpret_cast<RAcc*>(p + o_acc);
    P.tab2 = reinterpret_cast<unsigned long long*>(p + o_tab2);
    P.tab1 = reinterpret_cast<uint32_t*>(p + o_tab1);
    P.mask = slots - 1;
    if (write) {
        P.dst = dst;
        P.dst_len = dst_len;
        P.out_cap = out_cap;
        P.out_off = out_off;
        P.out_len = out_len;
        P.src_index = src_index;
        P.nfrag = nfrag;
        const OutChainCols oc = out_chain_cols(out_chain);
        P.oc_nh = oc.nh, P.oc_ty = oc.ty, P.oc_of = oc.of;
    }
    rs.ctl[0] = rs.ctl[1] = rs.ctl[2] = 0;
    const dim3 blk(kRBlock);
    if (nb) {
        // the datagrams' words and the two tables start as zeros
        if ((e = hipMemsetAsync(p + o_acc, 0, need - o_acc, s)) != hipSuccess) return hip_fail(ctx, e, "hipMemsetAsync (pkt_reasm_batch)");
        hipLaunchKernelGGL(rs_classify_kernel, dim3(nb), blk, 0, s, P);
        hipLaunchKernelGGL(rs_group_kernel, dim3(nb), blk, 0, s, P);
        hipLaunchKernelGGL(rs_link_kernel, dim3(nb), blk, 0, s, P);
        hipLaunchKernelGGL(rs_count_kernel, dim3(hits && nb > kCountBlocks ? kCountBlocks : nb), blk, 0, s, P);
    }
    pktgpu_out_scan_launch(P.blk_bytes, P.blk_cnt, nb, !write, out_cap, dst_len, P.tot, rs.ctl_dev, s);
    if (nb && (write || out_index)) hipLaunchKernelGGL(rs_emit_kernel, dim3(nb), blk, 0, s, P);
    if (write) {
        const uint64_t lanes = n > out_cap ? n : out_cap;
        hipLaunchKernelGGL(rs_copy_kernel, dim3((unsigned)((lanes + kRBlock - 1) / kRBlock)), blk, 0, s, P);
    }
    if (nb && out_index) hipLaunchKernelGGL(rs_index_kernel, dim3(nb), blk, 0, s, P);
    if ((e = hipGetLastError()) != hipSuccess) return hip_fail(ctx, e, "pkt_reasm_batch launch");
    return PKT_SUCCESS;
}

}  // namespace

extern "C" {

int pkt_reasm_batch(pkt_ctx_t* ctx, const pkt_batch_t* batch, const pkt_chain_t* chain, uint32_t which_ip, uint32_t flags,
                    const uint8_t* select, uint8_t* status, uint32_t* out_index, uint8_t* dst, uint64_t dst_len,
                    uint64_t out_cap, uint64_t* out_off, uint32_t* out_len, uint32_t* src_index, uint32_t* nfrag,
                    const pkt_chain_t* out_chain, uint64_t* hits, uint64_t* bytes_out_total, uint64_t* n_out, void* stream) {
    const auto queue = [&](hipStream_t s) {
        return rs_queue(ctx, batch, chain, which_ip, flags, select, status, out_index, dst, dst_len, out_cap, out_off, out_len,
                        src_index, nfrag, out_chain, hits, s);
    };
    return pktgpu_out_batch(ctx, kReasmEntry, queue, stream, bytes_out_total, n_out);
}

int pkt_reasm_batch_async(pkt_ctx_t* ctx, const pkt_batch_t* batch, const pkt_chain_t* chain, uint32_t which_ip,
                          uint32_t flags, const uint8_t* select, uint8_t* status, uint32_t* out_index, uint8_t* dst,
                          uint64_t dst_len, uint64_t out_cap, uint64_t* out_off, uint32_t* out_len, uint32_t* src_index,
                          uint32_t* nfrag, const pkt_chain_t* out_chain, uint64_t* hits, void* stream) {
    const auto queue = [&](hipStream_t s) {
        return rs_queue(ctx, batch, chain, which_ip, flags, select, status, out_index, dst, dst_len, out_cap, out_off, out_len,
                        src_index, nfrag, out_chain, hits, s);
    };
    return pktgpu_out_batch_async(ctx, kReasmEntry, queue, stream);
}

int pkt_reasm_result(pkt_ctx_t* ctx, uint64_t* bytes_out_total, uint64_t* n_out) {
    return pktgpu_out_result(ctx, kReasmEntry, bytes_out_total, n_out);
}

}  // extern "C"
