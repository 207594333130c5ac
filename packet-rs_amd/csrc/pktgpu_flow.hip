// pktgpu_flow.hip — pkt_flow_key_batch and the device half of pkt_flow_table_*.
//   flow_key_kernel<RSS>  a wave owns 64 consecutive packets.  Lane p reads packet p's offset, length and chain
//                    (the first four rows up front, chain_load), finds the IP entry and the entry behind it,
//                    reads the IP header's fragment and protocol bytes, decides the status, then loads the
//                    aligned 16-byte slab chunks that cover the address bytes (and the 4 port bytes where the
//                    L4 header follows the IP header at once: every parse's chain) and takes them out with
//                    take16: 1 to 4 chunks, each holding a byte of the packet.  The key's five words are
//                    ordered (SYMMETRIC), hashed, and, RSS, run through the Toeplitz hash a dword at a time
//                    with the key's windows in scalar registers.  The wave's 64 keys (2560 bytes) go through
//                    LDS so that its lanes store consecutive 16-byte chunks.
//   flow_claim_kernel / flow_publish_kernel / flow_count_kernel   one update of the table, a packet per lane:
//                    (1) find or claim the tag's entry by compare-and-swap on its tag word, and put the lowest
//                    base + i into its `first` word; (2) the packet that holds an entry's `first` stores its
//                    key there (the only writer, plain stores); (3) every packet compares its key with its
//                    entry's and adds to the counters.  No lane waits for another lane's write: the kernel
//                    boundaries publish.  Within a launch a table word that other lanes may write is touched
//                    by agent-scope atomics alone.  In (1) and (3) a wave's lanes that hold the same entry
//                    (and direction) issue one atomic per word between them, and (3) merges a block's first
//                    groups in LDS: one add per counter and 1024 packets for an elephant flow.
//   flow_tile_kernel / flow_scan_kernel / flow_emit_kernel   count and export: the entries per tile of 1024
//                    slots, their exclusive prefix (one block; the total goes to a pinned host word), and the
//                    records written in slot order.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pktgpu_ctx.hpp"
#include "pktgpu_flow.hpp"

namespace {

constexpr uint32_t kFkBlock = 256;
constexpr uint32_t kFkWaves = kFkBlock / 64;

struct KParams {
    BatchSrc src;
    uint64_t n;  // < 2^32
    const uint8_t* n_hdrs;
    const uint8_t* hdr_type;   // [PKT_MAX_HDRS][n]
    const uint16_t* hdr_off;   // [PKT_MAX_HDRS][n]
    uint8_t* keys;             // [n][40]
    uint64_t* hash;
    uint32_t* rss;
    uint8_t* dir;
    uint32_t* plen;
    uint8_t* status;
    uint64_t seed;
    uint32_t which, flags;
    uint32_t rk[12];  // rss_key as ten big-endian words, two zero words behind them
};

__device__ __forceinline__ bool is_ip(uint32_t t) { return t == PKT_HDR_IPV4 || t == PKT_HDR_IPV6; }

__device__ __forceinline__ uint32_t be16(const uint8_t* p) { return (uint32_t)p[0] << 8 | p[1]; }

__device__ __forceinline__ uint32_t swap16(uint32_t x) { return (x >> 8 | x << 8) & 0xFFFFu; }

__device__ __forceinline__ uint4 chunk_at(const uint8_t* a) { return *reinterpret_cast<const uint4*>(a); }

// One input dword of the Toeplitz hash: x = the dword's four bytes as a big-endian value (bit 31 first), k0 | k1
// = the 64 key bits from the dword's first bit on (uniform).  Input bit b takes the 32 key bits from bit b on.
__device__ __forceinline__ uint32_t toeplitz32(uint32_t x, uint32_t k0, uint32_t k1) {
    const uint64_t k = (uint64_t)k0 << 32 | k1;
    uint32_t r = 0;
#pragma unroll
    for (uint32_t b = 0; b < 32; b++) {
        const uint32_t win = (uint32_t)(k >> (32u - b));
        r ^= (0u - (x >> (31u - b) & 1u)) & win;
    }
    return r;
}

template <bool RSS>
__global__ __launch_bounds__(kFkBlock) void flow_key_kernel(KParams P) {
    __shared__ __align__(16) uint64_t s_key[kFkWaves][64 * 5];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t i = (uint64_t)blockIdx.x * kFkBlock + threadIdx.x;
    const bool in = i < P.n;
    // the IP entry and the entry right behind it
    uint32_t ipt = 0, ipo = 0, nxt = 0, nxo = 0, len = 0;
    uint64_t off = 0;
    if (in) {
        off = pkt_off(P.src, i);
        len = pkt_len(P.src, i, off);
        const ChainPre c = chain_load(P, i);
        const uint32_t nh = c.nh > PKT_MAX_HDRS ? PKT_MAX_HDRS : c.nh;
        uint32_t seen = 0;
        bool pend = false;  // the entry before this one was taken
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            const bool live = j < nh;
            nxt = live && pend ? c.ty[j] : nxt;
            nxo = live && pend ? c.of[j] : nxo;
            pend = live ? false : pend;
            const bool hit = live && is_ip(c.ty[j]);
            const bool take = hit && (P.which == PKT_FLOW_LAST || seen == P.which);
            ipt = take ? c.ty[j] : ipt;
            ipo = take ? c.of[j] : ipo;
            nxt = take ? 0u : nxt;
            nxo = take ? 0u : nxo;
            pend = take ? true : pend;
            seen += hit ? 1u : 0u;
        }
        for (uint32_t j = 4; j < nh; j++) {
            const uint32_t t = P.hdr_type[(uint64_t)j * P.n + i], o = P.hdr_off[(uint64_t)j * P.n + i];
            if (pend) {
                nxt = t;
                nxo = o;
                pend = false;
            }
            if (is_ip(t)) {
                if (P.which == PKT_FLOW_LAST || seen == P.which) {
                    ipt = t;
                    ipo = o;
                    nxt = nxo = 0;
                    pend = true;
                }
                seen++;
            }
        }
    }
    // the status; whether ports are taken
    const bool v4 = ipt == PKT_HDR_IPV4;
    const uint32_t hs = v4 ? 20u : 40u;
    const uint8_t* pkt = P.src.slab + off;
    uint32_t st = PKT_FLOW_NO_IP, proto = 0;
    bool ports = false;
    if (ipt) {
        if (ipo + hs > len) {
            st = PKT_FLOW_SPAN;
        } else {
            st = PKT_FLOW_OK;
            const uint32_t frag = v4 ? be16(pkt + ipo + 6) & 0x3FFFu : 0u;
            proto = pkt[ipo + (v4 ? 9u : 6u)];
            ports = (nxt == PKT_HDR_TCP || nxt == PKT_HDR_UDP) && !(P.flags & PKT_FLOW_NO_PORTS) && !frag;
            if (ports && nxo + 4u > len) st = PKT_FLOW_SPAN;
        }
    }
    const bool ok = st == PKT_FLOW_OK;
    // the key's words as they lie in memory
    uint64_t w[5] = {0, 0, 0, 0, 0};
    uint32_t d = 0;
    if (ok) {
        // The span [S, S + span): the addresses (the IP header's last 8 / 32 bytes) and, where the L4 header
        // follows at once, its 4 port bytes: every byte inside the packet.  Chunk k of the aligned chunks from
        // S's on is loaded iff it holds a byte of the span, so it lies at or below the slab's last aligned chunk.
        const bool contig = ports && nxo == ipo + hs;
        const uint64_t S = off + ipo + (v4 ? 12u : 8u);
        const uint32_t span = (v4 ? 8u : 32u) + (contig ? 4u : 0u), sh = (uint32_t)S & 15u;
        const uint32_t nch = (sh + span + 15u) >> 4;  // 1..4
        const uint8_t* A = P.src.slab + (S & ~(uint64_t)15);
        const uint4 z = make_uint4(0, 0, 0, 0);
        const uint4 c0 = chunk_at(A), c1 = nch > 1 ? chunk_at(A + 16) : z, c2 = nch > 2 ? chunk_at(A + 32) : z,
                    c3 = nch > 3 ? chunk_at(A + 48) : z;
        uint32_t o0[4], pw;
        take16(c0, c1, sh, o0);
        if (v4) {
            w[0] = o0[0];
            w[2] = o0[1];
            pw = o0[2];
        } else {
            uint32_t o1[4], o2[4];
            take16(c1, c2, sh, o1);
            take16(c2, c3, sh, o2);
            w[0] = o0[0] | (uint64_t)o0[1] << 32;
            w[1] = o0[2] | (uint64_t)o0[3] << 32;
            w[2] = o1[0] | (uint64_t)o1[1] << 32;
            w[3] = o1[2] | (uint64_t)o1[3] << 32;
            pw = o2[0];
        }
        if (ports && !contig) {  // a chain that puts the L4 header elsewhere: its bytes read here
            const uint8_t* q = pkt + nxo;
            pw = q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24;
        }
        uint32_t sport = ports ? swap16(pw & 0xFFFFu) : 0u, dport = ports ? swap16(pw >> 16) : 0u;
        if (P.flags & PKT_FLOW_SYMMETRIC) {
            const uint64_t a0 = __builtin_bswap64(w[0]), b0 = __builtin_bswap64(w[2]);
            const uint64_t a1 = __builtin_bswap64(w[1]), b1 = __builtin_bswap64(w[3]);
            const bool gt = a0 != b0 ? a0 > b0 : a1 != b1 ? a1 > b1 : sport > dport;
            if (gt) {
                uint64_t t = w[0];
                w[0] = w[2];
                w[2] = t;
                t = w[1];
                w[1] = w[3];
                w[3] = t;
                const uint32_t u = sport;
                sport = dport;
                dport = u;
                d = 1;
            }
        }
        w[4] = sport | (uint64_t)dport << 16 | (uint64_t)proto << 32 | (uint64_t)(v4 ? 4u : 6u) << 40;
    }
    const uint64_t h = ok ? flow_hash(P.seed, w) : 0ull;
    uint32_t r = 0;
    if (RSS) {
        // the input a dword at a time, as big-endian values: IPv4 src, dst, ports; IPv6 four each, then ports
        const uint32_t sp = (uint32_t)w[4] & 0xFFFFu, dp = (uint32_t)(w[4] >> 16) & 0xFFFFu;
        const uint32_t pin = ports && ok ? sp << 16 | dp : 0u;
        uint32_t x[9];
        x[0] = __builtin_bswap32((uint32_t)w[0]);
        x[1] = v4 ? __builtin_bswap32((uint32_t)w[2]) : __builtin_bswap32((uint32_t)(w[0] >> 32));
        x[2] = v4 ? pin : __builtin_bswap32((uint32_t)w[1]);
        x[3] = v4 ? 0u : __builtin_bswap32((uint32_t)(w[1] >> 32));
        x[4] = v4 ? 0u : __builtin_bswap32((uint32_t)w[2]);
        x[5] = v4 ? 0u : __builtin_bswap32((uint32_t)(w[2] >> 32));
        x[6] = v4 ? 0u : __builtin_bswap32((uint32_t)w[3]);
        x[7] = v4 ? 0u : __builtin_bswap32((uint32_t)(w[3] >> 32));
        x[8] = v4 ? 0u : pin;
        const bool wide = __ballot(ok && !v4) != 0;  // uniform: a wave of IPv4 packets stops after three dwords
#pragma unroll
        for (uint32_t q = 0; q < 9; q++)
            if (q < 3 || wide) r ^= toeplitz32(x[q], P.rk[q], P.rk[q + 1]);
    }
    // the wave's keys through LDS: lanes store consecutive chunks
    if (P.keys) {
        uint64_t* sk = s_key[wv];
#pragma unroll
        for (uint32_t q = 0; q < 5; q++) sk[lane * 5u + q] = w[q];
        wave_sync();
        const uint64_t i0 = (uint64_t)blockIdx.x * kFkBlock + 64ull * wv;  // the wave's first packet
        const uint32_t words = i0 < P.n ? (P.n - i0 < 64 ? (uint32_t)(P.n - i0) * 5u : 320u) : 0u;
        uint8_t* dst = P.keys + i0 * 40u;  // i0 * 40 is a multiple of 16
        if (((uintptr_t)P.keys & 15u) == 0) {
            for (uint32_t c = lane; 2u * c < words; c += 64u) {
                if (2u * c + 1u < words)
                    *reinterpret_cast<uint4*>(dst + 16u * c) = *reinterpret_cast<const uint4*>(sk + 2u * c);
                else  // an odd count of keys ends in half a chunk
                    *reinterpret_cast<uint64_t*>(dst + 16u * c) = sk[2u * c];
            }
        } else if (((uintptr_t)P.keys & 7u) == 0) {
            for (uint32_t k = lane; k < words; k += 64u) reinterpret_cast<uint64_t*>(dst)[k] = sk[k];
        } else {
            const uint16_t* s16 = reinterpret_cast<const uint16_t*>(sk);
            for (uint32_t k = lane; k < words * 4u; k += 64u) reinterpret_cast<uint16_t*>(dst)[k] = s16[k];
        }
    }
    if (in) {
        if (P.hash) P.hash[i] = h;
        if (RSS) P.rss[i] = r;
        if (P.dir) P.dir[i] = (uint8_t)d;
        if (P.plen) P.plen[i] = len;
        if (P.status) P.status[i] = (uint8_t)st;
    }
}

// ------------------------------------------------------------------ the table
constexpr uint32_t kFtBlock = 256;
constexpr uint32_t kFtWaves = kFtBlock / 64;
constexpr uint64_t kFlowChunk = 1ull << 20;  // packets per round when the caller gives no flow_id
constexpr uint32_t kFlowPer = 4;             // consecutive slots per thread of tile / emit
constexpr uint32_t kFlowTile = kFtBlock * kFlowPer;

struct TParams {
    FlowEntry* e;
    uint64_t slots;
    uint32_t tag_bits;
    FlowUpdate u;
    uint32_t* slot;  // [n]: the packets' entries between the launches (the caller's flow_id, or scratch)
};

#define FLOW_RLX __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// lane `lead`'s value (lead uniform)
__device__ __forceinline__ uint32_t lane_value(uint32_t v, uint32_t lead) {
    return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)__builtin_amdgcn_readfirstlane(lead));
}

__device__ __forceinline__ bool skipped(const FlowUpdate& u, uint64_t i) { return u.status && u.status[i]; }

__device__ __forceinline__ uint64_t lane_value64(uint64_t v, uint32_t lead) {
    return (uint64_t)lane_value((uint32_t)(v >> 32), lead) << 32 | lane_value((uint32_t)v, lead);
}

// the entry of `tag`, found or claimed in at most `slots` probes; kFlowNone: the table is full
__device__ __forceinline__ uint32_t flow_probe(const TParams& P, uint64_t tag) {
    uint64_t pos = flow_home(tag, P.slots);
    for (uint64_t probes = 0; probes < P.slots; probes++) {
        uint64_t cur = __hip_atomic_load(&P.e[pos].tag, FLOW_RLX);
        if (cur == 0 && __hip_atomic_compare_exchange_strong(&P.e[pos].tag, &cur, tag, __ATOMIC_RELAXED, FLOW_RLX)) cur = tag;
        if (cur == tag) return (uint32_t)pos;  // a tag word is written once: what it holds is final
        pos = (pos + 1) & (P.slots - 1);
    }
    return kFlowNone;
}

// (1) a packet's entry and the entry's lowest index
__global__ __launch_bounds__(kFtBlock) void flow_claim_kernel(TParams P) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t i = (uint64_t)blockIdx.x * kFtBlock + threadIdx.x;
    const bool live = i < P.u.n && !skipped(P.u, i);
    const uint64_t tag = live ? flow_tag(P.u.hash[i], P.tag_bits) : 0ull;  // 0 is no packet's tag
    uint32_t slot = kFlowNone;
    bool need = live;
    // A wave half of whose packets or more carry its first packet's tag (an elephant flow): one lane finds or
    // claims the entry for them all, so a flow that is new costs the wave one compare-and-swap, not 64.
    const uint64_t lv = __ballot(live);
    if (lv) {
        const uint32_t lead = (uint32_t)__ffsll((unsigned long long)lv) - 1u;
        const uint64_t t0 = lane_value64(tag, lead);
        const bool same = live && tag == t0;
        if (__popcll((unsigned long long)__ballot(same)) >= 32) {  // uniform
            uint32_t s0 = kFlowNone;
            if (lane == lead) s0 = flow_probe(P, t0);
            s0 = lane_value(s0, lead);
            slot = same ? s0 : slot;
            need = need && !same;
        }
    }
    if (need) slot = flow_probe(P, tag);
    // one atomic per distinct entry of the wave, by its lowest lane: the lowest index among them
    uint64_t todo = __ballot(slot != kFlowNone);
    while (todo) {
        const uint32_t lead = (uint32_t)__ffsll((unsigned long long)todo) - 1u;
        const uint32_t s = lane_value(slot, lead);
        const uint64_t m = __ballot(slot == s);
        if (lane == lead) {
            uint64_t* first = &P.e[s].first;
            const uint64_t idx = P.u.base + i;
            if (__hip_atomic_load(first, FLOW_RLX) > idx) __hip_atomic_fetch_min(first, idx, FLOW_RLX);
        }
        todo &= ~m;
    }
    if (i < P.u.n) P.slot[i] = slot;
}

__device__ __forceinline__ void load_key(const pkt_flow_key_t* keys, uint64_t i, uint64_t w[5]) {
    const uint64_t* k = reinterpret_cast<const uint64_t*>(keys) + 5 * i;  // 8-byte aligned (refused otherwise)
#pragma unroll
    for (uint32_t q = 0; q < 5; q++) w[q] = k[q];
}

// (2) the packet with an entry's lowest index stores its key: entries of earlier updates have a lower one
__global__ __launch_bounds__(kFtBlock) void flow_publish_kernel(TParams P) {
    const uint64_t i = (uint64_t)blockIdx.x * kFtBlock + threadIdx.x;
    if (i >= P.u.n) return;
    const uint32_t slot = P.slot[i];
    if (slot == kFlowNone) return;
    FlowEntry& e = P.e[slot];
    if (e.first != P.u.base + i) return;
    uint64_t w[5];
    load_key(P.u.keys, i, w);
#pragma unroll
    for (uint32_t q = 0; q < 5; q++) e.key[q] = w[q];
}

// (3) compare and count.  A block takes kFcPer rounds of 256 packets.  In a round a wave's lanes that share an
// entry and a direction become one (entry, direction, packets, bytes) group; the block's first kFcMerge groups
// go to LDS and are merged there, so that an elephant flow costs one add per counter and 1024 packets (adds to
// one address run at about 17 ns each on the MI355X: 64 packets an add was slower than 2^20 distinct flows);
// the groups past kFcMerge, a block of many flows, add at once.
constexpr uint32_t kFcPer = 4;
constexpr uint32_t kFcTile = kFtBlock * kFcPer;
constexpr uint32_t kFcMerge = 32;

__device__ __forceinline__ void flow_add(const TParams& P, uint32_t group, uint64_t cnt, uint64_t sum) {
    FlowEntry& e = P.e[group >> 1];
    __hip_atomic_fetch_add(&e.pkts[group & 1u], cnt, FLOW_RLX);
    if (P.u.weight) __hip_atomic_fetch_add(&e.bytes[group & 1u], sum, FLOW_RLX);
}

__global__ __launch_bounds__(kFtBlock) void flow_count_kernel(TParams P) {
    __shared__ uint32_t s_n;
    __shared__ uint64_t s_grp[kFcMerge];  // entry << 1 | direction, the packets in the high half
    __shared__ uint64_t s_sum[kFcMerge];
    const uint32_t lane = threadIdx.x & 63u;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    for (uint32_t p = 0; p < kFcPer; p++) {  // uniform
        const uint64_t i = (uint64_t)blockIdx.x * kFcTile + p * kFtBlock + threadIdx.x;
        uint32_t slot = kFlowNone, st = PKT_FLOW_UPD_SKIPPED, d = 0;
        uint64_t wgt = 0;
        if (i < P.u.n && !skipped(P.u, i)) {
            slot = P.slot[i];
            st = PKT_FLOW_UPD_FULL;
            if (slot != kFlowNone) {
                uint64_t w[5];
                load_key(P.u.keys, i, w);
                const uint64_t* k = P.e[slot].key;
                bool eq = true;
#pragma unroll
                for (uint32_t q = 0; q < 5; q++) eq = eq && k[q] == w[q];
                st = eq ? PKT_FLOW_UPD_OK : PKT_FLOW_UPD_COLLISION;
                slot = eq ? slot : kFlowNone;
                d = P.u.dir ? P.u.dir[i] & 1u : 0u;
                wgt = P.u.weight ? P.u.weight[i] : 0u;
            }
        }
        const bool ok = slot != kFlowNone;
        const uint32_t g = slot << 1 | d;  // slot < 2^28
        uint64_t todo = __ballot(ok);
        while (todo) {
            const uint32_t lead = (uint32_t)__ffsll((unsigned long long)todo) - 1u;
            const uint32_t gl = lane_value(g, lead);
            const bool mine = ok && g == gl;
            const uint64_t m = __ballot(mine);
            const uint32_t cnt = (uint32_t)__popcll((unsigned long long)m);
            uint64_t sum = wgt;
            if (cnt > 1) {  // uniform
                sum = mine ? wgt : 0ull;
#pragma unroll
                for (uint32_t x = 32; x; x >>= 1) sum += __shfl_xor(sum, (int)x, 64);
            }
            if (lane == lead) {
                const uint32_t at = atomicAdd(&s_n, 1u);
                if (at < kFcMerge) {
                    s_grp[at] = (uint64_t)cnt << 32 | gl;
                    s_sum[at] = sum;
                } else {
                    flow_add(P, gl, cnt, sum);
                }
            }
            todo &= ~m;
        }
        if (i < P.u.n) {
            if (P.u.flow_id) P.u.flow_id[i] = slot;
            if (P.u.upd_status) P.u.upd_status[i] = (uint8_t)st;
        }
    }
    __syncthreads();
    const uint32_t T = s_n < kFcMerge ? s_n : kFcMerge;
    if (threadIdx.x < T) {  // the first of the groups with its entry and direction adds for them all
        const uint32_t gl = (uint32_t)s_grp[threadIdx.x];
        bool owner = true;
        uint64_t cnt = 0, sum = 0;
        for (uint32_t k = 0; k < T; k++) {
            const uint64_t o = s_grp[k];
            if ((uint32_t)o != gl) continue;
            owner = owner && k >= threadIdx.x;
            cnt += o >> 32;
            sum += s_sum[k];
        }
        if (owner) flow_add(P, gl, cnt, sum);
    }
}

// 16 bytes per thread: the empty table
__global__ __launch_bounds__(kFtBlock) void flow_clear_kernel(FlowEntry* e, uint64_t slots) {
    const uint64_t c = (uint64_t)blockIdx.x * kFtBlock + threadIdx.x;
    if (c >= slots * 8) return;
    const uint32_t hi = (c & 7) == 0 ? 0xFFFFFFFFu : 0u;  // chunk 0: tag, first
    reinterpret_cast<uint4*>(e)[c] = make_uint4(0, 0, hi, hi);
}

// Exclusive prefix of v over the block's threads; total = the block's sum.  (s_w: one word per wave.)
__device__ __forceinline__ uint32_t flow_block_scan(uint32_t v, uint32_t* s_w, uint32_t& total) {
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t x = wave_incl_scan(v, lane);
    if (lane == 63) s_w[wv] = x;
    __syncthreads();
    uint32_t base = 0;
    total = 0;
#pragma unroll
    for (uint32_t k = 0; k < kFtWaves; k++) {
        const uint32_t t = s_w[k];
        base += k < wv ? t : 0;
        total += t;
    }
    __syncthreads();  // s_w may be written again
    return base + x - v;
}

__global__ __launch_bounds__(kFtBlock) void flow_tile_kernel(const FlowEntry* e, uint64_t slots, uint32_t* tile_cnt) {
    __shared__ uint32_t s_w[kFtWaves];
    const uint64_t s0 = (uint64_t)blockIdx.x * kFlowTile + threadIdx.x * kFlowPer;
    uint32_t v = 0;
#pragma unroll
    for (uint32_t j = 0; j < kFlowPer; j++) v += s0 + j < slots && e[s0 + j].tag ? 1u : 0u;
    uint32_t total;
    (void)flow_block_scan(v, s_w, total);
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = total;
}

// one block: the tiles' counts become their exclusive prefix; the total goes to the pinned host word
__global__ __launch_bounds__(kFtBlock) void flow_scan_kernel(uint32_t* tile_cnt, uint32_t nb, uint64_t* total_host) {
    __shared__ uint32_t s_w[kFtWaves];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < nb; base += kFtBlock) {
        const uint32_t k = base + threadIdx.x;
        const uint32_t v = k < nb ? tile_cnt[k] : 0u;
        uint32_t total;
        const uint32_t ex = carry + flow_block_scan(v, s_w, total);
        if (k < nb) tile_cnt[k] = ex;
        carry += total;
    }
    if (threadIdx.x == 0) *total_host = carry;
}

__global__ __launch_bounds__(kFtBlock) void flow_emit_kernel(const FlowEntry* e, uint64_t slots, const uint32_t* tile_cnt,
                                                             pkt_flow_record_t* records, uint64_t cap) {
    __shared__ uint32_t s_w[kFtWaves];
    const uint64_t s0 = (uint64_t)blockIdx.x * kFlowTile + threadIdx.x * kFlowPer;
    bool live[kFlowPer];
    uint32_t v = 0;
#pragma unroll
    for (uint32_t j = 0; j < kFlowPer; j++) {
        live[j] = s0 + j < slots && e[s0 + j].tag;
        v += live[j] ? 1u : 0u;
    }
    uint32_t total;
    uint64_t at = (uint64_t)tile_cnt[blockIdx.x] + flow_block_scan(v, s_w, total);
#pragma unroll
    for (uint32_t j = 0; j < kFlowPer; j++) {
        if (!live[j]) continue;
        if (at < cap) {
            const FlowEntry& en = e[s0 + j];
            uint64_t* r = reinterpret_cast<uint64_t*>(records + at);  // key, first, pkts, bytes: ten words
#pragma unroll
            for (uint32_t q = 0; q < 5; q++) r[q] = en.key[q];
            r[5] = en.first;
            r[6] = en.pkts[0];
            r[7] = en.pkts[1];
            r[8] = en.bytes[0];
            r[9] = en.bytes[1];
        }
        at++;
    }
}

int flow_hip_fail(pkt_flow_table* t, hipError_t e, const char* what) {
    t->err = std::string(what) + ": " + hipGetErrorString(e);
    return PKT_ERR_HIP;
}

int dev_update(pkt_flow_table* t, const FlowUpdate& u, void* stream) {
    hipError_t e = hipSetDevice(t->device);
    if (e != hipSuccess) return flow_hip_fail(t, e, "hipSetDevice");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    // the whole update at once where the caller's flow_id holds the entries between the launches, else in
    // rounds through the table's scratch words (ascending: a round's packets come before the next one's)
    const uint64_t step = u.flow_id ? u.n : kFlowChunk;
    for (uint64_t lo = 0; lo < u.n; lo += step) {
        TParams P{};
        P.e = t->e;
        P.slots = t->slots;
        P.tag_bits = t->tag_bits;
        P.u = u;
        P.u.n = u.n - lo < step ? u.n - lo : step;
        P.u.base = u.base + lo;
        P.u.keys = u.keys + lo;
        P.u.hash = u.hash + lo;
        P.u.dir = u.dir ? u.dir + lo : nullptr;
        P.u.weight = u.weight ? u.weight + lo : nullptr;
        P.u.status = u.status ? u.status + lo : nullptr;
        P.u.flow_id = u.flow_id ? u.flow_id + lo : nullptr;
        P.u.upd_status = u.upd_status ? u.upd_status + lo : nullptr;
        P.slot = u.flow_id ? P.u.flow_id : t->slot_scratch;
        const dim3 grid((unsigned)((P.u.n + kFtBlock - 1) / kFtBlock));
        hipLaunchKernelGGL(flow_claim_kernel, grid, dim3(kFtBlock), 0, s, P);
        hipLaunchKernelGGL(flow_publish_kernel, grid, dim3(kFtBlock), 0, s, P);
        hipLaunchKernelGGL(flow_count_kernel, dim3((unsigned)((P.u.n + kFcTile - 1) / kFcTile)), dim3(kFtBlock), 0, s, P);
        if ((e = hipGetLastError()) != hipSuccess) return flow_hip_fail(t, e, "flow table update launch");
    }
    return PKT_SUCCESS;
}

int dev_scan(pkt_flow_table* t, pkt_flow_record_t* records, uint64_t cap, uint64_t* n_out, void* stream) {
    hipError_t e = hipSetDevice(t->device);
    if (e != hipSuccess) return flow_hip_fail(t, e, "hipSetDevice");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const uint32_t nb = (uint32_t)((t->slots + kFlowTile - 1) / kFlowTile);
    hipLaunchKernelGGL(flow_tile_kernel, dim3(nb), dim3(kFtBlock), 0, s, t->e, t->slots, t->tile_cnt);
    hipLaunchKernelGGL(flow_scan_kernel, dim3(1), dim3(kFtBlock), 0, s, t->tile_cnt, nb, t->total_dev);
    if (cap)
        hipLaunchKernelGGL(flow_emit_kernel, dim3(nb), dim3(kFtBlock), 0, s, t->e, t->slots, t->tile_cnt, records, cap);
    if ((e = hipGetLastError()) != hipSuccess) return flow_hip_fail(t, e, "flow table export launch");
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return flow_hip_fail(t, e, "flow table export");
    *n_out = *t->total;
    return PKT_SUCCESS;
}

int dev_clear(pkt_flow_table* t, void* stream) {
    hipError_t e = hipSetDevice(t->device);
    if (e != hipSuccess) return flow_hip_fail(t, e, "hipSetDevice");
    const uint64_t chunks = t->slots * 8;
    hipLaunchKernelGGL(flow_clear_kernel, dim3((unsigned)((chunks + kFtBlock - 1) / kFtBlock)), dim3(kFtBlock), 0,
                       reinterpret_cast<hipStream_t>(stream), t->e, t->slots);
    if ((e = hipGetLastError()) != hipSuccess) return flow_hip_fail(t, e, "flow table clear launch");
    return PKT_SUCCESS;
}

int dev_destroy(pkt_flow_table* t) {
    (void)hipSetDevice(t->device);
    (void)hipDeviceSynchronize();
    if (t->e) (void)hipFree(t->e);
    if (t->slot_scratch) (void)hipFree(t->slot_scratch);
    if (t->tile_cnt) (void)hipFree(t->tile_cnt);
    if (t->total) (void)hipHostFree(t->total);
    return PKT_SUCCESS;
}

constexpr FlowDevOps kDevOps = {dev_update, dev_scan, dev_clear, dev_destroy};

}  // namespace

extern "C" int pkt_flow_table_create(pkt_ctx_t* ctx, uint64_t slots, pkt_flow_table_t** out) {
    if (!ctx || !out) return fail(ctx, PKT_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (slots < kFlowMinSlots || slots > kFlowMaxSlots || (slots & (slots - 1)))
        return fail(ctx, PKT_ERR_INVALID_ARG, "pkt_flow_table_create: slots is not a power of two in 64..2^28");
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    pkt_flow_table* t = new pkt_flow_table;
    t->ops = &kDevOps;
    t->slots = slots;
    t->device = ctx->device;
    const uint64_t nb = (slots + kFlowTile - 1) / kFlowTile;
    e = hipMalloc(reinterpret_cast<void**>(&t->e), slots * sizeof(FlowEntry));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&t->slot_scratch), kFlowChunk * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&t->tile_cnt), nb * sizeof(uint32_t));
    if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void**>(&t->total), sizeof(uint64_t), hipHostMallocMapped);
    if (e == hipSuccess) e = hipHostGetDevicePointer(reinterpret_cast<void**>(&t->total_dev), t->total, 0);
    int rc = e == hipSuccess ? PKT_SUCCESS : hip_fail(ctx, e, "pkt_flow_table_create");
    if (rc == PKT_SUCCESS && (rc = dev_clear(t, nullptr)) != PKT_SUCCESS) ctx->err = t->err;
    if (rc == PKT_SUCCESS && (e = hipStreamSynchronize(nullptr)) != hipSuccess) rc = hip_fail(ctx, e, "pkt_flow_table_create");
    if (rc != PKT_SUCCESS) {
        dev_destroy(t);
        delete t;
        return rc;
    }
    *out = t;
    return PKT_SUCCESS;
}

extern "C" int pkt_flow_key_batch(pkt_ctx_t* ctx, const pkt_batch_t* b, const pkt_chain_t* chain, uint32_t which_ip,
                                  uint32_t flags, uint64_t seed, const uint8_t rss_key[40], pkt_flow_key_t* keys,
                                  uint64_t* hash, uint32_t* rss, uint8_t* dir, uint32_t* plen, uint8_t* status,
                                  void* stream) {
    if (!ctx || !b || !chain) return fail(ctx, PKT_ERR_INVALID_ARG, "null argument");
    if (b->n >= (1ull << 32)) return fail(ctx, PKT_ERR_INVALID_ARG, "pkt_flow_key_batch: n >= 2^32");
    if (flags & ~(PKT_FLOW_SYMMETRIC | PKT_FLOW_NO_PORTS)) return fail(ctx, PKT_ERR_INVALID_ARG, "pkt_flow_key_batch: unknown flag bits");
    if (which_ip >= PKT_MAX_HDRS && which_ip != PKT_FLOW_LAST)
        return fail(ctx, PKT_ERR_INVALID_ARG, "pkt_flow_key_batch: which_ip is neither below 16 nor PKT_FLOW_LAST");
    if (rss && !rss_key) return fail(ctx, PKT_ERR_INVALID_ARG, "pkt_flow_key_batch: rss without rss_key");
    if ((uintptr_t)keys & 1) return fail(ctx, PKT_ERR_INVALID_ARG, "pkt_flow_key_batch: keys not 2-byte aligned");
    if (b->n == 0) return PKT_SUCCESS;
    if (!chain->n_hdrs || !chain->hdr_type || !chain->hdr_off)
        return fail(ctx, PKT_ERR_INVALID_ARG, "pkt_flow_key_batch: null chain column");
    int rc = check_batch_slab16(ctx, b);
    if (rc == PKT_SUCCESS) rc = check_batch_index(ctx, b);
    if (rc != PKT_SUCCESS) return rc;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    KParams P{};
    P.src = batch_src(b);
    P.n = b->n;
    P.n_hdrs = chain->n_hdrs;
    P.hdr_type = chain->hdr_type;
    P.hdr_off = chain->hdr_off;
    P.keys = reinterpret_cast<uint8_t*>(keys);
    P.hash = hash;
    P.rss = rss;
    P.dir = dir;
    P.plen = plen;
    P.status = status;
    P.seed = seed;
    P.which = which_ip;
    P.flags = flags;
    if (rss)
        for (int k = 0; k < 10; k++)
            P.rk[k] = (uint32_t)rss_key[4 * k] << 24 | (uint32_t)rss_key[4 * k + 1] << 16 | (uint32_t)rss_key[4 * k + 2] << 8 |
                      rss_key[4 * k + 3];
    const dim3 grid((unsigned)((b->n + kFkBlock - 1) / kFkBlock));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (rss)
        hipLaunchKernelGGL(flow_key_kernel<true>, grid, dim3(kFkBlock), 0, s, P);
    else
        hipLaunchKernelGGL(flow_key_kernel<false>, grid, dim3(kFkBlock), 0, s, P);
    if ((e = hipGetLastError()) != hipSuccess) return hip_fail(ctx, e, "flow key launch");
    return PKT_SUCCESS;
}
