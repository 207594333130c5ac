// pktgpu_nat.hip — pkt_nat_create and the device half of pkt_nat_*: NAPT44 sessions and translation.
// A lane owns a packet; no lane waits for another; the kernel boundaries publish.  One call, per chunk of 2^20 packets:
//   nat_claim_kernel   classify the OUT packets (nat_classify, pktgpu_nat.hpp), find or claim the key's slot of the
//                      forward index by a 64-bit compare-and-swap (pkt_flow_table_update's pattern); a slot with no
//                      session takes the lowest index of the packets that want one (a wave adds once per slot).
//   nat_rank_kernel    the creators (the packets that hold their slot's lowest index) per tile of 256 and protocol;
//                      their totals go to three device words.
//   nat_free_kernel    the free pool entries of each segment of the free map, in circular order from the cursor.
//   nat_scan_kernel    one block: the exclusive prefixes of both, the totals, and the cursor after the call.
//   nat_alloc_kernel   the j-th creator of a protocol, in index order, takes the j-th free entry in circular order
//                      (nat_select: a bisection over the segments' prefix, then popcounts), and publishes the reverse
//                      map, last_seen and the slot's value; creators past the free count leave the slot without one.
//   nat_mark_kernel    the entries taken go into the free map (the kernel before read it).
// The last four return at once when the chunk creates nothing: the scan kernel moves the creator counts where they read
// them, no host readback decides it.  Then, over the whole batch:
//   nat_xlate_kernel   classify again, OUT: look the key up (a session: OK, none: EXHAUSTED, no slot: TABLE_FULL), IN:
//                      statics by bisection, else the direct-mapped reverse map; refresh last_seen (an atomic max only
//                      where it is behind), rewrite with byte stores (nat_rewrite), and count per status as
//                      fwd_kernel does.
// Housekeeping: nat_expire_kernel frees the idle entries, nat_rebuild_kernel re-inserts the statics and the survivors
// into the second forward buffer, and the handle swaps the two.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "pktgpu_ctx.hpp"
#include "pktgpu_nat.hpp"

namespace {

constexpr uint32_t kNBlock = 256;
constexpr uint64_t kNatChunk = 1ull << 20;
constexpr uint32_t kNatTiles = (uint32_t)(kNatChunk / kNBlock);
constexpr uint32_t kScanBlock = 1024;
constexpr uint32_t kWaveGroups = 4;     // fwd_kernel's
constexpr uint32_t kCountBlocks = 1280;  // fwd_kernel's cap on a counting launch's grid, taken over, not measured again
// ctl words
constexpr uint32_t kCtlNew = 0, kCtlCreate = 3, kCtlCur0 = 6, kCtlExpired = 9, kCtlWords = 16;

#define NAT_RLX __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

struct NParams {
    NatView v;
    NatCall c;
    uint64_t c0;   // the chunk's first packet
    uint32_t cn;   // its packets
    uint32_t* slot_scr;
    uint32_t* tile_cnt;
    uint32_t* seg;
    uint32_t* ctl;
};

__device__ __forceinline__ uint32_t lane_value(uint32_t v, uint32_t lead) {
    return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)__builtin_amdgcn_readfirstlane(lead));
}

// the slot of `key` in the forward index (fkey, slots), claimed if it has none and there is room; kNatNoSlot: full
__device__ __forceinline__ uint32_t nat_claim(uint64_t* fkey, uint64_t slots, uint64_t key) {
    uint64_t pos = nat_home(key, slots);
    for (uint64_t probes = 0; probes < slots; probes++) {
        uint64_t cur = __hip_atomic_load(&fkey[pos], NAT_RLX);
        if (cur == 0 && __hip_atomic_compare_exchange_strong(&fkey[pos], &cur, key, __ATOMIC_RELAXED, NAT_RLX)) cur = key;
        if (cur == key) return (uint32_t)pos;  // a key word is written once: what it holds is final
        pos = (pos + 1) & (slots - 1);
    }
    return kNatNoSlot;
}

// the same with no claim: an empty slot ends the search (nothing is removed from a buffer in use)
__device__ __forceinline__ uint32_t nat_find(const uint64_t* fkey, uint64_t slots, uint64_t key) {
    uint64_t pos = nat_home(key, slots);
    for (uint64_t probes = 0; probes < slots; probes++) {
        const uint64_t cur = fkey[pos];
        if (cur == key) return (uint32_t)pos;
        if (cur == 0) return kNatNoSlot;
        pos = (pos + 1) & (slots - 1);
    }
    return kNatNoSlot;
}

__device__ __forceinline__ NatPkt classify(const NatCall& c, uint64_t i, uint32_t dir, uint64_t& off, uint32_t& len) {
    off = pkt_off(c.src, i);
    len = pkt_len(c.src, i, off);
    return nat_classify(c.src.slab + off, len, c.n_hdrs, c.hdr_type, c.hdr_off, c.n, i, c.which, dir);
}

__global__ __launch_bounds__(kNBlock) void nat_claim_kernel(NParams P) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t r = blockIdx.x * kNBlock + threadIdx.x;
    const uint64_t i = P.c0 + r;
    const bool in = r < P.cn;
    uint32_t slot = kNatNoSlot;
    if (in) {
        if (P.c.created) P.c.created[i] = 0;
        if (nat_dir(P.c, i) == PKT_NAT_OUT) {
            uint64_t off;
            uint32_t len;
            const NatPkt k = classify(P.c, i, PKT_NAT_OUT, off, len);
            if (k.st == PKT_NAT_OK) {
                slot = nat_claim(P.v.fkey, P.v.slots, k.key);
                // a value is written by nat_alloc_kernel alone: a slot that has one holds a session or a static
                if (slot != kNatNoSlot && P.v.fval[slot] != PKT_NAT_NONE) slot = kNatNoSlot;
            }
        }
    }
    // one atomic per distinct slot of the wave, by its lowest lane: the lowest index among them
    uint64_t todo = __ballot(slot != kNatNoSlot);
    while (todo) {
        const uint32_t lead = (uint32_t)__ffsll((unsigned long long)todo) - 1u;
        const uint32_t s = lane_value(slot, lead);
        const uint64_t m = __ballot(slot == s);
        if (lane == lead) {
            uint32_t* first = &P.v.ffirst[s];
            if (__hip_atomic_load(first, NAT_RLX) > (uint32_t)i) __hip_atomic_fetch_min(first, (uint32_t)i, NAT_RLX);
        }
        todo &= ~m;
    }
    if (in) P.slot_scr[r] = slot;
}

__global__ __launch_bounds__(kNBlock) void nat_rank_kernel(NParams P) {
    __shared__ uint32_t s_cnt[3];
    const uint32_t t = threadIdx.x, lane = t & 63u;
    if (t < 3) s_cnt[t] = 0;
    __syncthreads();
    const uint32_t r = blockIdx.x * kNBlock + t;
    const bool in = r < P.cn;
    uint32_t slot = in ? P.slot_scr[r] : kNatNoSlot, p = 3;
    if (slot != kNatNoSlot) {
        if (P.v.ffirst[slot] == (uint32_t)(P.c0 + r))
            p = nat_key_p(P.v.fkey[slot]);
        else
            slot = kNatNoSlot;
    }
    if (in) P.slot_scr[r] = slot;  // the creators' slots alone
    for (uint32_t q = 0; q < 3; q++) {
        const uint64_t m = __ballot(p == q);
        if (lane == 0 && m) atomicAdd(&s_cnt[q], (uint32_t)__popcll((unsigned long long)m));
    }
    __syncthreads();
    if (t < 3) {
        const uint32_t cnt = s_cnt[t];
        P.tile_cnt[t * kNatTiles + blockIdx.x] = cnt;
        if (cnt) __hip_atomic_fetch_add(&P.ctl[kCtlNew + t], cnt, NAT_RLX);
    }
}

__global__ __launch_bounds__(kNBlock) void nat_free_kernel(NParams P) {
    const uint32_t g = blockIdx.x * kNBlock + threadIdx.x, per = P.v.nblk + 1u;
    if (g >= 3u * per) return;
    const uint32_t p = g / per, k = g % per;
    if (P.ctl[kCtlNew + p] == 0) return;
    P.seg[p * (per + 1u) + k] = nat_segment_free(P.v.used + p * P.v.W, k, P.v.cursor[p], P.v.E, P.v.nblk);
}

// x[0 .. cnt) becomes its exclusive prefix; the sum is returned to every thread (one block of kScanBlock threads)
__device__ __forceinline__ uint32_t scan_in_place(uint32_t* x, uint32_t cnt, uint64_t* s_w) {
    uint64_t carry = 0;
    for (uint32_t base = 0; base < cnt; base += kScanBlock) {  // uniform
        const uint32_t idx = base + threadIdx.x;
        const uint64_t v = idx < cnt ? x[idx] : 0u;
        uint64_t total;
        const uint64_t ex = block_excl_scan<kScanBlock / 64>(v, s_w, total);
        if (idx < cnt) x[idx] = (uint32_t)(carry + ex);
        carry += total;
    }
    return (uint32_t)carry;
}

__global__ __launch_bounds__(kScanBlock) void nat_scan_kernel(NParams P) {
    __shared__ uint64_t s_w[kScanBlock / 64];
    __shared__ uint32_t s_nc[3];
    const uint32_t t = threadIdx.x;
    if (t < 3) s_nc[t] = P.ctl[kCtlNew + t];
    __syncthreads();
    if (t < 3) {
        P.ctl[kCtlCreate + t] = s_nc[t];
        P.ctl[kCtlNew + t] = 0;
    }
    const uint32_t ntiles = (P.cn + kNBlock - 1) / kNBlock, per = P.v.nblk + 1u;
    for (uint32_t p = 0; p < 3; p++) {  // uniform
        const uint32_t nc = s_nc[p];
        if (!nc) continue;
        scan_in_place(P.tile_cnt + p * kNatTiles, ntiles, s_w);
        uint32_t* seg = P.seg + p * (per + 1u);
        const uint32_t nfree = scan_in_place(seg, per, s_w);
        if (t == 0) seg[per] = nfree;
        __syncthreads();  // the prefix is the block's to read
        if (t == 0) {
            const uint32_t c = P.v.cursor[p], m = nc < nfree ? nc : nfree;
            P.ctl[kCtlCur0 + p] = c;
            if (m) P.v.cursor[p] = (nat_select(P.v.used + p * P.v.W, seg, m - 1u, c, P.v.E, P.v.nblk) + 1u) % P.v.E;
        }
    }
}

__global__ __launch_bounds__(kNBlock) void nat_alloc_kernel(NParams P) {
    __shared__ uint32_t s_w[kNBlock / 64][3];
    if (!(P.ctl[kCtlCreate] | P.ctl[kCtlCreate + 1] | P.ctl[kCtlCreate + 2])) return;  // uniform over the grid
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
    const uint32_t r = blockIdx.x * kNBlock + t;
    const bool in = r < P.cn;
    const uint32_t slot = in ? P.slot_scr[r] : kNatNoSlot;
    uint64_t key = 0;
    uint32_t p = 3, wr = 0;
    if (slot != kNatNoSlot) {
        key = P.v.fkey[slot];
        p = nat_key_p(key);
    }
    for (uint32_t q = 0; q < 3; q++) {
        const uint64_t m = __ballot(p == q);
        if (p == q) wr = (uint32_t)__popcll((unsigned long long)(m & ((1ull << lane) - 1ull)));
        if (lane == 0) s_w[wv][q] = (uint32_t)__popcll((unsigned long long)m);
    }
    __syncthreads();
    uint32_t ent = PKT_NAT_NONE;
    if (slot != kNatNoSlot) {
        uint32_t j = P.tile_cnt[p * kNatTiles + blockIdx.x] + wr;
        for (uint32_t w = 0; w < wv; w++) j += s_w[w][p];
        P.v.ffirst[slot] = ~0u;  // the slot's other packets compare it with their own index: neither value is theirs
        const uint32_t* pre = P.seg + p * (P.v.nblk + 2u);
        if (j < pre[P.v.nblk + 1u]) {
            const uint32_t e = nat_select(P.v.used + p * P.v.W, pre, j, P.ctl[kCtlCur0 + p], P.v.E, P.v.nblk);
            if (e < P.v.E) {  // (always, for j below the free count)
                ent = p * P.v.E + e;
                P.v.rev[ent] = key;
                P.v.seen[ent] = P.c.now;
                P.v.fval[slot] = ent;
                if (P.c.created) P.c.created[P.c0 + r] = 1;
            }
        }
    }
    if (in) P.slot_scr[r] = ent;  // for nat_mark_kernel
}

__global__ __launch_bounds__(kNBlock) void nat_mark_kernel(NParams P) {
    if (!(P.ctl[kCtlCreate] | P.ctl[kCtlCreate + 1] | P.ctl[kCtlCreate + 2])) return;
    const uint32_t r = blockIdx.x * kNBlock + threadIdx.x;
    if (r >= P.cn) return;
    const uint32_t ent = P.slot_scr[r];
    if (ent == PKT_NAT_NONE) return;
    const uint32_t p = ent / P.v.E, e = ent - p * P.v.E;
    __hip_atomic_fetch_or(&P.v.used[p * P.v.W + (e >> 5)], 1u << (e & 31u), NAT_RLX);
}

__global__ __launch_bounds__(kNBlock) void nat_xlate_kernel(NParams P) {
    __shared__ uint32_t s_hits[PKT_NAT_STATUS_COUNT];
    __shared__ unsigned long long s_bytes[PKT_NAT_STATUS_COUNT];
    const uint32_t t = threadIdx.x, lane = t & 63u;
    const bool counting = P.c.hits || P.c.bytes;  // uniform over the grid
    if (counting) {
        if (t < PKT_NAT_STATUS_COUNT) {
            s_hits[t] = 0;
            s_bytes[t] = 0;
        }
        __syncthreads();
    }
    const bool write = !(P.c.flags & PKT_NAT_NO_WRITE);
    const uint32_t ntiles = (uint32_t)((P.c.n + kNBlock - 1) / kNBlock);
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {  // uniform
        const uint64_t i = (uint64_t)tile * kNBlock + t;
        const bool act = i < P.c.n;
        uint32_t st = PKT_NAT_SKIPPED, len = 0;
        if (act) {
            uint64_t off = pkt_off(P.c.src, i);
            len = pkt_len(P.c.src, i, off);
            const uint32_t d = nat_dir(P.c, i);
            uint32_t ent = PKT_NAT_NONE;
            if (d < 2u) {
                const NatPkt k = classify(P.c, i, d, off, len);
                st = k.st;
                if (st == PKT_NAT_OK) {
                    if (d == PKT_NAT_OUT) {
                        const uint32_t slot = nat_find(P.v.fkey, P.v.slots, k.key);
                        if (slot == kNatNoSlot) {
                            st = PKT_NAT_TABLE_FULL;
                        } else {
                            ent = P.v.fval[slot];
                            if (ent == PKT_NAT_NONE) st = PKT_NAT_EXHAUSTED;
                        }
                    } else {
                        ent = nat_in_find(P.v, k.key, st);
                    }
                }
                if (st == PKT_NAT_OK) {
                    if (!(ent & PKT_NAT_STATIC) && __hip_atomic_load(&P.v.seen[ent], NAT_RLX) < P.c.now)
                        __hip_atomic_fetch_max(&P.v.seen[ent], P.c.now, NAT_RLX);
                    if (write) {
                        uint8_t* pkt = const_cast<uint8_t*>(P.c.src.slab) + off;
                        nat_rewrite(pkt + k.ipo, pkt + k.l4o, k.p, d, nat_target(P.v, ent, k.p, d));
                    }
                }
            }
            if (P.c.status) P.c.status[i] = (uint8_t)st;
            if (P.c.entry) P.c.entry[i] = ent;
        }
        // ---- counters: the wave's lanes of one status add once (fwd_kernel's groups)
        if (counting) {
            uint64_t todo = __ballot(act);
            for (uint32_t g = 0; g < kWaveGroups && todo; g++) {  // uniform
                const uint32_t lead = (uint32_t)__ffsll((unsigned long long)todo) - 1u;
                const uint32_t sl = lane_value(st, lead);
                const bool mine = act && st == sl;
                const uint64_t m = __ballot(mine);
                uint32_t sum = mine ? len : 0u;
#pragma unroll
                for (uint32_t x = 32; x; x >>= 1) sum += (uint32_t)__shfl_xor((int)sum, (int)x, 64);
                if (lane == lead) {
                    atomicAdd(&s_hits[sl], (uint32_t)__popcll((unsigned long long)m));
                    atomicAdd(&s_bytes[sl], (unsigned long long)sum);
                }
                todo &= ~m;
            }
            if ((todo >> lane) & 1ull) {
                atomicAdd(&s_hits[st], 1u);
                atomicAdd(&s_bytes[st], (unsigned long long)len);
            }
        }
    }
    if (!counting) return;
    __syncthreads();
    if (t < PKT_NAT_STATUS_COUNT) {
        const uint32_t h = s_hits[t];
        const uint64_t bsum = s_bytes[t];
        if (P.c.hits && h) __hip_atomic_fetch_add(P.c.hits + t, (uint64_t)h, NAT_RLX);
        if (P.c.bytes && bsum) __hip_atomic_fetch_add(P.c.bytes + t, bsum, NAT_RLX);
    }
}

// ---- housekeeping
struct EParams {
    NatView v;
    uint32_t now, idle[3];
    uint32_t* ctl;
    uint64_t* fkey;  // the buffer rebuilt into
    uint32_t* fval;
    uint32_t nent;   // 3 * E, or 0: the statics alone (pkt_nat_clear)
};

__global__ __launch_bounds__(kNBlock) void nat_expire_kernel(EParams P) {
    __shared__ uint32_t s_gone;
    if (threadIdx.x == 0) s_gone = 0;
    __syncthreads();
    const uint32_t ent = blockIdx.x * kNBlock + threadIdx.x;
    bool gone = false;
    if (ent < P.nent) {
        const uint32_t p = ent / P.v.E, e = ent - p * P.v.E;
        gone = P.v.rev[ent] && P.idle[p] && (uint64_t)P.v.seen[ent] + P.idle[p] <= P.now;
        if (gone) {
            P.v.rev[ent] = 0;
            __hip_atomic_fetch_and(&P.v.used[p * P.v.W + (e >> 5)], ~(1u << (e & 31u)), NAT_RLX);
        }
    }
    const uint64_t m = __ballot(gone);
    if ((threadIdx.x & 63u) == 0 && m) atomicAdd(&s_gone, (uint32_t)__popcll((unsigned long long)m));
    __syncthreads();
    if (threadIdx.x == 0 && s_gone) __hip_atomic_fetch_add(&P.ctl[kCtlExpired], s_gone, NAT_RLX);
}

// thread g < nstatic: static g; the threads behind them: entry g - nstatic, where it is mapped.  The buffer has room:
// it held them all before.
__global__ __launch_bounds__(kNBlock) void nat_rebuild_kernel(EParams P) {
    const uint32_t g = blockIdx.x * kNBlock + threadIdx.x;
    uint64_t key = 0;
    uint32_t val = PKT_NAT_NONE;
    if (g < P.v.nstatic) {
        key = P.v.st_in[g];
        val = PKT_NAT_STATIC | g;
    } else if (g - P.v.nstatic < P.nent) {
        key = P.v.rev[g - P.v.nstatic];
        val = g - P.v.nstatic;
    }
    if (!key) return;
    const uint32_t slot = nat_claim(P.fkey, P.v.slots, key);
    if (slot != kNatNoSlot) P.fval[slot] = val;
}

pkt_ctx* ctx_of(pkt_nat* t) { return static_cast<pkt_ctx*>(t->ctx); }

int nat_hip_fail(pkt_nat* t, hipError_t e, const char* what) {
    t->err = std::string(what) + ": " + hipGetErrorString(e);
    return hip_fail(ctx_of(t), e, what);
}

void nat_launch_rebuild(pkt_nat* t, uint64_t* fkey, uint32_t* fval, uint32_t nent, hipStream_t s) {
    EParams E{};
    E.v = t->v;
    E.ctl = t->ctl;
    E.fkey = fkey;
    E.fval = fval;
    E.nent = nent;
    const uint32_t threads = t->v.nstatic + nent;
    if (threads) hipLaunchKernelGGL(nat_rebuild_kernel, dim3((threads + kNBlock - 1) / kNBlock), dim3(kNBlock), 0, s, E);
}

int nat_dev_batch(pkt_nat* t, const NatCall& c, void* stream) {
    hipError_t e = hipSetDevice(t->device);
    if (e != hipSuccess) return nat_hip_fail(t, e, "hipSetDevice");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    NParams P{};
    P.v = t->v;
    P.c = c;
    P.slot_scr = t->slot_scr;
    P.tile_cnt = t->tile_cnt;
    P.seg = t->seg;
    P.ctl = t->ctl;
    const dim3 blk(kNBlock);
    for (uint64_t c0 = 0; c0 < c.n; c0 += kNatChunk) {
        P.c0 = c0;
        P.cn = (uint32_t)(c.n - c0 < kNatChunk ? c.n - c0 : kNatChunk);
        const dim3 tiles((P.cn + kNBlock - 1) / kNBlock);
        hipLaunchKernelGGL(nat_claim_kernel, tiles, blk, 0, s, P);
        hipLaunchKernelGGL(nat_rank_kernel, tiles, blk, 0, s, P);
        hipLaunchKernelGGL(nat_free_kernel, dim3((3u * (t->v.nblk + 1u) + kNBlock - 1) / kNBlock), blk, 0, s, P);
        hipLaunchKernelGGL(nat_scan_kernel, dim3(1), dim3(kScanBlock), 0, s, P);
        hipLaunchKernelGGL(nat_alloc_kernel, tiles, blk, 0, s, P);
        hipLaunchKernelGGL(nat_mark_kernel, tiles, blk, 0, s, P);
    }
    const uint64_t tiles = (c.n + kNBlock - 1) / kNBlock;
    const dim3 grid((unsigned)((c.hits || c.bytes) && tiles > kCountBlocks ? kCountBlocks : tiles));
    hipLaunchKernelGGL(nat_xlate_kernel, grid, blk, 0, s, P);
    if ((e = hipGetLastError()) != hipSuccess) return nat_hip_fail(t, e, "pkt_nat_batch launch");
    return PKT_SUCCESS;
}

int nat_dev_expire(pkt_nat* t, uint32_t now, const uint32_t idle[3], uint64_t* n_expired) {
    hipError_t e = hipSetDevice(t->device);
    if (e == hipSuccess) e = hipDeviceSynchronize();  // blocking: the queued calls on every stream are over
    if (e != hipSuccess) return nat_hip_fail(t, e, "pkt_nat_expire");
    const NatView& v = t->v;
    EParams E{};
    E.v = v;
    E.now = now;
    for (int p = 0; p < 3; p++) E.idle[p] = idle[p];
    E.ctl = t->ctl;
    E.nent = 3u * v.E;
    (void)hipMemsetAsync(t->ctl + kCtlExpired, 0, sizeof(uint32_t), nullptr);
    hipLaunchKernelGGL(nat_expire_kernel, dim3((E.nent + kNBlock - 1) / kNBlock), dim3(kNBlock), 0, nullptr, E);
    (void)hipMemsetAsync(t->fkey2, 0, v.slots * sizeof(uint64_t), nullptr);
    (void)hipMemsetAsync(t->fval2, 0xFF, v.slots * sizeof(uint32_t), nullptr);
    (void)hipMemsetAsync(t->ffirst2, 0xFF, v.slots * sizeof(uint32_t), nullptr);
    nat_launch_rebuild(t, t->fkey2, t->fval2, E.nent, nullptr);
    uint32_t gone = 0;
    e = hipMemcpy(&gone, t->ctl + kCtlExpired, sizeof(gone), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return nat_hip_fail(t, e, "pkt_nat_expire");
    std::swap(t->v.fkey, t->fkey2);
    std::swap(t->v.fval, t->fval2);
    std::swap(t->v.ffirst, t->ffirst2);
    if (n_expired) *n_expired = gone;
    return PKT_SUCCESS;
}

int nat_dev_fetch(pkt_nat* t, std::vector<uint64_t>* rev, std::vector<uint32_t>* seen, std::vector<uint32_t>* used) {
    hipError_t e = hipSetDevice(t->device);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    const NatView& v = t->v;
    if (e == hipSuccess && rev) {
        rev->resize(3ull * v.E);
        e = hipMemcpy(rev->data(), v.rev, rev->size() * sizeof(uint64_t), hipMemcpyDeviceToHost);
    }
    if (e == hipSuccess && seen) {
        seen->resize(3ull * v.E);
        e = hipMemcpy(seen->data(), v.seen, seen->size() * sizeof(uint32_t), hipMemcpyDeviceToHost);
    }
    if (e == hipSuccess && used) {
        used->resize(3ull * v.W);
        e = hipMemcpy(used->data(), v.used, used->size() * sizeof(uint32_t), hipMemcpyDeviceToHost);
    }
    return e == hipSuccess ? PKT_SUCCESS : nat_hip_fail(t, e, "pkt_nat_export / pkt_nat_count");
}

int nat_dev_put(pkt_nat* t, pkt_nat_record_t* dst, const pkt_nat_record_t* src, uint64_t count) {
    const hipError_t e = hipMemcpy(dst, src, count * sizeof(pkt_nat_record_t), hipMemcpyHostToDevice);
    return e == hipSuccess ? PKT_SUCCESS : nat_hip_fail(t, e, "pkt_nat_export");
}

int nat_dev_clear(pkt_nat* t, void* stream) {
    hipError_t e = hipSetDevice(t->device);
    if (e != hipSuccess) return nat_hip_fail(t, e, "hipSetDevice");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const NatView& v = t->v;
    (void)hipMemsetAsync(v.fkey, 0, v.slots * sizeof(uint64_t), s);
    (void)hipMemsetAsync(v.fval, 0xFF, v.slots * sizeof(uint32_t), s);
    (void)hipMemsetAsync(v.ffirst, 0xFF, v.slots * sizeof(uint32_t), s);
    (void)hipMemsetAsync(v.rev, 0, 3ull * v.E * sizeof(uint64_t), s);
    (void)hipMemsetAsync(v.seen, 0, 3ull * v.E * sizeof(uint32_t), s);
    (void)hipMemsetAsync(v.used, 0, 3ull * v.W * sizeof(uint32_t), s);
    (void)hipMemsetAsync(v.cursor, 0, 4 * sizeof(uint32_t), s);
    (void)hipMemsetAsync(t->ctl, 0, kCtlWords * sizeof(uint32_t), s);
    nat_launch_rebuild(t, v.fkey, v.fval, 0, s);
    if ((e = hipGetLastError()) != hipSuccess) return nat_hip_fail(t, e, "pkt_nat_clear");
    return PKT_SUCCESS;
}

int nat_dev_destroy(pkt_nat* t) {
    (void)hipSetDevice(t->device);
    return hipFree(t->dev_buf) == hipSuccess ? PKT_SUCCESS : PKT_ERR_HIP;
}

void nat_dev_refused(pkt_nat* t) {
    if (t->ctx) ctx_of(t)->err = t->err;
}

const NatDevOps kDevOps = {nat_dev_batch, nat_dev_expire, nat_dev_fetch, nat_dev_put, nat_dev_clear, nat_dev_destroy, nat_dev_refused};

}  // namespace

extern "C" int pkt_nat_create(pkt_ctx_t* ctx, const uint8_t* pool, uint32_t naddr, uint32_t port_lo, uint32_t port_hi,
                              uint64_t slots, const pkt_nat_static_t* statics, uint32_t nstatic, pkt_nat_t** out) {
    if (!ctx || !out) return fail(ctx, PKT_ERR_INVALID_ARG, "pkt_nat_create: null argument");
    *out = nullptr;
    pkt_nat* t = new pkt_nat;
    if (const char* msg = nat_create_error(pool, naddr, port_lo, port_hi, slots, statics, nstatic, t->img)) {
        ctx->err = std::string("pkt_nat_create: ") + msg;
        delete t;
        return PKT_ERR_INVALID_ARG;
    }
    t->ops = &kDevOps;
    t->ctx = ctx;
    t->device = ctx->device;
    const NatImage& g = t->img;
    NatView& v = t->v;
    nat_view_config(v, g);
    // one allocation: every piece starts 16-byte aligned, the 64-bit arrays first
    uint64_t at = 0;
    auto piece = [&](uint64_t bytes) {
        const uint64_t o = at;
        at += round16(bytes);
        return o;
    };
    const uint64_t ents = 3ull * g.E, ns = g.nstatic;
    const uint64_t o_fkey = piece(slots * 8), o_fkey2 = piece(slots * 8), o_rev = piece(ents * 8);
    const uint64_t o_sti = piece(ns * 8), o_sto = piece(ns * 8), o_sk = piece(ns * 8), o_ps = piece(g.naddr * 8ull);
    const uint64_t o_fval = piece(slots * 4), o_fval2 = piece(slots * 4), o_ff = piece(slots * 4), o_ff2 = piece(slots * 4);
    const uint64_t o_seen = piece(ents * 4), o_used = piece(3ull * g.W * 4), o_cur = piece(16), o_pool = piece(g.naddr * 4ull);
    const uint64_t o_si = piece(ns * 4), o_scr = piece(kNatChunk * 4), o_tile = piece(3ull * kNatTiles * 4);
    const uint64_t o_seg = piece(3ull * (g.nblk + 2) * 4), o_ctl = piece(kCtlWords * 4);
    hipError_t e = hipSetDevice(ctx->device);
    uint8_t* base = nullptr;
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&base), at);
    if (e != hipSuccess) {
        delete t;
        return hip_fail(ctx, e, "pkt_nat_create");
    }
    t->dev_buf = base;
    auto p64 = [&](uint64_t o) { return reinterpret_cast<uint64_t*>(base + o); };
    auto p32 = [&](uint64_t o) { return reinterpret_cast<uint32_t*>(base + o); };
    v.fkey = p64(o_fkey), t->fkey2 = p64(o_fkey2), v.rev = p64(o_rev);
    v.st_in = p64(o_sti), v.st_out = p64(o_sto), v.sin_key = p64(o_sk), v.pool_sorted = p64(o_ps);
    v.fval = p32(o_fval), t->fval2 = p32(o_fval2), v.ffirst = p32(o_ff), t->ffirst2 = p32(o_ff2);
    v.seen = p32(o_seen), v.used = p32(o_used), v.cursor = p32(o_cur), v.pool = p32(o_pool), v.sin_idx = p32(o_si);
    t->slot_scr = p32(o_scr), t->tile_cnt = p32(o_tile), t->seg = p32(o_seg), t->ctl = p32(o_ctl);
    auto up = [&](uint64_t o, const void* src, uint64_t bytes) {
        if (e == hipSuccess && bytes) e = hipMemcpy(base + o, src, bytes, hipMemcpyHostToDevice);
    };
    up(o_sti, g.st_in.data(), ns * 8), up(o_sto, g.st_out.data(), ns * 8), up(o_sk, g.sin_key.data(), ns * 8);
    up(o_ps, g.pool_sorted.data(), g.naddr * 8ull), up(o_pool, g.pool.data(), g.naddr * 4ull), up(o_si, g.sin_idx.data(), ns * 4);
    int rc = e == hipSuccess ? nat_dev_clear(t, nullptr) : hip_fail(ctx, e, "pkt_nat_create");
    if (rc == PKT_SUCCESS && (e = hipDeviceSynchronize()) != hipSuccess) rc = hip_fail(ctx, e, "pkt_nat_create");
    if (rc != PKT_SUCCESS) {
        (void)hipFree(base);
        delete t;
        return rc;
    }
    *out = t;
    return PKT_SUCCESS;
}
