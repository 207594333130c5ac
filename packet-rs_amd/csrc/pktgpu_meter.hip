// pktgpu_meter.hip — pkt_meter_create and the device half of pkt_meter_*: srTCM / trTCM policers over a batch.
// The model is a sequential walk per meter; the kernels reproduce it exactly.  No lane waits for another, every loop is
// bounded by the chunk's packets, the kernel boundaries publish, and nothing but the call's integer hits / bytes is
// added to global memory, so the result is the same from run to run.  One call, per chunk of 2^20 packets (the state
// carries over, so a chunk is a call of its own):
//   group   an LSD radix sort of the METERED packets' (meter, index) pairs by meter, 8 bits a pass, ceil(bits / 8)
//           passes (one for up to 256 meters).  A pass is pkt_dispatch_batch's stable partition: a tile of 2048 items,
//           a block of 4 waves, wave w owning items [512 w, 512 w + 512) 64 at a time, so that (tile, wave, round,
//           lane) order is source order.  meter_count_kernel: the lanes of one digit find each other by ballots and
//           the group's lowest lane adds to the wave's LDS histogram; the tile's counts go to cnt[digit][tile].
//           meter_scan_kernel: one block, the exclusive prefix in place; the total (the metered packets, m) goes to
//           ctl[0].  meter_place_kernel: histograms again, each wave's first position per digit, the ranks, the pair
//           stored.  Pass 0 reads the caller's meter / select arrays and drops the unmetered packets; later passes
//           read the m pairs of the pass before.
//   walk    meter_walk_kernel, a thread per sorted position.  A run is a meter's packets, in index order (the sort
//           is stable).  The head of a run shorter than 64 walks it alone.  The head of a longer run (at most one per
//           wave: such a run covers 64 positions from its head) has its wave walk it, 64 packets a step: the lanes
//           gather cost, time and colour, a max-scan of the times gives every packet's dt and so its gains (they do
//           not depend on the state), and if every packet of the step turns out green the step is one scan per
//           bucket (green_step); otherwise every lane takes the 64 packets in order from the lanes that hold them
//           (readlane: adds, compares and selects, no multiplication) and keeps its own packet's colour.  The
//           owner loads the meter's state once and stores it once.
//   emit    meter_emit_kernel, a lane per packet of the chunk: colour, pass, marked and the DSCP stores
//           (meter_emit, pktgpu_meter.hpp), and the call's hits / bytes, summed per wave and block first.
// PKTGPU_METER_GREEN_STEP=0 compiles the green step out (the A/B of DESIGN.md section 4 and profiles/meter).  No
// all-red shortcut is built.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "pktgpu_ctx.hpp"
#include "pktgpu_meter.hpp"

namespace {

constexpr uint32_t kMBlock = 256, kMWaves = 4, kMRounds = 8;
constexpr uint32_t kMTile = kMBlock * kMRounds;  // 2048 items
constexpr uint32_t kMeterChunk = 1u << 20;
constexpr uint32_t kMeterTiles = kMeterChunk / kMTile;
constexpr uint32_t kDigits = 256, kNoDigit = 256;
constexpr uint32_t kScanBlock = 1024, kScanPer = 16;  // the scan's block, and the elements a thread takes per pass
constexpr uint32_t kCountBlocks = 1280;  // fwd_kernel's cap on a counting launch's grid
constexpr uint32_t kCtlWords = 4;

#define METER_RLX __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

struct MParams {
    MeterView v;
    MeterCall c;
    uint64_t c0;      // the chunk's first packet
    uint32_t cn;      // its packets
    uint32_t ntiles;  // of the chunk
    uint32_t pass, shift, nbits;  // the radix pass, its digit's first bit and its bits (0..8)
    const uint32_t* key_in;  // passes above 0, and the walk: the sorted pairs
    const uint32_t* idx_in;
    uint32_t* key_out;
    uint32_t* idx_out;
    uint32_t* cnt;
    uint32_t* ctl;
    uint8_t* col;
};

// The lanes of the wave that are active and hold the same digit as this one (itself included).
__device__ __forceinline__ uint64_t peers_of(uint32_t d, bool act, uint32_t nbits) {
    uint64_t m = __ballot(act);
    for (uint32_t k = 0; k < nbits; k++) {  // uniform
        const bool bit = (d >> k) & 1u;
        const uint64_t bal = __ballot(bit);
        m &= bit ? bal : ~bal;
    }
    return m;
}

// The tile's items of this lane: round r = position tile * kMTile + wave * 512 + r * 64 + lane; dg = kNoDigit where
// there is none.
__device__ __forceinline__ void load_items(const MParams& P, uint32_t tile, uint32_t wv, uint32_t lane,
                                           uint32_t key[kMRounds], uint32_t idx[kMRounds], uint32_t dg[kMRounds]) {
    const uint32_t p0 = tile * kMTile + wv * (kMTile / kMWaves) + lane;
    const uint32_t mask = (1u << P.nbits) - 1u;
    const uint32_t m = P.pass ? P.ctl[0] : P.cn;
#pragma unroll
    for (uint32_t r = 0; r < kMRounds; r++) {
        const uint32_t p = p0 + 64u * r;
        key[r] = ~0u;
        idx[r] = p;
        if (p < m) {
            if (P.pass) {
                key[r] = P.key_in[p];
                idx[r] = P.idx_in[p];
            } else {
                key[r] = meter_of(P.c, P.v.nmeters, P.c0 + p);
            }
        }
        dg[r] = key[r] != ~0u ? (key[r] >> P.shift) & mask : kNoDigit;
    }
}

// The wave's histogram of its 512 items into its own LDS row (zeroed by the caller, behind a barrier).  Distinct groups
// hold distinct digits, so the leaders' read-modify-writes never meet.
__device__ __forceinline__ void wave_hist(const uint32_t dg[kMRounds], uint32_t nbits, uint32_t lane, uint32_t* h) {
#pragma unroll
    for (uint32_t r = 0; r < kMRounds; r++) {
        const bool act = dg[r] != kNoDigit;
        const uint64_t peers = peers_of(dg[r], act, nbits);
        if (act && (uint32_t)__ffsll((unsigned long long)peers) - 1u == lane) h[dg[r]] += (uint32_t)__popcll(peers);
        wave_sync();
    }
}

__global__ __launch_bounds__(kMBlock) void meter_count_kernel(MParams P) {
    __shared__ uint32_t s_h[kMWaves][kDigits];
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6, tile = blockIdx.x;
    for (uint32_t b = t; b < kMWaves * kDigits; b += kMBlock) (&s_h[0][0])[b] = 0;
    uint32_t key[kMRounds], idx[kMRounds], dg[kMRounds];
    load_items(P, tile, wv, lane, key, idx, dg);
    __syncthreads();
    wave_hist(dg, P.nbits, lane, s_h[wv]);
    __syncthreads();
    for (uint32_t b = t; b < kDigits; b += kMBlock)
        P.cnt[b * P.ntiles + tile] = s_h[0][b] + s_h[1][b] + s_h[2][b] + s_h[3][b];
}

// cnt[0 .. 256 * ntiles) becomes its exclusive prefix; the sum, the chunk's metered packets, goes to ctl[0]
__global__ __launch_bounds__(kScanBlock) void meter_scan_kernel(MParams P) {
    __shared__ uint64_t s_w[kScanBlock / 64];
    const uint32_t total = kDigits * P.ntiles;  // a multiple of 4; cnt is 16-byte aligned
    uint4* cnt4 = reinterpret_cast<uint4*>(P.cnt);
    uint64_t carry = 0;
    for (uint32_t base = 0; base < total; base += kScanBlock * kScanPer) {  // uniform: a thread takes 16 elements a pass
        const uint32_t e0 = base + threadIdx.x * kScanPer;
        uint4 v[kScanPer / 4];
        uint64_t mine = 0;
#pragma unroll
        for (uint32_t q = 0; q < kScanPer / 4; q++) {
            v[q] = e0 + 4u * q < total ? cnt4[(e0 >> 2) + q] : make_uint4(0, 0, 0, 0);
            mine += (uint64_t)v[q].x + v[q].y + v[q].z + v[q].w;
        }
        uint64_t sum;
        uint32_t at = (uint32_t)(carry + block_excl_scan<kScanBlock / 64>(mine, s_w, sum));  // at most 2^20
#pragma unroll
        for (uint32_t q = 0; q < kScanPer / 4; q++) {
            const uint4 o = make_uint4(at, at + v[q].x, at + v[q].x + v[q].y, at + v[q].x + v[q].y + v[q].z);
            at = o.w + v[q].w;
            if (e0 + 4u * q < total) cnt4[(e0 >> 2) + q] = o;
        }
        carry += sum;
    }
    if (threadIdx.x == 0) P.ctl[0] = (uint32_t)carry;
}

__global__ __launch_bounds__(kMBlock) void meter_place_kernel(MParams P) {
    __shared__ uint32_t s_h[kMWaves][kDigits];
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6, tile = blockIdx.x;
    for (uint32_t b = t; b < kMWaves * kDigits; b += kMBlock) (&s_h[0][0])[b] = 0;
    uint32_t key[kMRounds], idx[kMRounds], dg[kMRounds];
    load_items(P, tile, wv, lane, key, idx, dg);
    __syncthreads();
    wave_hist(dg, P.nbits, lane, s_h[wv]);
    __syncthreads();
    // the waves' counts -> each wave's first position in each digit
    for (uint32_t b = t; b < kDigits; b += kMBlock) {
        uint32_t at = P.cnt[b * P.ntiles + tile];
#pragma unroll
        for (uint32_t w = 0; w < kMWaves; w++) {
            const uint32_t c = s_h[w][b];
            s_h[w][b] = at;
            at += c;
        }
    }
    __syncthreads();
    uint32_t* h = s_h[wv];
#pragma unroll
    for (uint32_t r = 0; r < kMRounds; r++) {
        const bool act = dg[r] != kNoDigit;
        const uint64_t peers = peers_of(dg[r], act, P.nbits);
        const uint32_t first = act ? h[dg[r]] : 0u;
        const uint32_t pos = first + (uint32_t)__popcll(peers & ((1ull << lane) - 1ull));
        wave_sync();  // the group has read its count before its lowest lane moves it on
        if (act && (uint32_t)__ffsll((unsigned long long)peers) - 1u == lane) h[dg[r]] = first + (uint32_t)__popcll(peers);
        wave_sync();
        if (act && pos < P.cn) {  // (always: the counts of all tiles sum to at most cn)
            P.key_out[pos] = key[r];
            P.idx_out[pos] = idx[r];
        }
    }
}

// what step 2 and the colour-aware rule read of the chunk's packet at `pos`
struct MItem {
    uint64_t B, t;
    uint32_t len, ic;
};
__device__ __forceinline__ MItem load_item(const MParams& P, uint32_t pos, uint32_t w) {
    const uint64_t i = P.c0 + pos;
    const uint64_t off = pkt_off(P.c.src, i);
    MItem it;
    it.len = pkt_len(P.c.src, i, off);
    it.B = meter_cost(it.len, P.v.adjust);
    it.t = P.c.time ? P.c.time[i] : P.c.now;
    it.ic = meter_in_color(P.c, w, i);
    return it;
}

// lane j's value, j uniform over the wave
__device__ __forceinline__ uint32_t lane32(uint32_t v, uint32_t j) {
    return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)__builtin_amdgcn_readfirstlane(j));
}
__device__ __forceinline__ uint64_t lane64(uint64_t v, uint32_t j) {
    return (uint64_t)lane32((uint32_t)(v >> 32), j) << 32 | lane32((uint32_t)v, j);
}

// The levels of a bucket after each lane's packet if every packet of the step pays from it: refill-then-pay is
// x -> min(x + gain, cap) - cost = min(x + A, K) with A = gain - cost, K = cap - cost, and such maps compose to
// (A1 + A2, min(K1 + A2, K2)): an inclusive scan of the pairs, then the bucket's level before the step put in.
// gain <= cap and cost <= cap + 1 (the caller's clamps: a cost above the cap cannot be paid whatever the level), cap <
// 2^56, so 64 lanes' sums stay below 2^63.  A lane past the run holds (0, cap), the identity on [0, cap].
__device__ __forceinline__ int64_t levels_if_paid(uint64_t level0, uint64_t gain, uint64_t cost, uint64_t cap, bool valid, uint32_t lane) {
    int64_t A = valid ? (int64_t)gain - (int64_t)cost : 0, K = valid ? (int64_t)cap - (int64_t)cost : (int64_t)cap;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const int64_t Ay = __shfl_up(A, d, 64), Ky = __shfl_up(K, d, 64);
        if (lane >= d) {
            K = Ky + A < K ? Ky + A : K;
            A += Ay;
        }
    }
    const int64_t x = (int64_t)level0 + A;
    return x < K ? x : K;
}

#ifndef PKTGPU_METER_GREEN_STEP
#define PKTGPU_METER_GREEN_STEP 1
#endif

// The shortcut of a wave's step: if every packet of it turns out green, the step is one scan per bucket.  The levels
// are worked out as if every packet were green; if none is negative the assumption holds by induction (the first
// packet that is not green would see exactly the level the scan gives it, and that level is negative) and `run` moves
// on by the whole step.  Otherwise nothing is touched and the caller walks the step.
__device__ __forceinline__ bool green_step(MeterRun& run, const MeterCfg& g, bool tr, bool valid, uint32_t cnt, uint32_t lane,
                                           const MItem& it, uint64_t a, uint64_t gx) {
    const uint32_t ic = it.ic;
    if (__ballot(valid && ic != PKT_METER_GREEN)) return false;  // uniform
    const uint64_t ac = a < g.ccap ? a : g.ccap;  // what the committed bucket can take of it
    const int64_t lc = levels_if_paid(run.s.c, ac, it.B <= g.ccap ? it.B : g.ccap + 1u, g.ccap, valid, lane);
    int64_t lx = 0;
    if (tr) lx = levels_if_paid(run.s.x, gx, it.B <= g.xcap ? it.B : g.xcap + 1u, g.xcap, valid, lane);  // uniform
    if (__ballot(valid && (lc < 0 || lx < 0))) return false;  // uniform
    if (cnt == 0) return true;
    uint64_t x = lane64((uint64_t)lx, cnt - 1u);
    if (!tr) {
        // srTCM: the excess bucket only gains in such a step, what the committed one could not take, so it is capped once
        int64_t before = __shfl_up(lc, 1, 64);
        if (lane == 0) before = (int64_t)run.s.c;
        const uint64_t up = (uint64_t)before + a;  // a <= ccap + xcap
        uint64_t spill = valid && up > g.ccap ? up - g.ccap : 0ull;
#pragma unroll
        for (uint32_t d = 32; d; d >>= 1) spill += __shfl_xor(spill, d, 64);  // below 64 * 2^57
        x = run.s.x + spill;
        x = x < g.xcap ? x : g.xcap;
    }
    uint32_t len = valid ? it.len : 0u;
#pragma unroll
    for (uint32_t d = 32; d; d >>= 1) len += (uint32_t)__shfl_xor((int)len, (int)d, 64);
    run.s.c = lane64((uint64_t)lc, cnt - 1u);
    run.s.x = x;
    run.pk[0] += cnt;
    run.by[0] += len;
    return true;
}

__global__ __launch_bounds__(kMBlock) void meter_walk_kernel(MParams P) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t m = P.ctl[0];
    const uint32_t p = blockIdx.x * kMBlock + threadIdx.x;
    uint32_t k = 0;
    bool head = false, lng = false;
    if (p < m) {
        k = P.key_in[p];
        head = p == 0 || P.key_in[p - 1] != k;
        lng = head && p + 63u < m && P.key_in[p + 63u] == k;  // sorted: the run has 64 packets or more
    }
    if (head && !lng) {  // a lane per run
        const MeterCfg g = P.v.cfg[k];
        const uint32_t w = P.v.word[k];
        MeterRun run = meter_run_load(P.v.st[k]);
        for (uint32_t q = p; q < m && q < p + 63u && P.key_in[q] == k; q++) {
            const uint32_t pos = P.idx_in[q];
            const MItem it = load_item(P, pos, w);
            P.col[pos] = (uint8_t)meter_run_packet(run, g, w, it.t, it.B, it.ic, it.len);
        }
        meter_run_store(P.v.st[k], run);
    }
    const uint64_t lm = __ballot(lng);
    if (!lm) return;  // uniform over the wave
    // a wave per run: the one long run that starts in this wave's 64 positions
    const uint32_t lead = (uint32_t)__ffsll((unsigned long long)lm) - 1u;
    const uint32_t p0 = p - lane + lead;
    const uint32_t k0 = (uint32_t)__builtin_amdgcn_readlane((int)k, (int)__builtin_amdgcn_readfirstlane(lead));
    const MeterCfg g = P.v.cfg[k0];
    const uint32_t w = P.v.word[k0];
    const bool tr = w & 1u;
    MeterRun run = meter_run_load(P.v.st[k0]);  // every lane holds it and moves it on alike; lane 0 stores it
    for (uint32_t q0 = p0; q0 < m; q0 += 64u) {  // uniform
        const uint32_t q = q0 + lane;
        const bool valid = q < m && P.key_in[q] == k0;  // a prefix of the lanes
        uint32_t pos = 0;
        MItem it{0, 0, 0, PKT_METER_GREEN};
        if (valid) {
            pos = P.idx_in[q];
            it = load_item(P, pos, w);
        }
        const uint32_t cnt = (uint32_t)__popcll((unsigned long long)__ballot(valid));
        // the gains depend on the times alone: te = the meter's `last` after this lane's packet (the running maximum)
        uint64_t te = it.t;
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint64_t y = __shfl_up(te, d, 64);
            if (lane >= d) te = te > y ? te : y;
        }
        te = te > run.s.last ? te : run.s.last;
        uint64_t tp = __shfl_up(te, 1, 64);
        if (lane == 0) tp = run.s.last;
        uint64_t a, gx;
        meter_gains(g, tr, te - tp, a, gx);
        uint32_t col = PKT_METER_GREEN;
        bool done = false;
#if PKTGPU_METER_GREEN_STEP
        done = green_step(run, g, tr, valid, cnt, lane, it, a, gx);
#endif
        if (!done) {  // the plain walk: every lane takes the packets in order from the lanes that hold them
            for (uint32_t j = 0; j < cnt; j++) {  // uniform
                meter_refill(run.s, g, tr, lane64(a, j), lane64(gx, j));
                const uint32_t c = meter_decide(run.s, tr, lane32(it.ic, j), lane64(it.B, j));
                col = lane == j ? c : col;
            }
            // the counters take the step at once: each lane holds its packet's colour
#pragma unroll
            for (uint32_t c = 0; c < 3; c++) {
                const bool mine = valid && col == c;
                uint32_t len = mine ? it.len : 0u;
#pragma unroll
                for (uint32_t d = 32; d; d >>= 1) len += (uint32_t)__shfl_xor((int)len, (int)d, 64);
                run.pk[c] += (uint32_t)__popcll((unsigned long long)__ballot(mine));
                run.by[c] += len;
            }
        }
        run.s.last = lane64(te, 63u);
        if (valid) P.col[pos] = (uint8_t)col;
        if (cnt < 64u) break;  // uniform: the run ended
    }
    if (lane == 0) meter_run_store(P.v.st[k0], run);
}

__global__ __launch_bounds__(kMBlock) void meter_emit_kernel(MParams P) {
    __shared__ uint32_t s_hits[PKT_METER_COLORS];
    __shared__ unsigned long long s_bytes[PKT_METER_COLORS];
    const uint32_t t = threadIdx.x, lane = t & 63u;
    const bool counting = P.c.hits || P.c.bytes;  // uniform over the grid
    if (counting) {
        if (t < PKT_METER_COLORS) {
            s_hits[t] = 0;
            s_bytes[t] = 0;
        }
        __syncthreads();
    }
    const uint32_t ntiles = (P.cn + kMBlock - 1) / kMBlock;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {  // uniform
        const uint32_t pos = tile * kMBlock + t;
        const bool act = pos < P.cn;
        uint32_t col = PKT_METER_UNMETERED, len = 0;
        if (act) {
            const uint64_t i = P.c0 + pos;
            const uint64_t off = pkt_off(P.c.src, i);
            len = pkt_len(P.c.src, i, off);
            const uint32_t k = meter_of(P.c, P.v.nmeters, i);
            uint32_t w = 0;
            if (k != ~0u) {
                col = P.col[pos];
                w = P.v.word[k];
            }
            meter_emit(P.c, i, col, w, off, len);
        }
        if (counting) {
#pragma unroll
            for (uint32_t q = 0; q < PKT_METER_COLORS; q++) {
                const bool mine = act && col == q;
                const uint64_t mm = __ballot(mine);
                if (!mm) continue;  // uniform
                uint32_t sum = mine ? len : 0u;
#pragma unroll
                for (uint32_t x = 32; x; x >>= 1) sum += (uint32_t)__shfl_xor((int)sum, (int)x, 64);
                if (lane == 0) {
                    atomicAdd(&s_hits[q], (uint32_t)__popcll((unsigned long long)mm));
                    atomicAdd(&s_bytes[q], (unsigned long long)sum);
                }
            }
        }
    }
    if (!counting) return;
    __syncthreads();
    if (t < PKT_METER_COLORS) {
        const uint32_t h = s_hits[t];
        const uint64_t bsum = s_bytes[t];
        if (P.c.hits && h) __hip_atomic_fetch_add(P.c.hits + t, (uint64_t)h, METER_RLX);
        if (P.c.bytes && bsum) __hip_atomic_fetch_add(P.c.bytes + t, bsum, METER_RLX);
    }
}

__global__ __launch_bounds__(kMBlock) void meter_reset_kernel(MeterView v) {
    const uint32_t k = blockIdx.x * kMBlock + threadIdx.x;
    if (k < v.nmeters) meter_state_reset(v.st[k], v.cfg[k]);
}

pkt_ctx* ctx_of(pkt_meter* t) { return static_cast<pkt_ctx*>(t->ctx); }

int meter_hip_fail(pkt_meter* t, hipError_t e, const char* what) {
    t->err = std::string(what) + ": " + hipGetErrorString(e);
    return hip_fail(ctx_of(t), e, what);
}

int meter_dev_batch(pkt_meter* t, const MeterCall& c, void* stream) {
    hipError_t e = hipSetDevice(t->device);
    if (e != hipSuccess) return meter_hip_fail(t, e, "hipSetDevice");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    MParams P{};
    P.v = t->v;
    P.c = c;
    P.cnt = t->cnt;
    P.ctl = t->ctl;
    P.col = t->col;
    const uint32_t passes = t->bits <= 8 ? 1u : (t->bits + 7u) / 8u;
    const dim3 blk(kMBlock);
    for (uint64_t c0 = 0; c0 < c.n; c0 += kMeterChunk) {
        P.c0 = c0;
        P.cn = (uint32_t)(c.n - c0 < kMeterChunk ? c.n - c0 : kMeterChunk);
        P.ntiles = (P.cn + kMTile - 1) / kMTile;
        uint32_t cur = 0;  // the buffers the pass writes
        for (uint32_t pass = 0; pass < passes; pass++, cur ^= 1u) {
            P.pass = pass;
            P.shift = 8u * pass;
            P.nbits = t->bits > P.shift ? (t->bits - P.shift < 8u ? t->bits - P.shift : 8u) : 0u;
            P.key_in = t->key[cur ^ 1u], P.idx_in = t->idx[cur ^ 1u];
            P.key_out = t->key[cur], P.idx_out = t->idx[cur];
            hipLaunchKernelGGL(meter_count_kernel, dim3(P.ntiles), blk, 0, s, P);
            hipLaunchKernelGGL(meter_scan_kernel, dim3(1), dim3(kScanBlock), 0, s, P);
            hipLaunchKernelGGL(meter_place_kernel, dim3(P.ntiles), blk, 0, s, P);
        }
        P.key_in = t->key[cur ^ 1u], P.idx_in = t->idx[cur ^ 1u];  // what the last pass wrote
        const uint32_t tiles = (P.cn + kMBlock - 1) / kMBlock;
        hipLaunchKernelGGL(meter_walk_kernel, dim3(tiles), blk, 0, s, P);
        hipLaunchKernelGGL(meter_emit_kernel, dim3((c.hits || c.bytes) && tiles > kCountBlocks ? kCountBlocks : tiles), blk, 0, s, P);
    }
    if ((e = hipGetLastError()) != hipSuccess) return meter_hip_fail(t, e, "pkt_meter_batch launch");
    return PKT_SUCCESS;
}

int meter_dev_reset(pkt_meter* t, void* stream) {
    hipError_t e = hipSetDevice(t->device);
    if (e != hipSuccess) return meter_hip_fail(t, e, "hipSetDevice");
    hipLaunchKernelGGL(meter_reset_kernel, dim3((t->v.nmeters + kMBlock - 1) / kMBlock), dim3(kMBlock), 0,
                       reinterpret_cast<hipStream_t>(stream), t->v);
    if ((e = hipGetLastError()) != hipSuccess) return meter_hip_fail(t, e, "pkt_meter_reset");
    return PKT_SUCCESS;
}

int meter_dev_export(pkt_meter* t, uint32_t first, uint32_t count, pkt_meter_state_t* out) {
    hipError_t e = hipSetDevice(t->device);
    if (e == hipSuccess) e = hipDeviceSynchronize();  // blocking: the queued calls on every stream are over
    if (e == hipSuccess && count)
        e = hipMemcpy(out, t->v.st + first, (uint64_t)count * sizeof(pkt_meter_state_t), hipMemcpyDeviceToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    return e == hipSuccess ? PKT_SUCCESS : meter_hip_fail(t, e, "pkt_meter_export");
}

int meter_dev_destroy(pkt_meter* t) {
    (void)hipSetDevice(t->device);
    return hipFree(t->dev_buf) == hipSuccess ? PKT_SUCCESS : PKT_ERR_HIP;
}

void meter_dev_refused(pkt_meter* t) {
    if (t->ctx) ctx_of(t)->err = t->err;
}

const MeterDevOps kDevOps = {meter_dev_batch, meter_dev_reset, meter_dev_export, meter_dev_destroy, meter_dev_refused};

}  // namespace

extern "C" int pkt_meter_create(pkt_ctx_t* ctx, const pkt_meter_cfg_t* cfg, uint32_t nmeters, int32_t adjust, pkt_meter_t** out) {
    if (!ctx || !out) return fail(ctx, PKT_ERR_INVALID_ARG, "pkt_meter_create: null argument");
    *out = nullptr;
    if (const char* msg = meter_create_error(cfg, nmeters)) {
        ctx->err = std::string("pkt_meter_create: ") + msg;
        return PKT_ERR_INVALID_ARG;
    }
    pkt_meter* t = new pkt_meter;
    t->ops = &kDevOps;
    t->ctx = ctx;
    t->device = ctx->device;
    meter_pack(cfg, nmeters, t->h_cfg, t->h_word);
    for (t->bits = 0; t->bits < 32 && (1ull << t->bits) < nmeters; t->bits++) {}
    // one allocation: every piece starts 16-byte aligned, the 64-bit arrays first
    uint64_t at = 0;
    auto piece = [&](uint64_t bytes) {
        const uint64_t o = at;
        at += round16(bytes);
        return o;
    };
    const uint64_t o_cfg = piece((uint64_t)nmeters * sizeof(MeterCfg)), o_st = piece((uint64_t)nmeters * sizeof(pkt_meter_state_t));
    const uint64_t o_word = piece((uint64_t)nmeters * 4);
    const uint64_t o_k0 = piece(kMeterChunk * 4ull), o_k1 = piece(kMeterChunk * 4ull);
    const uint64_t o_i0 = piece(kMeterChunk * 4ull), o_i1 = piece(kMeterChunk * 4ull);
    const uint64_t o_cnt = piece((uint64_t)kDigits * kMeterTiles * 4), o_ctl = piece(kCtlWords * 4), o_col = piece(kMeterChunk);
    hipError_t e = hipSetDevice(ctx->device);
    uint8_t* base = nullptr;
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&base), at);
    if (e != hipSuccess) {
        delete t;
        return hip_fail(ctx, e, "pkt_meter_create");
    }
    t->dev_buf = base;
    auto p32 = [&](uint64_t o) { return reinterpret_cast<uint32_t*>(base + o); };
    MeterView& v = t->v;
    v.cfg = reinterpret_cast<const MeterCfg*>(base + o_cfg);
    v.st = reinterpret_cast<pkt_meter_state_t*>(base + o_st);
    v.word = p32(o_word);
    v.nmeters = nmeters;
    v.adjust = adjust;
    t->key[0] = p32(o_k0), t->key[1] = p32(o_k1), t->idx[0] = p32(o_i0), t->idx[1] = p32(o_i1);
    t->cnt = p32(o_cnt), t->ctl = p32(o_ctl), t->col = base + o_col;
    e = hipMemcpy(base + o_cfg, t->h_cfg.data(), (uint64_t)nmeters * sizeof(MeterCfg), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(base + o_word, t->h_word.data(), (uint64_t)nmeters * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(t->ctl, 0, kCtlWords * 4);
    int rc = e == hipSuccess ? meter_dev_reset(t, nullptr) : hip_fail(ctx, e, "pkt_meter_create");
    if (rc == PKT_SUCCESS && (e = hipDeviceSynchronize()) != hipSuccess) rc = hip_fail(ctx, e, "pkt_meter_create");
    if (rc != PKT_SUCCESS) {
        (void)hipFree(base);
        delete t;
        return rc;
    }
    t->h_cfg.clear(), t->h_cfg.shrink_to_fit();
    t->h_word.clear(), t->h_word.shrink_to_fit();
    *out = t;
    return PKT_SUCCESS;
}
