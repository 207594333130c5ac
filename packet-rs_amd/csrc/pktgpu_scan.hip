// pktgpu_scan.hip — pkt_scan_create and the device half of pkt_scan_batch.
//   scan_kernel<LDS>   a block first copies the compiled set's first level (the two 256-entry root tables and the
//                    two-byte bitmap, 10 KiB) into LDS and, LDS, its deep part too (the open-addressed edge table,
//                    the states' pattern lists and the groups); its hit counters are zeroed in LDS.  Then each WAVE
//                    takes tiles of 64 consecutive packets, strided over the grid (no block barrier inside).  Lane p
//                    reads packet p's offset, length and, PAYLOAD, its chain (the first four rows up front,
//                    chain_load), decides the status and the region [r0, r1) (scan_region_*, pktgpu_scan.hpp) and
//                    counts the aligned 16-byte slab chunks that hold a byte of it.  A wave prefix sum of the counts
//                    goes to LDS and the wave walks the FLATTENED chunk list 64 chunks a step, as l4_kernel does: a
//                    lane finds its (packet, chunk) in the prefix and loads ONE aligned chunk into the wave's stage;
//                    lanes 0..3 also load the four chunks that follow the step's last.  A packet's chunks are
//                    neighbours in the list, so behind every start position of the step lie 63 further staged bytes
//                    of the same packet (or bytes past r1, which the walk never takes).  A lane then tries its
//                    chunk's up to 16 start positions with THE walk (scan_start): most end at the root entries or
//                    the bitmap, all in LDS.  An occurrence goes to the packet's LDS slots — add (count), min
//                    (pattern << 16 | s), or (groups) — and to the block's LDS hit counter: order-independent, so
//                    the outputs are identical from run to run.  Lane p then writes packet p's outputs (coalesced).
//                    At the end the block adds each non-zero hit counter once (match_kernel's scheme); these are the
//                    only global atomics, and no lane waits for another.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pktgpu_ctx.hpp"
#include "pktgpu_scan.hpp"

namespace {

constexpr uint32_t kScanBlock = 256;
constexpr uint32_t kScanWaves = kScanBlock / 64;
constexpr uint32_t kScanAhead = 4;        // chunks staged past a step's 64: byte 15 of the last + 63 = chunk 68's byte 14
constexpr uint32_t kScanMaxBlocks = 2048; // 8 blocks a CU: the tables are copied once per block, not per tile
constexpr uint32_t kScanTilesPerBlock = 512;  // at most: a block's 32-bit LDS hit counters cannot wrap (below)
static_assert(16u * kScanAhead >= 15u + PKT_SCAN_MAX_LEN - 16u + 1u, "the stage holds 63 bytes behind every start");

struct SParams {
    BatchSrc src;
    uint64_t n;  // < 2^32
    const uint8_t* n_hdrs;
    const uint8_t* hdr_type;  // [PKT_MAX_HDRS][n]
    const uint16_t* hdr_off;  // [PKT_MAX_HDRS][n]
    const uint8_t* select;
    uint8_t* status;
    uint32_t* pat;
    uint16_t* off;
    uint32_t* action;
    uint8_t* sel;
    uint32_t* count;
    uint64_t* matched;
    uint64_t* hits;
    ScanView t;
    uint32_t region;
};

// an occurrence of pattern p at start s of the wave's packet pk
struct DevEmit {
    uint32_t* cnt;
    uint64_t* best;
    uint64_t* grp;
    const uint32_t* group;
    uint32_t* hits;  // NULL: not counted
    uint32_t pk, s;
    __device__ __forceinline__ void operator()(uint32_t p) const {
        atomicAdd(&cnt[pk], 1u);
        atomicMin(reinterpret_cast<unsigned long long*>(&best[pk]), (unsigned long long)p << 16 | s);
        atomicOr(reinterpret_cast<unsigned long long*>(&grp[pk]), 1ull << group[p]);
        if (hits) atomicAdd(&hits[p], 1u);
    }
};

template <bool LDS>
__global__ __launch_bounds__(kScanBlock) void scan_kernel(SParams P) {
    __shared__ uint4 s_stage[kScanWaves][64 + kScanAhead];
    __shared__ uint32_t s_pre[kScanWaves][65];   // exclusive prefix of the packets' chunk counts
    __shared__ uint64_t s_at[kScanWaves][64];    // the region's first byte in the slab
    __shared__ uint32_t s_span[kScanWaves][64];  // r1 - r0 | r0 << 16
    __shared__ uint32_t s_cnt[kScanWaves][64];
    __shared__ uint64_t s_best[kScanWaves][64];
    __shared__ uint64_t s_grp[kScanWaves][64];
    __shared__ uint32_t s_first[kScanFirstWords];
    extern __shared__ uint32_t s_dyn[];  // LDS: the deep part; then, hits: npats + 1 counters
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint32_t* const s_hits = P.hits ? s_dyn + (LDS ? P.t.deep_words : 0u) : nullptr;
    for (uint32_t k = threadIdx.x; k < kScanFirstWords; k += kScanBlock) s_first[k] = P.t.first[k];
    if (LDS)
        for (uint32_t k = threadIdx.x; k < P.t.deep_words; k += kScanBlock) s_dyn[k] = P.t.deep[k];
    if (s_hits)
        for (uint32_t k = threadIdx.x; k <= P.t.npats; k += kScanBlock) s_hits[k] = 0;
    __syncthreads();
    const uint32_t* const deep = LDS ? s_dyn : P.t.deep;
    const ScanTabs tabs = scan_tabs(s_first, deep, P.t);
    const uint32_t* const group = deep + P.t.group_w;
    const uint8_t* const stage = reinterpret_cast<const uint8_t*>(s_stage[wv]);

    const uint64_t tiles = (P.n + 63) >> 6;
    for (uint64_t tile = (uint64_t)blockIdx.x * kScanWaves + wv; tile < tiles; tile += (uint64_t)gridDim.x * kScanWaves) {
        const uint64_t i = tile * 64 + lane;
        uint32_t st = PKT_SCAN_SKIPPED, r0 = 0, r1 = 0;
        uint64_t off = 0;
        if (i < P.n && (!P.select || P.select[i])) {
            off = pkt_off(P.src, i);
            r1 = pkt_len(P.src, i, off);
            st = PKT_SCAN_MISS;
            if (P.region == PKT_SCAN_PAYLOAD) {  // uniform
                const ChainPre c = chain_load(P, i);
                const uint32_t nh = c.nh > PKT_MAX_HDRS ? PKT_MAX_HDRS : c.nh;
                ScanRegion r;
#pragma unroll
                for (uint32_t j = 0; j < 4; j++)
                    if (j < nh) scan_region_step(r, c.ty[j], c.of[j]);
                for (uint32_t j = 4; j < nh; j++)
                    scan_region_step(r, P.hdr_type[(uint64_t)j * P.n + i], P.hdr_off[(uint64_t)j * P.n + i]);
                st = scan_region_status(r, c.nh, r1);
                r0 = r.r0;
            }
        }
        const uint32_t span = st == PKT_SCAN_MISS ? r1 - r0 : 0u;
        const uint64_t S0 = off + r0;
        const uint32_t chunks = span ? (uint32_t)(((S0 + span + 15) >> 4) - (S0 >> 4)) : 0u;
        const uint32_t incl = wave_incl_scan(chunks, lane);
        if (lane == 0) s_pre[wv][0] = 0;
        s_pre[wv][lane + 1] = incl;
        s_at[wv][lane] = S0;
        s_span[wv][lane] = span | r0 << 16;  // both <= 65535
        s_cnt[wv][lane] = 0;
        s_best[wv][lane] = kScanNoBest;
        s_grp[wv][lane] = 0;
        wave_sync();
        const uint32_t total = __builtin_amdgcn_readfirstlane(s_pre[wv][64]);  // <= 64 * 4097
        const FlatWalk walk = flat_walk(chunks);
        for (uint32_t base = 0; base < total; base += 64u) {  // uniform
            // Flat chunk f is chunk k of packet p's region: it holds at least one byte of [S, S + span), which lies
            // inside the slab, so it is at or below the slab's last aligned chunk.
            const uint32_t f = base + lane;
            uint32_t pk = 64, lo = 0, hi = 0, s_lo = 0, avail_lo = 0;
            if (f < total) {
                const FlatAt at = locate(walk, s_pre[wv], f);
                pk = at.p;
                const uint64_t S = s_at[wv][pk], A = (S & ~(uint64_t)15) + 16ull * at.k;
                const uint32_t sp = s_span[wv][pk];
                const int64_t b = (int64_t)(S - A), e = b + (sp & 0xFFFFu);  // the region, relative to the chunk
                lo = b < 0 ? 0u : (uint32_t)b;                                // b <= 15
                hi = e > 16 ? 16u : (uint32_t)e;                              // e >= 1
                s_lo = (sp >> 16) + (uint32_t)((int64_t)lo - b);              // start lo, from the packet's first byte
                avail_lo = (uint32_t)(e - (int64_t)lo);                       // bytes from start lo to r1
                s_stage[wv][lane] = *reinterpret_cast<const uint4*>(P.src.slab + A);
            }
            if (lane < kScanAhead && base + 64u + lane < total) {
                const FlatAt at = locate(walk, s_pre[wv], base + 64u + lane);
                const uint64_t S = s_at[wv][at.p], A = (S & ~(uint64_t)15) + 16ull * at.k;
                s_stage[wv][64u + lane] = *reinterpret_cast<const uint4*>(P.src.slab + A);
            }
            wave_sync();
            if (pk < 64) {
                DevEmit emit{s_cnt[wv], s_best[wv], s_grp[wv], group, s_hits, pk, 0u};
                for (uint32_t j = lo; j < hi; j++) {
                    emit.s = s_lo + (j - lo);
                    scan_start(tabs, stage + 16u * lane + j, avail_lo - (j - lo), emit);
                }
            }
            wave_sync();  // the next step overwrites the stage
        }
        const uint32_t cnt = s_cnt[wv][lane];
        if (s_hits) {
            const uint32_t miss = (uint32_t)__popcll(__ballot(st == PKT_SCAN_MISS && cnt == 0));
            if (lane == 0 && miss) atomicAdd(&s_hits[P.t.npats], miss);
        }
        if (i < P.n) scan_store(P, i, scan_result(st, cnt, s_best[wv][lane], s_grp[wv][lane], P.t));
        wave_sync();  // the next tile rewrites the slots
    }
    if (!s_hits) return;  // uniform
    // A counter gains at most 65535 per packet and a block takes at most 4 * (kScanTilesPerBlock / 4 + 1) * 64
    // packets (the launch's grid), so it stays below 2^32.
    __syncthreads();
    for (uint32_t k = threadIdx.x; k <= P.t.npats; k += kScanBlock) {
        const uint32_t h = s_hits[k];
        if (h) __hip_atomic_fetch_add(P.hits + k, (uint64_t)h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

int scan_hip_fail(pkt_scan* s, hipError_t e, const char* what) {
    s->err = std::string(what) + ": " + hipGetErrorString(e);
    return PKT_ERR_HIP;
}

int dev_run(pkt_scan* s, const ScanCall& c, void* stream) {
    hipError_t e = hipSetDevice(s->device);
    if (e != hipSuccess) return scan_hip_fail(s, e, "hipSetDevice");
    SParams P{};
    P.src = c.src;
    P.n = c.n;
    P.n_hdrs = c.n_hdrs;
    P.hdr_type = c.hdr_type;
    P.hdr_off = c.hdr_off;
    P.select = c.select;
    P.status = c.status;
    P.pat = c.pat;
    P.off = c.off;
    P.action = c.action;
    P.sel = c.sel;
    P.count = c.count;
    P.matched = c.matched;
    P.hits = c.hits;
    P.t = s->view;
    P.region = c.region;
    const bool lds = s->info.placement == PKT_SCAN_PLACE_LDS;
    const uint64_t tiles = (c.n + 63) >> 6, by_wave = (tiles + kScanWaves - 1) / kScanWaves;
    const uint64_t least = (tiles + kScanTilesPerBlock - 1) / kScanTilesPerBlock;  // <= 2^17
    uint64_t blocks = by_wave < kScanMaxBlocks ? by_wave : kScanMaxBlocks;
    blocks = blocks < least ? least : blocks;
    const size_t dyn = 4ull * ((lds ? s->view.deep_words : 0u) + (c.hits ? s->view.npats + 1u : 0u));  // <= 32772
    const dim3 grid((unsigned)blocks);
    hipStream_t q = reinterpret_cast<hipStream_t>(stream);
    if (lds)
        hipLaunchKernelGGL(scan_kernel<true>, grid, dim3(kScanBlock), dyn, q, P);
    else
        hipLaunchKernelGGL(scan_kernel<false>, grid, dim3(kScanBlock), dyn, q, P);
    if ((e = hipGetLastError()) != hipSuccess) return scan_hip_fail(s, e, "scan launch");
    return PKT_SUCCESS;
}

int dev_destroy(pkt_scan* s) {
    (void)hipSetDevice(s->device);
    (void)hipDeviceSynchronize();
    if (s->dev_words) (void)hipFree(s->dev_words);
    return PKT_SUCCESS;
}

constexpr ScanDevOps kDevOps = {dev_run, dev_destroy};

}  // namespace

extern "C" int pkt_scan_create(pkt_ctx_t* ctx, const uint8_t* bytes, uint64_t nbytes, const pkt_scan_pattern_t* pats,
                               uint32_t npats, uint32_t default_action, pkt_scan_t** out) {
    if (!ctx || !out) return fail(ctx, PKT_ERR_INVALID_ARG, "pkt_scan_create: null argument");
    *out = nullptr;
    ScanImage img;
    int rc = scan_compile(bytes, nbytes, pats, npats, img, ctx->err);
    if (rc != PKT_SUCCESS) return rc;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    pkt_scan* s = new pkt_scan;
    s->ops = &kDevOps;
    s->device = ctx->device;
    s->info = img.info;
    s->info.placement = img.fits_lds ? PKT_SCAN_PLACE_LDS : PKT_SCAN_PLACE_GLOBAL;
    e = hipMalloc(reinterpret_cast<void**>(&s->dev_words), img.info.table_bytes);
    if (e == hipSuccess) e = hipMemcpy(s->dev_words, img.words.data(), img.info.table_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        rc = hip_fail(ctx, e, "pkt_scan_create");
        dev_destroy(s);
        delete s;
        return rc;
    }
    s->view = img.view(s->dev_words, default_action);
    *out = s;
    return PKT_SUCCESS;
}
