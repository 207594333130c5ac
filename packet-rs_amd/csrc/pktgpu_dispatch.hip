// pktgpu_dispatch.hip — pkt_dispatch_create / _destroy / _batch and pkt_reorder_batch: a stable bucket partition
// of a batch, and the gather that turns it into per-bucket batches.
//   Dispatch is three launches whose boundaries publish the data; no lane waits for another, nothing is added
//   to global memory, so the result is the same from run to run.  A TILE is kTile = 2048 consecutive packets, a
//   block of 4 waves; wave w owns the tile's packets [512 w, 512 w + 512) and takes them 64 at a time (8 rounds),
//   so that (tile, wave, round, lane) order is source order.  b' = the bucket, nbuckets for a dropped packet.
//   count_kernel   a wave's lanes with the same b' find each other by ballots over its bits (peers_of: the same
//                  cost whatever the bucket mix); the group's lowest lane adds the group's size to the wave's own
//                  LDS histogram.  After a barrier the four histograms are summed and stored, plain vector
//                  stores, to cnt[b' * ntiles + tile]: bucket-major, so that ...
//   scan_kernel    ... ONE exclusive scan over the flat array gives off[b' * ntiles + tile] = the packets of
//                  lower buckets + this bucket's packets of earlier tiles: the tile's first position in the
//                  bucket.  Block g scans elements [g * chunk, (g + 1) * chunk), kScanPass = 1024 a pass of its
//                  loop, after summing everything below its chunk itself (reads, not waits).  The element
//                  b' * ntiles is start[b'].
//   place_kernel   each tile computes its waves' histograms again, turns them into each wave's first position
//                  per bucket (off + the earlier waves' counts), and ranks its packets: a lane's position is its
//                  wave's running count for b' plus popcount(peers & lanes_below); the group's lowest lane then
//                  moves the count on.  Stores perm (scattered 4-byte stores, consecutive within a group), rank
//                  and bucket (coalesced).
//   reorder_bytes_kernel    a wave covers 64 positions and walks their 16-byte chunks together (flat_walk /
//                  locate, pktgpu_batch.hpp): two aligned 16-byte loads and take16 for a source at any alignment,
//                  one aligned 16-byte store, the tail chunk masked with bytes_below.
//   reorder_cols_kernel     a lane owns a position: perm[k] read once, the segment found in an LDS copy of
//                  seg_start, then every column of the table in the kernel arguments.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pktgpu_ctx.hpp"
#include "pktgpu_dispatch.hpp"

struct pkt_dispatch {
    pkt_ctx* ctx;
    int device;
    uint32_t nbuckets;
    uint32_t mask;        // table_len - 1
    uint16_t* table;      // device, or nullptr: DIRECT mode
    uint64_t max_n;
    uint32_t* cnt;        // device scratch [nbuckets + 1][tiles(max_n)]
    uint32_t* off;        // the same size: cnt's exclusive scan
};

namespace {

constexpr uint32_t kDBlock = 256, kDWaves = 4, kRounds = 8;
constexpr uint32_t kTile = kDBlock * kRounds;  // 2048 packets
constexpr uint32_t kNB1 = PKT_DISPATCH_MAX_BUCKETS + 1;
constexpr uint32_t kScanBlock = 256, kScanPass = 4 * kScanBlock;  // elements a block scans per pass of its loop
constexpr uint32_t kScanMaxBlocks = 256;

constexpr bool col_sizes_agree() {
    for (int c = 0; c < kNumCols; c++)
        if (kColSize[c] != kReorderColSize[c]) return false;
    return kNumCols == kReorderCols && kColHdrType == kReorderHdrType && kColHdrOff == kReorderHdrOff;
}
static_assert(col_sizes_agree(), "kColSize (pktgpu_ctx.hpp) and kReorderColSize (pktgpu_dispatch.hpp) differ");

struct DParams {
    const uint32_t* key;
    const uint8_t* select;
    const uint16_t* table;
    uint32_t mask, nbuckets, nbits;  // nbits: the bits of b' (0..nbuckets)
    uint32_t n, ntiles;
    uint32_t* cnt;
    uint32_t* off;
    uint16_t* bucket;
    uint32_t* perm;
    uint32_t* rank;
};

// The lanes of the wave that are active and hold the same b' as this one (itself included).
__device__ __forceinline__ uint64_t peers_of(uint32_t b, bool act, uint32_t nbits) {
    uint64_t m = __ballot(act);
    for (uint32_t k = 0; k < nbits; k++) {  // uniform
        const bool bit = (b >> k) & 1u;
        const uint64_t bal = __ballot(bit);
        m &= bit ? bal : ~bal;
    }
    return m;
}

// The tile's b' values of this lane, round r = packet tile * kTile + wave * 512 + r * 64 + lane (kNB1 past n).
__device__ __forceinline__ void load_buckets(const DParams& P, uint32_t tile, uint32_t wv, uint32_t lane,
                                             uint32_t bk[kRounds]) {
    uint32_t key[kRounds];
    uint8_t sel[kRounds];
    const uint64_t i0 = (uint64_t)tile * kTile + wv * (kTile / kDWaves) + lane;
#pragma unroll
    for (uint32_t r = 0; r < kRounds; r++) {
        const uint64_t i = i0 + 64u * r;
        key[r] = 0;
        sel[r] = 1;
        if (i < P.n) {
            key[r] = P.key[i];
            if (P.select) sel[r] = P.select[i];
        }
    }
#pragma unroll
    for (uint32_t r = 0; r < kRounds; r++) {
        const uint64_t i = i0 + 64u * r;
        bk[r] = i < P.n ? dispatch_bucket(key[r], sel[r] != 0, P.nbuckets, P.table, P.mask) : kNB1;
    }
}

// The wave's histogram of its 512 packets into its own LDS row h[0..nbuckets] (zeroed by the caller, behind a
// barrier).  Distinct groups hold distinct b', so the leaders' read-modify-writes never meet.
__device__ __forceinline__ void wave_hist(const uint32_t bk[kRounds], uint32_t nbits, uint32_t lane, uint32_t* h) {
#pragma unroll
    for (uint32_t r = 0; r < kRounds; r++) {
        const bool act = bk[r] != kNB1;
        const uint64_t peers = peers_of(bk[r], act, nbits);
        if (act && (uint32_t)__ffsll((unsigned long long)peers) - 1u == lane) h[bk[r]] += (uint32_t)__popcll(peers);
        wave_sync();
    }
}

__global__ __launch_bounds__(kDBlock) void count_kernel(DParams P) {
    __shared__ uint32_t s_h[kDWaves][kNB1];
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6, tile = blockIdx.x;
    const uint32_t nb1 = P.nbuckets + 1;
    for (uint32_t b = t; b < kDWaves * kNB1; b += kDBlock) (&s_h[0][0])[b] = 0;
    uint32_t bk[kRounds];
    load_buckets(P, tile, wv, lane, bk);
    __syncthreads();
    wave_hist(bk, P.nbits, lane, s_h[wv]);
    __syncthreads();
    for (uint32_t b = t; b < nb1; b += kDBlock)
        P.cnt[(uint64_t)b * P.ntiles + tile] = s_h[0][b] + s_h[1][b] + s_h[2][b] + s_h[3][b];
}

// off = the exclusive scan of cnt[0, total); start[b] = off[b * ntiles] (b <= nbuckets), start[nbuckets + 1] = n.
__global__ __launch_bounds__(kScanBlock) void scan_kernel(const uint32_t* __restrict__ cnt, uint32_t* __restrict__ off,
                                                          uint64_t total, uint64_t chunk, uint32_t ntiles,
                                                          uint32_t nbuckets, uint32_t n, uint64_t* start) {
    __shared__ uint32_t s_w[kScanBlock / 64];
    __shared__ uint32_t s_carry;
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
    const uint64_t e0 = (uint64_t)blockIdx.x * chunk;
    const uint64_t e1 = e0 + chunk < total ? e0 + chunk : total;
    // everything below the chunk, summed by this block itself (e0 is a multiple of 4; cnt is 16-byte aligned)
    uint32_t below = 0;
    for (uint64_t q = t; q < e0 / 4; q += kScanBlock) {
        const uint4 v = reinterpret_cast<const uint4*>(cnt)[q];
        below += v.x + v.y + v.z + v.w;
    }
#pragma unroll
    for (uint32_t x = 32; x; x >>= 1) below += (uint32_t)__shfl_xor((int)below, (int)x, 64);
    if (lane == 0) s_w[wv] = below;
    __syncthreads();
    if (t == 0) s_carry = s_w[0] + s_w[1] + s_w[2] + s_w[3];
    __syncthreads();
    if (blockIdx.x == 0 && t == 0 && start) start[nbuckets + 1] = n;
    for (uint64_t base = e0; base < e1; base += kScanPass) {  // uniform
        const uint64_t e = base + 4u * t;
        uint32_t v[4];
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) v[j] = e + j < e1 ? cnt[e + j] : 0u;
        const uint32_t mine = v[0] + v[1] + v[2] + v[3];
        const uint32_t incl = wave_incl_scan(mine, lane);
        __syncthreads();  // the previous pass's carry is stored, its wave sums are read
        const uint32_t carry = s_carry;
        if (lane == 63) s_w[wv] = incl;
        __syncthreads();  // the carry is read before the last thread stores the next one
        uint32_t x = carry + incl - mine;
        for (uint32_t w = 0; w < wv; w++) x += s_w[w];  // uniform per wave
        if (t == kScanBlock - 1) s_carry = x + mine;
        // element e = row * ntiles + col (total < 2^32: at most 257 rows of 2^21 tiles); col == 0 is start[row]
        uint32_t row = (uint32_t)e / ntiles, col = (uint32_t)e - row * ntiles;
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            if (e + j < e1) {
                off[e + j] = x;
                if (start && col == 0) start[row] = x;
            }
            x += v[j];
            if (++col == ntiles) {
                col = 0;
                row++;
            }
        }
    }
}

__global__ __launch_bounds__(kDBlock) void place_kernel(DParams P) {
    __shared__ uint32_t s_h[kDWaves][kNB1];
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6, tile = blockIdx.x;
    const uint32_t nb1 = P.nbuckets + 1;
    const bool ranks = P.perm || P.rank;  // uniform over the grid
    uint32_t bk[kRounds];
    load_buckets(P, tile, wv, lane, bk);
    const uint64_t i0 = (uint64_t)tile * kTile + wv * (kTile / kDWaves) + lane;
    if (P.bucket) {
#pragma unroll
        for (uint32_t r = 0; r < kRounds; r++)
            if (bk[r] != kNB1) P.bucket[i0 + 64u * r] = (uint16_t)(bk[r] < P.nbuckets ? bk[r] : PKT_DISPATCH_DROP);
    }
    if (!ranks) return;
    for (uint32_t b = t; b < kDWaves * kNB1; b += kDBlock) (&s_h[0][0])[b] = 0;
    __syncthreads();
    wave_hist(bk, P.nbits, lane, s_h[wv]);
    __syncthreads();
    // the waves' counts -> each wave's first position in each bucket
    for (uint32_t b = t; b < nb1; b += kDBlock) {
        uint32_t at = P.off[(uint64_t)b * P.ntiles + tile];
#pragma unroll
        for (uint32_t w = 0; w < kDWaves; w++) {
            const uint32_t c = s_h[w][b];
            s_h[w][b] = at;
            at += c;
        }
    }
    __syncthreads();
    uint32_t* h = s_h[wv];
#pragma unroll
    for (uint32_t r = 0; r < kRounds; r++) {
        const bool act = bk[r] != kNB1;
        const uint64_t peers = peers_of(bk[r], act, P.nbits);
        const uint32_t first = act ? h[bk[r]] : 0u;
        const uint32_t pos = first + (uint32_t)__popcll(peers & ((1ull << lane) - 1ull));
        wave_sync();  // the group has read its count before its lowest lane moves it on
        if (act && (uint32_t)__ffsll((unsigned long long)peers) - 1u == lane) h[bk[r]] = first + (uint32_t)__popcll(peers);
        wave_sync();
        if (act) {  // pos < n: the counts of all tiles sum to n
            const uint64_t i = i0 + 64u * r;
            if (P.perm) P.perm[pos] = (uint32_t)i;
            if (P.rank) P.rank[i] = pos;
        }
    }
}

// ---- reorder
struct RSeg {
    const uint64_t* seg_start;  // [nseg + 1], or unused with nseg == 0
    uint32_t nseg, m;
};

// The first position that is not written: min(seg_start[nseg], m), or m without segments.
__device__ __forceinline__ uint32_t reorder_limit(const RSeg& S) {
    if (!S.nseg) return S.m;
    const uint64_t e = S.seg_start[S.nseg];
    return e < S.m ? (uint32_t)e : S.m;
}

struct RBParams {
    BatchSrc src;
    uint64_t n;
    const uint32_t* perm;
    RSeg seg;
    uint8_t* dst;
    uint32_t slot;
    uint32_t* out_len;
};

__global__ __launch_bounds__(kDBlock) void reorder_bytes_kernel(RBParams P) {
    __shared__ uint32_t s_pre[kDWaves][65];
    __shared__ uint64_t s_off[kDWaves][64];
    __shared__ uint32_t s_len[kDWaves][64];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t k0 = (uint64_t)blockIdx.x * kDBlock + 64u * wv;  // the wave's first position
    const uint64_t k = k0 + lane;
    const uint32_t limit = reorder_limit(P.seg);
    // (seg_start is non-decreasing from 0, the caller's promise: every position below the limit is in a segment)
    uint64_t off = 0;
    uint32_t len = 0;
    if (k < limit) {
        const uint64_t p = P.perm[k];
        if (p < P.n) {
            off = pkt_off(P.src, p);
            len = pkt_len(P.src, p, off);
            len = len < P.slot ? len : P.slot;
        }
        if (P.out_len) P.out_len[k] = len;
    }
    const uint32_t chunks = (len + 15u) >> 4;
    const uint32_t incl = wave_incl_scan(chunks, lane);
    if (lane == 0) s_pre[wv][0] = 0;
    s_pre[wv][lane + 1] = incl;
    s_off[wv][lane] = off;
    s_len[wv][lane] = len;
    wave_sync();
    const uint32_t total = __builtin_amdgcn_readfirstlane(s_pre[wv][64]);  // <= 64 * 4096
    const FlatWalk walk = flat_walk(chunks);
    // an aligned chunk at or past the slab's last one is not loaded again: its bytes are not needed
    const uint64_t last = P.src.slab_len ? ((P.src.slab_len + 15) & ~(uint64_t)15) - 16 : 0;
    for (uint32_t f = lane; f < total; f += 64u) {
        const FlatAt at = locate(walk, s_pre[wv], f);
        // bytes [16 c, min(16 c + 16, len)) of the packet lie inside the slab, so the first aligned chunk is at or
        // below the slab's last one; the second is loaded only when it is too
        const uint64_t A = s_off[wv][at.p] + 16u * at.k, A0 = A & ~(uint64_t)15;
        const uint4 v0 = *reinterpret_cast<const uint4*>(P.src.slab + A0);
        const uint4 v1 = *reinterpret_cast<const uint4*>(P.src.slab + A0 + (A0 >= last ? 0u : 16u));
        uint32_t o[4];
        take16(v0, v1, (uint32_t)A & 15u, o);
        const uint32_t left = s_len[wv][at.p] - 16u * at.k;  // >= 1
        if (left < 16u) {
            const Le128 keep = bytes_below(left);
            o[0] &= (uint32_t)keep.lo;
            o[1] &= (uint32_t)(keep.lo >> 32);
            o[2] &= (uint32_t)keep.hi;
            o[3] &= (uint32_t)(keep.hi >> 32);
        }
        // inside the slot: 16 k + 16 <= round_up(len, 16) <= slot, and (k0 + p + 1) * slot <= m * slot <= dst_len
        *reinterpret_cast<uint4*>(P.dst + (k0 + at.p) * P.slot + 16u * at.k) = make_uint4(o[0], o[1], o[2], o[3]);
    }
}

struct RCol {
    const uint8_t* src;
    uint8_t* dst;
    uint32_t sz, slots;  // element bytes; 1 = a slot column
};
struct RCParams {
    RCol col[kNumCols];
    uint32_t ncol;
    uint64_t n;
    const uint32_t* perm;
    const uint8_t* n_hdrs;  // the source's, or nullptr
    RSeg seg;
    bool any_slots;
};

// element e of a column of sz-byte elements: dst[e] = empty ? 0 : src[s]
__device__ __forceinline__ void move_elem(const RCol& c, uint64_t s, uint64_t e, bool empty) {
    switch (c.sz) {  // uniform
        case 1: c.dst[e] = empty ? (uint8_t)0 : c.src[s]; break;
        case 2: reinterpret_cast<uint16_t*>(c.dst)[e] = empty ? (uint16_t)0 : reinterpret_cast<const uint16_t*>(c.src)[s]; break;
        case 4: reinterpret_cast<uint32_t*>(c.dst)[e] = empty ? 0u : reinterpret_cast<const uint32_t*>(c.src)[s]; break;
        case 8: reinterpret_cast<uint64_t*>(c.dst)[e] = empty ? 0ull : reinterpret_cast<const uint64_t*>(c.src)[s]; break;
        default: {  // 16: the ipv6 addresses, dwords (a caller's column need not be 16-byte aligned)
            const uint32_t* sp = reinterpret_cast<const uint32_t*>(c.src) + 4 * s;
            uint32_t* dp = reinterpret_cast<uint32_t*>(c.dst) + 4 * e;
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) dp[j] = empty ? 0u : sp[j];
        }
    }
}

__global__ __launch_bounds__(kDBlock) void reorder_cols_kernel(RCParams P) {
    __shared__ uint32_t s_seg[PKT_REORDER_MAX_SEGS + 1];
    const uint32_t t = threadIdx.x;
    for (uint32_t s = t; s <= P.seg.nseg && P.seg.nseg; s += kDBlock) {
        const uint64_t v = P.seg.seg_start[s];
        s_seg[s] = v < P.seg.m ? (uint32_t)v : P.seg.m;
    }
    __syncthreads();
    const uint64_t k = (uint64_t)blockIdx.x * kDBlock + t;
    if (k >= P.seg.m) return;
    const ReorderSeg sg = reorder_seg(s_seg, P.seg.nseg, (uint32_t)k, P.seg.m);
    if (!sg.live) return;
    const uint64_t p = P.perm[k];
    const bool empty = p >= P.n;
    uint32_t rows = PKT_MAX_HDRS;
    if (P.any_slots && P.n_hdrs && !empty) {
        rows = P.n_hdrs[p];
        rows = rows < PKT_MAX_HDRS ? rows : PKT_MAX_HDRS;
    }
    const uint64_t e0 = (uint64_t)PKT_MAX_HDRS * sg.s0 + (k - sg.s0);  // the position's row 0: < 16 m
    for (uint32_t c = 0; c < P.ncol; c++) {  // uniform
        const RCol& col = P.col[c];
        if (col.slots) {
            for (uint32_t j = 0; j < rows; j++) move_elem(col, (uint64_t)j * P.n + p, e0 + (uint64_t)j * sg.ns, empty);
        } else {
            move_elem(col, p, k, empty);
        }
    }
}

uint32_t tiles_of(uint64_t n) { return (uint32_t)((n + kTile - 1) / kTile); }

}  // namespace

extern "C" int pkt_dispatch_create(pkt_ctx_t* ctx, uint32_t nbuckets, const uint16_t* table, uint32_t table_len,
                                   uint64_t max_n, pkt_dispatch_t** out) {
    if (!ctx || !out) return fail(ctx, PKT_ERR_INVALID_ARG, "pkt_dispatch_create: null argument");
    *out = nullptr;
    if (const char* msg = dispatch_create_error(nbuckets, table, table_len, max_n, true))
        return fail(ctx, PKT_ERR_INVALID_ARG, msg);
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    pkt_dispatch* d = new pkt_dispatch{ctx, ctx->device, nbuckets, table ? table_len - 1 : 0u, nullptr, max_n, nullptr, nullptr};
    // (the scratch rounded up to whole 16-byte chunks: the scan sums cnt by uint4)
    const uint64_t elems = ((uint64_t)(nbuckets + 1) * tiles_of(max_n) + 3) & ~3ull;
    e = hipMalloc(reinterpret_cast<void**>(&d->cnt), elems * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d->off), elems * sizeof(uint32_t));
    if (e == hipSuccess && table) {
        e = hipMalloc(reinterpret_cast<void**>(&d->table), table_len * sizeof(uint16_t));
        if (e == hipSuccess) e = hipMemcpy(d->table, table, table_len * sizeof(uint16_t), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
        if (d->cnt) (void)hipFree(d->cnt);
        if (d->off) (void)hipFree(d->off);
        if (d->table) (void)hipFree(d->table);
        delete d;
        return hip_fail(ctx, e, "pkt_dispatch_create");
    }
    *out = d;
    return PKT_SUCCESS;
}

extern "C" int pkt_dispatch_destroy(pkt_dispatch_t* d) {
    if (!d) return PKT_ERR_INVALID_ARG;
    (void)hipSetDevice(d->device);
    hipError_t e = hipFree(d->cnt);
    const hipError_t e2 = hipFree(d->off);
    const hipError_t e3 = d->table ? hipFree(d->table) : hipSuccess;
    e = e != hipSuccess ? e : e2 != hipSuccess ? e2 : e3;
    delete d;
    return e == hipSuccess ? PKT_SUCCESS : PKT_ERR_HIP;
}

extern "C" int pkt_dispatch_batch(pkt_dispatch_t* d, const uint32_t* key, const uint8_t* select, uint64_t n,
                                  uint16_t* bucket, uint32_t* perm, uint32_t* rank, uint64_t* start, void* stream) {
    if (!d) return PKT_ERR_INVALID_ARG;
    pkt_ctx* ctx = d->ctx;
    if (const char* msg = dispatch_call_error(key, n, d->max_n, start)) return fail(ctx, PKT_ERR_INVALID_ARG, msg);
    if (!bucket && !perm && !rank && !start) return PKT_SUCCESS;
    hipError_t e = hipSetDevice(d->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (n == 0) {
        if (start && (e = hipMemsetAsync(start, 0, (d->nbuckets + 2) * sizeof(uint64_t), s)) != hipSuccess)
            return hip_fail(ctx, e, "pkt_dispatch_batch: zeroing start");
        return PKT_SUCCESS;
    }
    DParams P{};
    P.key = key;
    P.select = select;
    P.table = d->table;
    P.mask = d->mask;
    P.nbuckets = d->nbuckets;
    P.nbits = 32u - (uint32_t)__builtin_clz(d->nbuckets);  // b' <= nbuckets
    P.n = (uint32_t)n;
    P.ntiles = tiles_of(n);
    P.cnt = d->cnt;
    P.off = d->off;
    P.bucket = bucket;
    P.perm = perm;
    P.rank = rank;
    if (perm || rank || start) {
        hipLaunchKernelGGL(count_kernel, dim3(P.ntiles), dim3(kDBlock), 0, s, P);
        if ((e = hipGetLastError()) != hipSuccess) return hip_fail(ctx, e, "dispatch count_kernel launch");
        const uint64_t total = (uint64_t)(d->nbuckets + 1) * P.ntiles;
        uint64_t blocks = (total + kScanPass - 1) / kScanPass;
        blocks = blocks < kScanMaxBlocks ? blocks : kScanMaxBlocks;
        uint64_t chunk = (total + blocks - 1) / blocks;
        chunk = (chunk + kScanPass - 1) / kScanPass * kScanPass;
        blocks = (total + chunk - 1) / chunk;
        hipLaunchKernelGGL(scan_kernel, dim3((unsigned)blocks), dim3(kScanBlock), 0, s, d->cnt, d->off, total, chunk,
                           P.ntiles, d->nbuckets, P.n, start);
        if ((e = hipGetLastError()) != hipSuccess) return hip_fail(ctx, e, "dispatch scan_kernel launch");
    }
    if (perm || rank || bucket) {
        hipLaunchKernelGGL(place_kernel, dim3(P.ntiles), dim3(kDBlock), 0, s, P);
        if ((e = hipGetLastError()) != hipSuccess) return hip_fail(ctx, e, "dispatch place_kernel launch");
    }
    return PKT_SUCCESS;
}

extern "C" int pkt_reorder_batch(pkt_ctx_t* ctx, const pkt_batch_t* b, const pkt_out_t* cols, const uint32_t* perm,
                                 uint64_t m, const uint64_t* seg_start, uint32_t nseg, uint8_t* dst, uint64_t dst_len,
                                 uint32_t slot, uint32_t* out_len, const pkt_out_t* out_cols, void* stream) {
    if (!ctx) return PKT_ERR_INVALID_ARG;
    if (const char* msg = reorder_error(b, cols, perm, m, seg_start, nseg, dst, dst_len, slot, out_len, out_cols, true))
        return fail(ctx, PKT_ERR_INVALID_ARG, msg);
    if (m == 0) return PKT_SUCCESS;
    RCParams C{};
    for (int c = 0; c < kNumCols; c++) {
        const void* in = reorder_col(cols, c);
        void* out = reorder_col(out_cols, c);
        if (!in || !out) continue;
        const bool slots = c == kColHdrType || c == kColHdrOff;
        C.col[C.ncol++] = RCol{static_cast<const uint8_t*>(in), static_cast<uint8_t*>(out), kColSize[c], slots ? 1u : 0u};
        C.any_slots = C.any_slots || slots;
    }
    if (!dst && !C.ncol) return PKT_SUCCESS;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const RSeg seg{seg_start, nseg, (uint32_t)m};
    const dim3 grid((unsigned)((m + kDBlock - 1) / kDBlock));
    if (dst) {
        RBParams B{};
        B.src = batch_src(b);
        B.n = b->n;
        B.perm = perm;
        B.seg = seg;
        B.dst = dst;
        B.slot = slot;
        B.out_len = out_len;
        hipLaunchKernelGGL(reorder_bytes_kernel, grid, dim3(kDBlock), 0, s, B);
        if ((e = hipGetLastError()) != hipSuccess) return hip_fail(ctx, e, "reorder_bytes_kernel launch");
    }
    if (C.ncol) {
        C.n = b->n;
        C.perm = perm;
        C.n_hdrs = static_cast<const uint8_t*>(reorder_col(cols, kReorderNHdrs));
        C.seg = seg;
        hipLaunchKernelGGL(reorder_cols_kernel, grid, dim3(kDBlock), 0, s, C);
        if ((e = hipGetLastError()) != hipSuccess) return hip_fail(ctx, e, "reorder_cols_kernel launch");
    }
    return PKT_SUCCESS;
}
