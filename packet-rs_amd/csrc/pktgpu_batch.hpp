// pktgpu_batch.hpp — the small pieces every source that walks a pkt_batch_t shares.
//   host and device: BatchSrc (a batch's five source fields, as kernels take them) with THE offset rule
//                    (pkt_off) and THE length clamp (pkt_len), the pkt_batch_t refusal rules, and the list of
//                    the 22 header sizes;
//   device only:     wave_sync, wave_incl_scan, block_excl_scan, take16, the little-endian Le128, the flattened
//                    chunk walk's locator (flat_walk, locate) and the chain's first four rows loaded up front
//                    (chain_load).
// Every object depends on this header (HDRS in the Makefile), the parse kernels' included: keep it to what is
// settled.
// It needs include/pktgpu.h alone (not the parser's walk, pktgpu_device.hpp), and the host part compiles without
// a HIP compiler (pktgpu_host.cpp under g++).
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#endif

#include <cstdint>

#include "../../include/pktgpu.h"

#ifdef __HIPCC__
#define PKT_HD __host__ __device__ __forceinline__
#else
#define PKT_HD inline
#endif

// Where a batch's packets are: pkt_batch_t without n.  Kernel parameter structs hold one.
struct BatchSrc {
    const uint8_t* slab;
    uint64_t slab_len;
    const uint64_t* offsets;
    const uint32_t* lens;
    uint32_t stride;
};

PKT_HD BatchSrc batch_src(const pkt_batch_t* b) { return BatchSrc{b->slab, b->slab_len, b->offsets, b->lens, b->stride}; }

// packet i's first byte in the slab
PKT_HD uint64_t pkt_off(const BatchSrc& s, uint64_t i) { return s.offsets ? s.offsets[i] : i * s.stride; }

// packet i's length: clamped to the slab end (0 for an offset at or past it) and to 65535
PKT_HD uint32_t pkt_len(const BatchSrc& s, uint64_t i, uint64_t off) {
    uint32_t l = s.lens ? s.lens[i] : s.stride;
    const uint64_t room = off < s.slab_len ? s.slab_len - off : 0;
    l = l > room ? (uint32_t)room : l;
    return l > 65535u ? 65535u : l;
}

// What is wrong with a batch of n > 0 packets, as the refusal's text, or nullptr.  The index rules hold for every
// entry point; the slab rules for those whose kernels load aligned 16-byte chunks of it (pktgpu_ctx.hpp has both
// with the ctx's error text: check_batch_index, check_batch_slab16).
inline bool batch_null_slab(const pkt_batch_t* b) { return b->slab_len && !b->slab; }

inline const char* batch_index_error(const pkt_batch_t* b) {
    if (b->offsets && !b->lens) return "offsets without lens";
    if (!b->offsets && b->stride == 0) return "stride 0";
    return nullptr;
}

inline const char* batch_slab16_error(const pkt_batch_t* b) {
    if (batch_null_slab(b)) return "null slab";
    if ((uintptr_t)b->slab & 15) return "slab not 16-byte aligned";
    return nullptr;
}

// pkt_hdr_size by header type (make_header! of the reference, src/headers.rs:529-827): the one list the device
// tables are defined from; pktgpu_host.cpp's kHdrs[].size is checked against it at compile time.
#define PKT_HDR_SIZE_LIST {0, 14, 4, 20, 40, 4, 20, 8, 28, 8, 14, 3, 5, 4, 4, 4, 4, 8, 12, 8, 35, 4}
constexpr uint8_t kHdrSizes[PKT_HDR_COUNT] = PKT_HDR_SIZE_LIST;

#ifdef __HIPCC__

// Order a wave's LDS writes before its other lanes' reads (no block barrier).
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// inclusive prefix sum of x over the wave's 64 lanes (uint32_t or uint64_t)
template <typename T>
__device__ __forceinline__ T wave_incl_scan(T x, uint32_t lane) {
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const T y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    return x;
}

// Exclusive prefix of v over the threads of a block of WAVES waves; total = the block's sum.  (s_w: one word per wave.)
template <uint32_t WAVES>
__device__ __forceinline__ uint64_t block_excl_scan(uint64_t v, uint64_t* s_w, uint64_t& total) {
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint64_t x = wave_incl_scan(v, lane);
    if (lane == 63) s_w[wv] = x;
    __syncthreads();
    uint64_t base = 0;
    total = 0;
#pragma unroll
    for (uint32_t k = 0; k < WAVES; k++) {
        const uint64_t t = s_w[k];
        base += k < wv ? t : 0;
        total += t;
    }
    __syncthreads();  // s_w may be written again
    return base + x - v;
}

// o = the 16 bytes at (aligned address of v0) + sh, sh in 0..15, of the 32 bytes v0 | v1: two rounds of
// dword selects by sh's bits 2 and 3, then one v_alignbyte per dword
__device__ __forceinline__ void take16(uint4 v0, uint4 v1, uint32_t sh, uint32_t o[4]) {
    const bool b2 = sh & 4u, b3 = sh & 8u;
    const uint32_t t0 = b2 ? v0.y : v0.x, t1 = b2 ? v0.z : v0.y, t2 = b2 ? v0.w : v0.z, t3 = b2 ? v1.x : v0.w;
    const uint32_t t4 = b2 ? v1.y : v1.x, t5 = b2 ? v1.z : v1.y, t6 = b2 ? v1.w : v1.z;
    const uint32_t u0 = b3 ? t2 : t0, u1 = b3 ? t3 : t1, u2 = b3 ? t4 : t2, u3 = b3 ? t5 : t3, u4 = b3 ? t6 : t4;
    const uint32_t r = sh & 3u;
    o[0] = __builtin_amdgcn_alignbyte(u1, u0, r);
    o[1] = __builtin_amdgcn_alignbyte(u2, u1, r);
    o[2] = __builtin_amdgcn_alignbyte(u3, u2, r);
    o[3] = __builtin_amdgcn_alignbyte(u4, u3, r);
}

// 16 bytes as they lie in memory: lo = bytes 0..7, hi = bytes 8..15.  (U128, pktgpu_device.hpp, is the
// big-endian one.)
struct Le128 {
    uint64_t lo, hi;
};

// ones in bits [0, k), k in 0..128
__device__ __forceinline__ Le128 bits_below(uint32_t k) {
    const uint64_t lo = k >= 64 ? ~0ull : (1ull << k) - 1;
    const uint64_t hi = k <= 64 ? 0ull : k >= 128 ? ~0ull : (1ull << (k - 64)) - 1;
    return Le128{lo, hi};
}

// ones in bytes [0, b), b in 0..16
__device__ __forceinline__ Le128 bytes_below(uint32_t b) {
    const uint64_t lo = b >= 8 ? ~0ull : (1ull << (8u * b)) - 1;
    const uint64_t hi = b <= 8 ? 0ull : b >= 16 ? ~0ull : (1ull << (8u * (b - 8))) - 1;
    return Le128{lo, hi};
}

// v's bytes moved up by b (0..15) places, zeros coming in
__device__ __forceinline__ Le128 bytes_up(Le128 v, uint32_t b) {
    const uint32_t s = 8u * (b & 7u);
    if (b >= 8) return Le128{0, v.lo << s};
    if (!s) return v;
    return Le128{v.lo << s, v.hi << s | v.lo >> (64u - s)};
}

// v's bytes moved down by b (0..15) places
__device__ __forceinline__ Le128 bytes_down(Le128 v, uint32_t b) {
    const uint32_t s = 8u * (b & 7u);
    if (b >= 8) return Le128{v.hi >> s, 0};
    if (!s) return v;
    return Le128{v.lo >> s | v.hi << (64u - s), v.hi >> s};
}

// The flattened chunk walk: a wave's 64 items (packets, pairs) hold `chunks` 16-byte chunks each, the wave keeps
// the exclusive prefix of the counts in LDS (pre[0..64], pre[64] = the total) and its lanes take the chunks 64 at
// a time, so that one long item costs its bytes, not 64 times its length.  locate() finds flat chunk f's item p
// and its chunk k within it.  Every item with the same count c (a batch of equal-length packets): p = f / c, by
// a multiplication (exact for f < 2^18, c <= 4097); otherwise a search in the prefix.
// (Plain values in and out: with p and k as reference parameters the kernels' code came out different.)
struct FlatWalk {
    bool uni;
    uint32_t c_uni, magic;
};
struct FlatAt {
    uint32_t p, k;
};
__device__ __forceinline__ FlatWalk flat_walk(uint32_t chunks) {
    const uint32_t c_uni = __builtin_amdgcn_readfirstlane(chunks);
    const bool uni = c_uni > 1 && __ballot(chunks == c_uni) == ~0ull;
    const uint32_t magic = uni ? 0xFFFFFFFFu / c_uni + 1u : 0u;
    return FlatWalk{uni, c_uni, magic};
}
__device__ __forceinline__ FlatAt locate(FlatWalk w, const uint32_t* pre, uint32_t f) {
    uint32_t p, k;
    if (w.uni) {
        p = __umulhi(f, w.magic);
        k = f - p * w.c_uni;
    } else {
        // the item holding flat chunk f: the number of prefix ends at or below f
        p = 0;
#pragma unroll
        for (uint32_t st = 32; st; st >>= 1)
            if (pre[p + st] <= f) p += st;
        k = f - pre[p];
    }
    return FlatAt{p, k};
}

// Packet i's n_hdrs and the first 4 rows of its slot-major chain columns ([PKT_MAX_HDRS][n]), loaded
// unconditionally (rows past n_hdrs are readable; their bytes are never used), so that they are in flight together
// with the caller's other loads: one memory round trip for the common chains instead of one per slot.
static_assert(PKT_MAX_HDRS >= 4, "first 4 slot rows loaded unconditionally");
struct ChainPre {
    uint32_t nh, ty[4], of[4];
};
template <typename Cols>  // Cols: n_hdrs, hdr_type, hdr_off and n (a kernel's parameter struct)
__device__ __forceinline__ ChainPre chain_load(const Cols& b, uint64_t i) {
    ChainPre c;
    c.nh = b.n_hdrs[i];
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) {
        c.ty[j] = b.hdr_type[(uint64_t)j * b.n + i];
        c.of[j] = b.hdr_off[(uint64_t)j * b.n + i];
    }
    return c;
}

#endif  // __HIPCC__
