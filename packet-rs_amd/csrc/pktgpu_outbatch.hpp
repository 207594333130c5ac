// pktgpu_outbatch.hpp — the output-batch contract pkt_frag_*, pkt_reasm_* and pkt_icmp_err_* share: source packets
// become output packets packed at 16-byte-aligned offsets of a second slab, with a per-output table (out_off, out_len,
// src_index, out_chain) whose tail up to out_cap is empty, a sizing pass (*_NO_WRITE) and an overflow verdict.
//   host and device: the rounding and the overflow rule, the refusals every entry ends in, the out_chain's columns
//                    as writable pointers and the empty tail as the host twins write it (pktgpu_host.cpp, g++ alone);
//   device only:     the clamped 16-byte slab loads of the copy walks and the per-status `hits` counters.
// The tile scan with the verdict and the call plumbing are pktgpu_outbatch.hip's (declared in pktgpu_ctx.hpp).
#pragma once
#include <cstdint>

#include "pktgpu_batch.hpp"

PKT_HD uint32_t out_round16(uint32_t x) { return (x + 15u) & ~15u; }

// did the outputs fit what the caller gave? (the device decides it in the scan kernel, the host after its first pass)
PKT_HD bool out_overflow(uint64_t n_out, uint64_t bytes, uint64_t out_cap, uint64_t dst_len) {
    return n_out > out_cap || n_out >= (1ull << 32) || bytes > dst_len;
}

// The refusals the three entries end in, after their own (b and chain are not null): the text, or nullptr.
// null_out: the entry's text for a missing dst / out_off / out_len, which names its NO_WRITE flag.
// device: the slab's alignment rule; else the host twin.
inline const char* out_call_error(const pkt_batch_t* b, const pkt_chain_t* chain, bool no_write, const char* null_out,
                                  const uint8_t* dst, uint64_t out_cap, const uint64_t* out_off, const uint32_t* out_len,
                                  const uint64_t* hits, bool device) {
    if ((uintptr_t)hits & 7) return "hits not 8-byte aligned";
    if ((uintptr_t)dst & 15) return "dst not 16-byte aligned";
    if ((uintptr_t)out_off & 7) return "out_off not 8-byte aligned";
    if (!no_write) {
        if (!dst || !out_off || !out_len) return null_out;
        if (out_cap == 0 || out_cap >= (1ull << 32)) return "out_cap is 0 or >= 2^32";
    }
    if (b->n) {
        if (!chain->n_hdrs || !chain->hdr_type || !chain->hdr_off) return "null chain column";
        const char* msg = device ? batch_slab16_error(b) : batch_null_slab(b) ? "null slab" : nullptr;
        if (msg) return msg;
        return batch_index_error(b);
    }
    return nullptr;
}

// out_chain's columns as the writers take them (all null without an out_chain)
struct OutChainCols {
    uint8_t* nh;
    uint8_t* ty;
    uint16_t* of;
};
inline OutChainCols out_chain_cols(const pkt_chain_t* oc) {
    if (!oc) return OutChainCols{nullptr, nullptr, nullptr};
    return OutChainCols{const_cast<uint8_t*>(oc->n_hdrs), const_cast<uint8_t*>(oc->hdr_type), const_cast<uint16_t*>(oc->hdr_off)};
}

// The empty tail [q, out_cap) of the per-output arrays, as a host twin writes it.  extra: the entry's own column.
template <typename T>
inline void out_empty_tail(uint64_t q, uint64_t out_cap, uint64_t* out_off, uint32_t* out_len, uint32_t* src_index,
                           T* extra, uint8_t* oc_nh) {
    static_assert(PKT_FRAG_NONE == PKT_REASM_NONE && PKT_FRAG_NONE == PKT_ICMPE_NONE, "one NONE");
    for (; q < out_cap; q++) {
        out_off[q] = 0;
        out_len[q] = 0;
        if (src_index) src_index[q] = PKT_FRAG_NONE;
        if (extra) extra[q] = 0;
        if (oc_nh) oc_nh[q] = 0;
    }
}

#ifdef __HIPCC__

// the slab's last aligned 16-byte chunk (slab_len > 0 wherever a packet has a byte)
__device__ __forceinline__ uint64_t slab_last16(const BatchSrc& s) {
    return s.slab_len ? ((s.slab_len + 15) & ~(uint64_t)15) - 16 : 0;
}

// the 16 slab bytes from `pos` on, pos < slab_len, as four little-endian dwords / as a Le128: the second aligned chunk
// is clamped to the slab's last one (what it then gives lies past the slab, so past every packet: the caller masks it
// off or does not use it)
__device__ __forceinline__ void load16w(const uint8_t* slab, uint64_t pos, uint64_t last16, uint32_t o[4]) {
    const uint64_t A = pos & ~(uint64_t)15;
    const uint64_t B = A + 16 > last16 ? last16 : A + 16;
    const uint4 v0 = *reinterpret_cast<const uint4*>(slab + A);
    const uint4 v1 = *reinterpret_cast<const uint4*>(slab + B);
    take16(v0, v1, (uint32_t)pos & 15u, o);
}
__device__ __forceinline__ Le128 le128(const uint32_t o[4]) {
    return Le128{(uint64_t)o[0] | (uint64_t)o[1] << 32, (uint64_t)o[2] | (uint64_t)o[3] << 32};
}
__device__ __forceinline__ Le128 load16(const uint8_t* slab, uint64_t pos, uint64_t last16) {
    uint32_t o[4];
    load16w(slab, pos, last16, o);
    return le128(o);
}

// The per-status `hits` of a counting kernel, N statuses: an LDS word per status (s_hits[N]), zeroed by the block,
// one ballot per status and tile, one agent-scope add per block and non-zero status.  Every thread of the block calls
// each (they hold the block's barriers); the caller skips all three when no hits were asked for.
template <uint32_t N>
__device__ __forceinline__ void hits_zero(uint32_t* s_hits, uint32_t t) {  // t: threadIdx.x
    if (t < N) s_hits[t] = 0;
    __syncthreads();
}
template <uint32_t N>
__device__ __forceinline__ void hits_add(uint32_t* s_hits, uint32_t t, bool act, uint32_t st) {
    const uint32_t lane = t & 63u;
#pragma unroll
    for (uint32_t s = 0; s < N; s++) {
        const uint64_t b = __ballot(act && st == s);
        if (lane == 0 && b) atomicAdd(&s_hits[s], (uint32_t)__popcll((unsigned long long)b));
    }
}
template <uint32_t N>
__device__ __forceinline__ void hits_flush(const uint32_t* s_hits, uint32_t t, uint64_t* hits) {
    __syncthreads();
    if (t < N) {
        const uint64_t h = s_hits[t];  // (64 bits here: widened inside the add, two of the callers' instructions moved)
        if (h) __hip_atomic_fetch_add(hits + t, h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

#endif  // __HIPCC__
