// pktgpu.hip — the parse kernels of the MI355X batched parser and the code that launches them.
//
// Kernels
//   parse_kernel<NCH>       fast::parse_<entry> over a batch: per-lane windows of NCH 16-byte
//                           chunks staged in LDS, the chain walk, and the fused field/checksum
//                           extraction of the first Ether/Vlan/IPv4/IPv6/TCP/UDP (Q11).
//   parse_span_kernel<NCH>  the same with wave spans staged by LDS-DMA (pkt_ctx_set_staging 2).
//   parse_multi_kernel<NCH> parse_kernel over several same-shaped batches in one launch.
//   max_hdrs_kernel         the largest n_hdrs of a batch (pkt_chain_max_hdrs).
// C ABI (include/pktgpu.h): pkt_parse_batch, pkt_parse_batches, pkt_chain_max_hdrs; internal entries
// (pktgpu_ctx.hpp): pktgpu_parse and its two wrappers, pktgpu_ensure_max_scratch.  The ctx and its knobs:
// pktgpu_ctx.cpp; the host-memory paths: pktgpu_hostpath.cpp; the other kernels: see pktgpu_ctx.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "pktgpu_ctx.hpp"
#include "pktgpu_device.hpp"

using namespace pktgpu;

namespace {

// Output column groups.  A kernel is specialised on GM = the groups whose columns are ALL
// requested (no per-column checks at all), or GM = G_RUNTIME (each column checked for NULL).
enum : uint32_t {
    G_CHAIN = 1, G_ETHER = 2, G_VLAN = 4, G_IPV4 = 8, G_IPV6 = 16, G_TCP = 32, G_UDP = 64,
    G_ALL = 127, G_RUNTIME = 128,
    // flag: store the columns non-temporally.  Set for the indexed-batch (lockstep) kernels: C4
    // isolated 105 -> 98 us, pipelined 86 -> 82.5 us, line requests 2.39M -> 2.29M (the columns
    // no longer evict the records' lines from L2); fixed-stride C2 keeps plain stores (pipelined
    // +0.3 us with them), profiles/ab/r02ntst_nt_column_stores.txt
    G_NT = 256
};

template <uint32_t GM, uint32_t G>
__device__ __forceinline__ bool want(const void* p) {
    if constexpr ((GM & G_RUNTIME) != 0) return p != nullptr;
    else return (GM & G) != 0;
}

// Store at a 32-bit byte offset from a column base (global_store ... saddr: one VGPR offset).
template <bool NT, class T>
__device__ __forceinline__ void st(T* base, uint32_t boff, T v) {
    if constexpr (NT && std::is_integral<T>::value)
        __builtin_nontemporal_store(v, reinterpret_cast<T*>(reinterpret_cast<char*>(base) + boff));
    else
        *reinterpret_cast<T*>(reinterpret_cast<char*>(base) + boff) = v;
}

// Record (type, offset) in header slot `slot` of packet i (slot-major columns, row stride ns = the
// batch size): 32-bit byte offsets from the column bases while every slot row of the batch lies
// within 4 GiB of them (ns <= 2^27, a wave-uniform branch), the 64-bit products beyond.
template <uint32_t GM>
__device__ __forceinline__ void push_slot(const pkt_out_t& out, uint64_t ns, uint32_t slot, uint32_t i, uint32_t ty,
                                          uint32_t o) {
    if (ns <= (1ull << 27)) {
        const uint32_t e = slot * (uint32_t)ns + i;
        if (want<GM, G_CHAIN>(out.hdr_type)) st<false, uint8_t>(out.hdr_type, e, (uint8_t)ty);
        if (want<GM, G_CHAIN>(out.hdr_off)) st<false, uint16_t>(out.hdr_off, 2u * e, (uint16_t)o);
    } else {
        if (want<GM, G_CHAIN>(out.hdr_type)) out.hdr_type[(uint64_t)slot * ns + i] = (uint8_t)ty;
        if (want<GM, G_CHAIN>(out.hdr_off)) out.hdr_off[(uint64_t)slot * ns + i] = (uint16_t)o;
    }
}

// Fields of the first header of each group (Q11), from the walk's first offsets.
// `i` is the packet index within this launch (< kLaunchChunk = 2^26, so every per-packet byte
// offset, up to i * 16 for the IPv6 addresses, fits 32 bits).
template <uint32_t GM, class View>
__device__ __forceinline__ void emit_fields(const pkt_out_t& out, uint32_t i, const View& pv,
                                            const WalkResult& r, bool ok) {
    const uint32_t o1 = i, o2 = i * 2u, o4 = i * 4u, o8 = i * 8u, o16 = i * 16u;
    // Ether (headers.rs:530-540): dst 0-47, src 48-95, etype 96-111
    if (want<GM, G_ETHER>(out.eth_dst) || want<GM, G_ETHER>(out.eth_src) || want<GM, G_ETHER>(out.eth_etype)) {
        uint32_t d[4] = {0, 0, 0, 0};
        const bool h = ok && r.f_eth >= 0;
        if (h) pv.template hdr<4>((uint32_t)r.f_eth, 14, d);
        if (want<GM, G_ETHER>(out.eth_dst)) st<(GM & G_NT) != 0, uint64_t>(out.eth_dst, o8, ((uint64_t)d[0] << 16) | (d[1] >> 16));
        if (want<GM, G_ETHER>(out.eth_src)) st<(GM & G_NT) != 0, uint64_t>(out.eth_src, o8, ((uint64_t)(d[1] & 0xFFFFu) << 32) | d[2]);
        if (want<GM, G_ETHER>(out.eth_etype)) st<(GM & G_NT) != 0, uint16_t>(out.eth_etype, o2, (uint16_t)(d[3] >> 16));
    }
    // Vlan (headers.rs:543-552): pcp 0-2, cfi 3, vid 4-15, etype 16-31
    if (want<GM, G_VLAN>(out.vlan_pcp) || want<GM, G_VLAN>(out.vlan_cfi) || want<GM, G_VLAN>(out.vlan_vid) ||
        want<GM, G_VLAN>(out.vlan_etype)) {
        uint32_t d[1] = {0};
        if (ok && r.f_vlan >= 0) pv.template hdr<1>((uint32_t)r.f_vlan, 4, d);
        if (want<GM, G_VLAN>(out.vlan_pcp)) st<(GM & G_NT) != 0, uint8_t>(out.vlan_pcp, o1, (uint8_t)(d[0] >> 29));
        if (want<GM, G_VLAN>(out.vlan_cfi)) st<(GM & G_NT) != 0, uint8_t>(out.vlan_cfi, o1, (uint8_t)((d[0] >> 28) & 1u));
        if (want<GM, G_VLAN>(out.vlan_vid)) st<(GM & G_NT) != 0, uint16_t>(out.vlan_vid, o2, (uint16_t)((d[0] >> 16) & 0xFFFu));
        if (want<GM, G_VLAN>(out.vlan_etype)) st<(GM & G_NT) != 0, uint16_t>(out.vlan_etype, o2, (uint16_t)(d[0] & 0xFFFFu));
    }
    // IPv4 (headers.rs:555-574) + Packet::ipv4_checksum (packet.rs:93-107)
    if (want<GM, G_IPV4>(out.ipv4_version) || want<GM, G_IPV4>(out.ipv4_ihl) || want<GM, G_IPV4>(out.ipv4_diffserv) ||
        want<GM, G_IPV4>(out.ipv4_total_len) || want<GM, G_IPV4>(out.ipv4_identification) ||
        want<GM, G_IPV4>(out.ipv4_flags) || want<GM, G_IPV4>(out.ipv4_frag_startset) || want<GM, G_IPV4>(out.ipv4_ttl) ||
        want<GM, G_IPV4>(out.ipv4_protocol) || want<GM, G_IPV4>(out.ipv4_header_checksum) ||
        want<GM, G_IPV4>(out.ipv4_src) || want<GM, G_IPV4>(out.ipv4_dst) || want<GM, G_IPV4>(out.ipv4_csum_calc)) {
        uint32_t d[5] = {0, 0, 0, 0, 0};
        const bool h = ok && r.f_ipv4 >= 0;
        if (h) pv.template hdr<5>((uint32_t)r.f_ipv4, 20, d);
        if (want<GM, G_IPV4>(out.ipv4_version)) st<(GM & G_NT) != 0, uint8_t>(out.ipv4_version, o1, (uint8_t)(d[0] >> 28));
        if (want<GM, G_IPV4>(out.ipv4_ihl)) st<(GM & G_NT) != 0, uint8_t>(out.ipv4_ihl, o1, (uint8_t)((d[0] >> 24) & 0xFu));
        if (want<GM, G_IPV4>(out.ipv4_diffserv)) st<(GM & G_NT) != 0, uint8_t>(out.ipv4_diffserv, o1, (uint8_t)((d[0] >> 16) & 0xFFu));
        if (want<GM, G_IPV4>(out.ipv4_total_len)) st<(GM & G_NT) != 0, uint16_t>(out.ipv4_total_len, o2, (uint16_t)(d[0] & 0xFFFFu));
        if (want<GM, G_IPV4>(out.ipv4_identification)) st<(GM & G_NT) != 0, uint16_t>(out.ipv4_identification, o2, (uint16_t)(d[1] >> 16));
        if (want<GM, G_IPV4>(out.ipv4_flags)) st<(GM & G_NT) != 0, uint8_t>(out.ipv4_flags, o1, (uint8_t)((d[1] >> 13) & 7u));
        if (want<GM, G_IPV4>(out.ipv4_frag_startset)) st<(GM & G_NT) != 0, uint16_t>(out.ipv4_frag_startset, o2, (uint16_t)(d[1] & 0x1FFFu));
        if (want<GM, G_IPV4>(out.ipv4_ttl)) st<(GM & G_NT) != 0, uint8_t>(out.ipv4_ttl, o1, (uint8_t)(d[2] >> 24));
        if (want<GM, G_IPV4>(out.ipv4_protocol)) st<(GM & G_NT) != 0, uint8_t>(out.ipv4_protocol, o1, (uint8_t)((d[2] >> 16) & 0xFFu));
        if (want<GM, G_IPV4>(out.ipv4_header_checksum)) st<(GM & G_NT) != 0, uint16_t>(out.ipv4_header_checksum, o2, (uint16_t)(d[2] & 0xFFFFu));
        if (want<GM, G_IPV4>(out.ipv4_src)) st<(GM & G_NT) != 0, uint32_t>(out.ipv4_src, o4, d[3]);
        if (want<GM, G_IPV4>(out.ipv4_dst)) st<(GM & G_NT) != 0, uint32_t>(out.ipv4_dst, o4, d[4]);
        if (want<GM, G_IPV4>(out.ipv4_csum_calc)) {
            // nine BE words, word 5 (byte offset 10) skipped; fold ((s>>16)+s)&0xFFFF (Q1)
            uint32_t s = (d[0] >> 16) + (d[0] & 0xFFFFu) + (d[1] >> 16) + (d[1] & 0xFFFFu) +
                         (d[2] >> 16) + (d[3] >> 16) + (d[3] & 0xFFFFu) + (d[4] >> 16) + (d[4] & 0xFFFFu);
            s = ((s >> 16) + s) & 0xFFFFu;
            st<(GM & G_NT) != 0, uint16_t>(out.ipv4_csum_calc, o2, h ? (uint16_t)(~s) : (uint16_t)0);
        }
    }
    // IPv6 (headers.rs:577-592); src/dst as the raw 16 bytes of bytes(msb, lsb)
    if (want<GM, G_IPV6>(out.ipv6_version) || want<GM, G_IPV6>(out.ipv6_traffic_class) ||
        want<GM, G_IPV6>(out.ipv6_flow_label) || want<GM, G_IPV6>(out.ipv6_payload_len) ||
        want<GM, G_IPV6>(out.ipv6_next_hdr) || want<GM, G_IPV6>(out.ipv6_hop_limit) ||
        want<GM, G_IPV6>(out.ipv6_src) || want<GM, G_IPV6>(out.ipv6_dst)) {
        uint32_t d[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (ok && r.f_ipv6 >= 0) pv.template hdr<10>((uint32_t)r.f_ipv6, 40, d);
        if (want<GM, G_IPV6>(out.ipv6_version)) st<(GM & G_NT) != 0, uint8_t>(out.ipv6_version, o1, (uint8_t)(d[0] >> 28));
        if (want<GM, G_IPV6>(out.ipv6_traffic_class)) st<(GM & G_NT) != 0, uint8_t>(out.ipv6_traffic_class, o1, (uint8_t)((d[0] >> 20) & 0xFFu));
        if (want<GM, G_IPV6>(out.ipv6_flow_label)) st<(GM & G_NT) != 0, uint32_t>(out.ipv6_flow_label, o4, d[0] & 0xFFFFFu);
        if (want<GM, G_IPV6>(out.ipv6_payload_len)) st<(GM & G_NT) != 0, uint16_t>(out.ipv6_payload_len, o2, (uint16_t)(d[1] >> 16));
        if (want<GM, G_IPV6>(out.ipv6_next_hdr)) st<(GM & G_NT) != 0, uint8_t>(out.ipv6_next_hdr, o1, (uint8_t)((d[1] >> 8) & 0xFFu));
        if (want<GM, G_IPV6>(out.ipv6_hop_limit)) st<(GM & G_NT) != 0, uint8_t>(out.ipv6_hop_limit, o1, (uint8_t)(d[1] & 0xFFu));
        if (want<GM, G_IPV6>(out.ipv6_src))
            st<(GM & G_NT) != 0, uint4>(reinterpret_cast<uint4*>(out.ipv6_src), o16,
                      make_uint4(bswap32(d[2]), bswap32(d[3]), bswap32(d[4]), bswap32(d[5])));
        if (want<GM, G_IPV6>(out.ipv6_dst))
            st<(GM & G_NT) != 0, uint4>(reinterpret_cast<uint4*>(out.ipv6_dst), o16,
                      make_uint4(bswap32(d[6]), bswap32(d[7]), bswap32(d[8]), bswap32(d[9])));
    }
    // TCP (headers.rs:606-622)
    if (want<GM, G_TCP>(out.tcp_src) || want<GM, G_TCP>(out.tcp_dst) || want<GM, G_TCP>(out.tcp_seq_no) ||
        want<GM, G_TCP>(out.tcp_ack_no) || want<GM, G_TCP>(out.tcp_data_startset) || want<GM, G_TCP>(out.tcp_res) ||
        want<GM, G_TCP>(out.tcp_flags) || want<GM, G_TCP>(out.tcp_window) || want<GM, G_TCP>(out.tcp_checksum) ||
        want<GM, G_TCP>(out.tcp_urgent_ptr)) {
        uint32_t d[5] = {0, 0, 0, 0, 0};
        if (ok && r.f_tcp >= 0) pv.template hdr<5>((uint32_t)r.f_tcp, 20, d);
        if (want<GM, G_TCP>(out.tcp_src)) st<(GM & G_NT) != 0, uint16_t>(out.tcp_src, o2, (uint16_t)(d[0] >> 16));
        if (want<GM, G_TCP>(out.tcp_dst)) st<(GM & G_NT) != 0, uint16_t>(out.tcp_dst, o2, (uint16_t)(d[0] & 0xFFFFu));
        if (want<GM, G_TCP>(out.tcp_seq_no)) st<(GM & G_NT) != 0, uint32_t>(out.tcp_seq_no, o4, d[1]);
        if (want<GM, G_TCP>(out.tcp_ack_no)) st<(GM & G_NT) != 0, uint32_t>(out.tcp_ack_no, o4, d[2]);
        if (want<GM, G_TCP>(out.tcp_data_startset)) st<(GM & G_NT) != 0, uint8_t>(out.tcp_data_startset, o1, (uint8_t)(d[3] >> 28));
        if (want<GM, G_TCP>(out.tcp_res)) st<(GM & G_NT) != 0, uint8_t>(out.tcp_res, o1, (uint8_t)((d[3] >> 24) & 0xFu));
        if (want<GM, G_TCP>(out.tcp_flags)) st<(GM & G_NT) != 0, uint8_t>(out.tcp_flags, o1, (uint8_t)((d[3] >> 16) & 0xFFu));
        if (want<GM, G_TCP>(out.tcp_window)) st<(GM & G_NT) != 0, uint16_t>(out.tcp_window, o2, (uint16_t)(d[3] & 0xFFFFu));
        if (want<GM, G_TCP>(out.tcp_checksum)) st<(GM & G_NT) != 0, uint16_t>(out.tcp_checksum, o2, (uint16_t)(d[4] >> 16));
        if (want<GM, G_TCP>(out.tcp_urgent_ptr)) st<(GM & G_NT) != 0, uint16_t>(out.tcp_urgent_ptr, o2, (uint16_t)(d[4] & 0xFFFFu));
    }
    // UDP (headers.rs:625-634)
    if (want<GM, G_UDP>(out.udp_src) || want<GM, G_UDP>(out.udp_dst) || want<GM, G_UDP>(out.udp_length) ||
        want<GM, G_UDP>(out.udp_checksum)) {
        uint32_t d[2] = {0, 0};
        if (ok && r.f_udp >= 0) pv.template hdr<2>((uint32_t)r.f_udp, 8, d);
        if (want<GM, G_UDP>(out.udp_src)) st<(GM & G_NT) != 0, uint16_t>(out.udp_src, o2, (uint16_t)(d[0] >> 16));
        if (want<GM, G_UDP>(out.udp_dst)) st<(GM & G_NT) != 0, uint16_t>(out.udp_dst, o2, (uint16_t)(d[0] & 0xFFFFu));
        if (want<GM, G_UDP>(out.udp_length)) st<(GM & G_NT) != 0, uint16_t>(out.udp_length, o2, (uint16_t)(d[1] >> 16));
        if (want<GM, G_UDP>(out.udp_checksum)) st<(GM & G_NT) != 0, uint16_t>(out.udp_checksum, o2, (uint16_t)(d[1] & 0xFFFFu));
    }
}

// Packet i's start (byte offset in the slab) and length, clamped to the slab so that no read
// can leave the caller's allocation whatever the batch description says.
__device__ __forceinline__ void packet_range(const KParams& p, uint32_t i, uint64_t& off,
                                             uint32_t& len) {
    if (p.offsets) {
        off = p.offsets[i] - p.off_bias;
        len = p.lens[i];
    } else {
        off = (p.i0 + i) * (uint64_t)p.stride;
        if (p.lens) len = p.lens[i];
        else len = p.stride;
    }
    uint64_t room = off < p.slab_len ? p.slab_len - off : 0;
    if ((uint64_t)len > room) len = (uint32_t)room;
    if (len > 0xFFFFu) len = 0xFFFFu;  // u16 offsets/lengths in the ABI
}

// Dynamic LDS of a parse block (base 16-byte aligned; nothing static in front of it): the packet
// windows, packet-major: packet q's window at q * lane_stride, lane_stride = 4*NCH+1 dwords (odd, so the
// per-lane dword reads of the walk hit 64 distinct banks); +16 B for the last lane's over-read.
// (A chunk-major layout with ds_write_b128 staging had 4-way conflicts on the walk's reads: C4
// 3 % slower, C2/C3 neutral, scripts/ab_bench.sh.)
__host__ __device__ constexpr uint32_t lane_stride(int nch) { return (uint32_t)(4 * nch + 1) * 4u; }
__host__ __device__ constexpr size_t window_lds(int nch) {
    return ((size_t)kBlock * lane_stride(nch) + 16 + 15) & ~(size_t)15;
}

__device__ __forceinline__ PacketView make_view(const KParams& p, uint8_t* lds, uint32_t q, uint64_t off,
                                                uint32_t len, int nch) {
    PacketView pv;
    pv.lw = lds + q * lane_stride(nch);
    pv.slab = p.slab;
    pv.off = off;
    pv.last4 = ((p.slab_len + 15) & ~(uint64_t)15) - 4;
    pv.shift = (uint32_t)(off & 15);
    pv.win_lo = 0;
    pv.win_end = (uint32_t)nch * 16u - pv.shift;
    pv.len = len;
    return pv;
}

template <uint32_t GM>
__device__ __forceinline__ void emit_chain(const pkt_out_t& out, uint32_t i, uint32_t len, const WalkResult& r) {
    const bool ok = r.status == PKT_OK;
    if (want<GM, G_CHAIN>(out.status)) st<(GM & G_NT) != 0, uint8_t>(out.status, i, (uint8_t)r.status);
    if (want<GM, G_CHAIN>(out.n_hdrs)) st<(GM & G_NT) != 0, uint8_t>(out.n_hdrs, i, ok ? (uint8_t)r.n : (uint8_t)0);
    if (want<GM, G_CHAIN>(out.payload_off)) st<(GM & G_NT) != 0, uint16_t>(out.payload_off, 2 * i, ok ? (uint16_t)r.payload_off : (uint16_t)0);
    if (want<GM, G_CHAIN>(out.payload_len)) st<(GM & G_NT) != 0, uint16_t>(out.payload_len, 2 * i, ok ? (uint16_t)(len - r.payload_off) : (uint16_t)0);
    if (want<GM, G_CHAIN>(out.hdr_mask)) st<(GM & G_NT) != 0, uint32_t>(out.hdr_mask, 4 * i, ok ? r.mask : 0u);
}

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

#ifndef PKTGPU_LATE_COLS
#define PKTGPU_LATE_COLS 1  // parse_kernel loads its column bases after the walk (0: at the start)
#endif
#define KARG_AS __attribute__((address_space(4)))
// A generic pointer the caller knows to be global memory, re-marked as such (addrspacecast to global
// and back): loads and stores through it stay global_* instructions instead of flat_*.
template <class T>
__device__ __forceinline__ T* as_global(T* q) {
    return (T*)((__attribute__((address_space(1))) T*)q);
}

// Diagnostic build only (-DPKTGPU_STAMPS=1: scripts/build_variant.sh, read by scripts/stamps.py): s_memtime stamps per wave of the
// parse kernel — start, windows in LDS, walk done, emit issued, stores drained — plus the wave's
// hardware id, written by lane 0 to a debug buffer no other code reads (pkt_debug_stamps).  In the
// normal build no stamp executes.
#ifndef PKTGPU_STAMPS
#define PKTGPU_STAMPS 0
#endif
#if PKTGPU_STAMPS
__device__ uint64_t* g_pkt_stamps;
#define PKT_STAMP(k)                                                                          \
    do {                                                                                      \
        __builtin_amdgcn_sched_barrier(0);                                                    \
        uint64_t t_;                                                                          \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");            \
        __builtin_amdgcn_sched_barrier(0);                                                    \
        pkt_st[k] = t_;                                                                       \
    } while (0)
#else
#define PKT_STAMP(k) \
    do {             \
    } while (0)
#endif

// Lane t's packet range and its first NCH 16-byte chunks (from the 16-byte-aligned start) by
// per-lane dwordx4 loads (faster than the LDS-DMA gather, scripts/probe.py).  Chunks past the
// readable end of the slab (round_up(slab_len, 16)) are clamped to an in-bounds chunk; those
// bytes lie beyond every packet and are never interpreted.
template <int NCH>
__device__ __forceinline__ void load_packet(const KParams& p, uint32_t i, bool active, u32x4 (&chunk)[NCH],
                                            uint64_t& off, uint32_t& len) {
    off = 0;
    len = 0;
    if (active) packet_range(p, i, off, len);
    const uint64_t a0 = off & ~(uint64_t)15;
    const uint64_t last16 = ((p.slab_len + 15) & ~(uint64_t)15) - 16;
#pragma unroll
    for (int c = 0; c < NCH; c++) {
        uint64_t o = a0 + 16u * (uint32_t)c;
        o = o > last16 ? last16 : o;
        chunk[c] = *reinterpret_cast<const u32x4*>(p.slab + o);
    }
}

// Packet q's window: its chunks as dwords at q * lane_stride(NCH) (odd dword stride).
template <int NCH>
__device__ __forceinline__ void stage_window(uint8_t* lds, uint32_t q, const u32x4 (&chunk)[NCH]) {
#pragma unroll
    for (int c = 0; c < NCH; c++) {
        uint32_t* w = reinterpret_cast<uint32_t*>(lds + q * lane_stride(NCH)) + 4 * c;
        w[0] = chunk[c].x;
        w[1] = chunk[c].y;
        w[2] = chunk[c].z;
        w[3] = chunk[c].w;
    }
}

// ---- several batches in one launch (pkt_parse_batches) ----
// K batches of the same size and layout whose outputs lie at one common byte distance from batch
// 0's (e.g. one packed output buffer each): block j parses tile j % bpb of batch j / bpb.  Every
// per-batch value comes from the kernel arguments (a scalar load at a computed offset: no table
// read from memory before the block can start), and the launch's ramp and drain are paid once for
// the K batches instead of once per batch.
constexpr int kMaxMulti = 16;
struct MultiBatch {
    const uint8_t* slab;
    uint64_t slab_len;
    const uint64_t* offsets;
    const uint32_t* lens;
    int64_t out_delta;  // bytes from batch 0's column pointers to this batch's
};
struct MultiParams {
    KParams base;  // batch 0 (its slab, index, outputs), the shared n / stride / entry / knobs
    uint32_t bpb;  // blocks per batch
    uint32_t k;
    MultiBatch per[kMaxMulti];
};
static_assert(offsetof(MultiParams, base) == 0, "the late column loads read base.out at offsetof(KParams, out)");

// Where the emit's column bases come from (LATE): L_EARLY = the KParams the kernel holds since its
// start; L_SINGLE = loaded after the walk from the kernel arguments (parse_kernel: one KParams);
// L_MULTI = the same from a MultiParams (its base.out) plus batch `mb`'s out_delta, also loaded after
// the walk (parse_multi_kernel).
enum LateCols : int { L_EARLY = 0, L_SINGLE = 1, L_MULTI = 2 };

template <int NCH, uint32_t GM, int WK, bool STAGED = false, int LATE = L_EARLY>
__device__ __forceinline__ void parse_tile(const KParams& p, uint8_t* lds, uint32_t base,
                                           const u32x4 (&chunk)[NCH], uint64_t off_own, uint32_t len_own,
                                           bool active_own, uint64_t* pkt_st, const DispatchLds* T, uint32_t mb);

// Dynamic LDS of a lockstep launch: the windows (or spans), then the dispatch tables.
__host__ __device__ constexpr size_t with_tables(size_t bytes, int wk) {
    return wk == 1 ? ((bytes + 15) & ~(size_t)15) + sizeof(DispatchLds) : bytes;
}
template <int WK>
__device__ __forceinline__ const DispatchLds* tables(uint8_t* lds, size_t at, uint32_t t, uint32_t nt) {
    if constexpr (WK != 1) return nullptr;
    DispatchLds* T = reinterpret_cast<DispatchLds*>(lds + ((at + 15) & ~(size_t)15));
    dispatch_init(T, t, nt);
    __syncthreads();
    return T;
}

// One block = 256 packets, one lane per packet.  (A persistent grid of k blocks per CU striding
// over the tiles, each lane's loads of its next packet in flight while it parsed the current one,
// was measured no faster at k = 4 and slower at k = 1, 2: DESIGN.md §5.)
// Resident waves per SIMD the compiler may assume (VGPR budget 512 / waves): 8 for fixed-stride
// windows (<= 64 VGPRs); for indexed windows what their LDS allows anyway — 6 for the 96-byte
// windows (25.6 KB per block, 6 blocks per CU), 5 for the 112-byte ones (29.7 KB, 5 blocks), 4 for
// the 144-byte ones (37.9 KB, 4 blocks); wider windows unconstrained.
__host__ __device__ constexpr int waves_per_eu(int nch, int wk) {
    return nch > 9 ? 1 : (wk == 1 && nch >= 6 ? (nch == 9 ? 4 : nch == 7 ? 5 : 6) : 8);
}
// Tile `blk` (256 packets) of the batch `p` describes: load, stage, walk, emit.
template <int NCH, uint32_t GM, int WK, int LATE = L_EARLY>
__device__ __forceinline__ void parse_block(const KParams& p, uint32_t blk, uint8_t* lds, const DispatchLds* T,
                                            uint64_t* pkt_st, uint32_t mb = 0) {
    uint32_t base = blk * (uint32_t)kBlock;  // within this launch
    uint32_t n_eff = p.n;
    if (p.n_dev) {  // wave-uniform: the count the device produced (scalar load)
        const uint64_t nd = *p.n_dev;
        n_eff = nd < (uint64_t)n_eff ? (uint32_t)nd : n_eff;
        if (p.i0_dev) base += (uint32_t)*p.i0_dev;  // the launch starts at a device-produced index
        if (base >= n_eff) return;  // the whole block is past the count
    }
    const bool act = base + threadIdx.x < n_eff;
    u32x4 chunk[NCH];
    uint64_t off;
    uint32_t len;
    if constexpr (NCH >= 4) {
        // The wave loads its 64 windows cooperatively: the 64*NCH (packet, chunk) pairs, pair
        // 64k + lane in load k, so consecutive lanes fetch consecutive 16-byte chunks of one packet
        // and each window comes from one or two wave instructions — the per-lane shape (each lane
        // fetching its own chunks) is request-bound, 42 us for the 2^20 C4 windows alone
        // (scripts/probe_c4.py), and separate instructions to the same 128-B line re-request it from
        // memory (scripts/fetch_calib.py).  Each chunk goes straight into the owning lane's LDS
        // window.  C4 pipelined 78 vs 82 us/step, C2 23.9 vs 25.2, C3 43.3 vs 46.1 against per-lane
        // loads (profiles/ab/r02p_c4_coop_windows.txt, r02x_coop_fixed_stride.txt).
        // Lockstep (indexed) launches skip the chunks that start past their packet's end: a short
        // record (Dot3, ARP) fetches only its own lines.
        off = 0;
        len = 0;
        if (act) packet_range(p, base + threadIdx.x, off, len);
        const uint32_t wl = threadIdx.x & 63u, wave0 = threadIdx.x & ~63u;
        const uint64_t last16 = ((p.slab_len + 15) & ~(uint64_t)15) - 16;
#pragma unroll
        for (uint32_t k = 0; k < (uint32_t)NCH; k++) {
            const uint32_t pid = 64u * k + wl, r = pid / (uint32_t)NCH, c = pid % (uint32_t)NCH;
            const uint64_t offr = ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(off >> 32), (int)r, 64) << 32) |
                                  (uint32_t)__shfl((int)(uint32_t)off, (int)r, 64);
            if constexpr (WK == 1) {
                const uint32_t lenr = (uint32_t)__shfl((int)len, (int)r, 64);
                if (16u * c >= (uint32_t)(offr & 15) + lenr) continue;  // chunk past the packet
            }
            uint64_t a = (offr & ~(uint64_t)15) + 16u * c;
            a = a > last16 ? last16 : a;
            const u32x4 v = *reinterpret_cast<const u32x4*>(p.slab + a);
            uint32_t* w = reinterpret_cast<uint32_t*>(lds + (wave0 + r) * lane_stride(NCH)) + 4 * c;
            w[0] = v.x;
            w[1] = v.y;
            w[2] = v.z;
            w[3] = v.w;
        }
        wave_sync();
        PKT_STAMP(1);
        parse_tile<NCH, GM, WK, true, LATE>(p, lds, base, chunk, off, len, act, pkt_st, T, mb);
        return;
    }
    load_packet<NCH>(p, base + threadIdx.x, act, chunk, off, len);
    parse_tile<NCH, GM, WK, false, LATE>(p, lds, base, chunk, off, len, act, pkt_st, T, mb);
}

template <int NCH, uint32_t GM, int WK>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(waves_per_eu(NCH, WK))))
void parse_kernel(KParams p) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    uint64_t pkt_st[5] = {0, 0, 0, 0, 0};
    PKT_STAMP(0);
    const DispatchLds* T = tables<WK>(lds, window_lds(NCH), threadIdx.x, kBlock);
    parse_block<NCH, GM, WK, PKTGPU_LATE_COLS != 0 ? L_SINGLE : L_EARLY>(p, blockIdx.x, lds, T, pkt_st);
}

// Block j parses tile j % bpb of batch j / bpb.  Only the slot columns (hdr_type / hdr_off, which
// the walk writes) are moved to the batch at the kernel start; the other 47 column bases and the
// batch's out_delta are loaded after the walk (L_MULTI), as parse_kernel does: adding the delta to
// all 49 bases up front held them through the walk and spilled 36 (C2 columns) / 42 (C4, all
// columns) SGPRs to VGPR lanes (round-4 review).
template <int NCH, uint32_t GM, int WK>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(waves_per_eu(NCH, WK))))
void parse_multi_kernel(MultiParams mp) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    uint64_t pkt_st[5] = {0, 0, 0, 0, 0};
    const DispatchLds* T = tables<WK>(lds, window_lds(NCH), threadIdx.x, kBlock);
    const uint32_t b = blockIdx.x / mp.bpb;  // wave-uniform
    const MultiBatch& mb = mp.per[b];
    KParams p = mp.base;
    p.slab = mb.slab;
    p.slab_len = mb.slab_len;
    p.offsets = mb.offsets;
    p.lens = mb.lens;
    if (p.out.hdr_type) p.out.hdr_type += mb.out_delta;
    if (p.out.hdr_off) p.out.hdr_off = reinterpret_cast<uint16_t*>(reinterpret_cast<uint8_t*>(p.out.hdr_off) + mb.out_delta);
    parse_block<NCH, GM, WK, L_MULTI>(p, blockIdx.x - b * mp.bpb, lds, T, pkt_st, b);
}

// The emit of one column group with its bases loaded from the kernel arguments right here (LATE): columns
// [LO, HI) of pkt_out_t (group G), through an opaque copy of their address taken after a compiler memory
// barrier, so the loads come after the previous group's stores.  One group's bases live at a time (at most
// 13 pointers): the all-columns and C3 emits held every group's (~40 bases, 80 SGPRs) at once and spilled
// 32-74 SGPRs to VGPR lanes (round-5 review).
template <uint32_t GM, uint32_t G, int LO, int HI, int LATE, class View>
__device__ __forceinline__ void emit_group_late(uint64_t kseg, int64_t delta, uint32_t i, uint32_t len, const View& pv,
                                                const WalkResult& r) {
    constexpr bool rt = (GM & G_RUNTIME) != 0;
    if constexpr (rt || (GM & G) != 0) {
        uint64_t ka = kseg + offsetof(KParams, out) + sizeof(void*) * LO;
        asm volatile("" : "+s"(ka)::"memory");
        const void* const KARG_AS* kc = reinterpret_cast<const void* const KARG_AS*>(ka);
        pkt_out_t oc{};
        void** ocp = reinterpret_cast<void**>(&oc);
#pragma unroll
        for (int c = LO; c < HI; c++) {
            const void* q = kc[c - LO];
            if constexpr (LATE == L_MULTI) q = q ? reinterpret_cast<const uint8_t*>(q) + delta : q;
            ocp[c] = as_global(const_cast<void*>(q));
        }
        constexpr uint32_t GG = rt ? GM : (G | (GM & G_NT));
        if constexpr (G == G_CHAIN) emit_chain<GG>(oc, i, len, r);
        else emit_fields<GG>(oc, i, pv, r, r.status == PKT_OK);
    }
}

template <int NCH, uint32_t GM, int WK, bool STAGED, int LATE>
__device__ __forceinline__ void parse_tile(const KParams& p, uint8_t* lds, uint32_t base,
                                           const u32x4 (&chunk)[NCH], uint64_t off_own, uint32_t len_own,
                                           bool active_own, uint64_t* pkt_st, const DispatchLds* T, uint32_t mb) {
    (void)pkt_st;
    (void)mb;
    const uint32_t t = threadIdx.x;
    const uint32_t i_own = base + t;
    // Register fast path (pkt_ctx_set_fastpath): an aligned packet whose EtherType chain is
    // 0x0800, 0x8100 0x0800 or 0x8100 0x8100 0x0800 (bytes 12, 16, 20: v = 0..2 VLAN tags), whose
    // IPv4 protocol (byte 23 + 4v) is 17 with a UDP dst port (bytes 36 + 4v) != 4789 and
    // len >= 42 + 4v, or 6 with len >= 54 + 4v, takes exactly fast.rs's Ether -> Vlan{v} -> IPv4 ->
    // UDP|TCP -> accept path (no bound or depth check can fail on it), so a few compares on the
    // loaded registers decide its whole chain: it skips the walk.
    bool fast = false, fudp = false;
    uint32_t fv = 0;
    if constexpr (NCH >= 4) {
        if (p.fast && active_own && (off_own & 15) == 0) {
            // dwords 3..11 of the packet (little-endian), from the registers or, when the wave
            // loaded its windows cooperatively, from the lane's own LDS window
            uint32_t d3, d4, d5, d6, d7, d9, d10, d11;
            if constexpr (STAGED) {
                const uint32_t* w = reinterpret_cast<const uint32_t*>(lds + t * lane_stride(NCH));
                d3 = w[3], d4 = w[4], d5 = w[5], d6 = w[6], d7 = w[7], d9 = w[9], d10 = w[10], d11 = w[11];
            } else {
                d3 = chunk[0].w, d4 = chunk[1].x, d5 = chunk[1].y, d6 = chunk[1].z, d7 = chunk[1].w;
                d9 = chunk[2].y, d10 = chunk[2].z, d11 = chunk[2].w;
            }
            const uint32_t e0 = d3 & 0xFFFFu, e1 = d4 & 0xFFFFu, e2 = d5 & 0xFFFFu;
            const bool v0 = e0 == 0x0008u;                    // little-endian 0x0800
            const bool v1 = e0 == 0x0081u && e1 == 0x0008u;   // 0x8100, 0x0800
            const bool v2 = e0 == 0x0081u && e1 == 0x0081u && e2 == 0x0008u;
            fv = v1 ? 1u : (v2 ? 2u : 0u);
            const uint32_t proto = (v0 ? d5 : v1 ? d6 : d7) >> 24;
            const uint32_t dport = (v0 ? d9 : v1 ? d10 : d11) & 0xFFFFu;
            const uint32_t l4 = 34u + 4u * fv;
            fudp = proto == 17u;
            fast = (v0 || v1 || v2) && ((fudp && len_own >= l4 + 8u && dport != 0xB512u) ||
                                        (proto == 6u && len_own >= l4 + 20u));
        }
    }
    // Fast lanes skip the walk; all lanes stage their window and emit from LDS together (one
    // store per column per wave).  (Decoding all-fast waves from registers instead: shorter
    // isolated launches, slower pipelined steps)
    const pkt_out_t& out = p.out;
    const uint64_t ns = p.n_slot_stride;
    auto push = [&](uint32_t slot, uint32_t ty, uint32_t o) { push_slot<GM>(out, ns, slot, i_own, ty, o); };
    // fast.rs:5-12 (>= 1500) -> parse_ethernet 35-48 (0x8100 -> parse_vlan 49-62, repeated;
    // 0x0800) -> parse_ipv4 84-98 (17 / 6) -> parse_udp 208-217 (dst != 4789) | parse_tcp 203-207
    // -> accept 223-227
    auto fast_result = [&](WalkResult& r, uint32_t v) {
        const uint32_t l4 = 34u + 4u * v;
        r.status = PKT_OK;
        r.n = 3 + v;
        r.payload_off = l4 + (fudp ? 8u : 20u);
        r.mask = (1u << PKT_HDR_ETHER) | (1u << PKT_HDR_IPV4) | (fudp ? 1u << PKT_HDR_UDP : 1u << PKT_HDR_TCP) |
                 (v ? 1u << PKT_HDR_VLAN : 0u);
        r.f_eth = 0;
        r.f_vlan = v ? 14 : -1;
        r.f_ipv4 = (int32_t)(14u + 4u * v);
        r.f_ipv6 = -1;
        r.f_tcp = fudp ? -1 : (int32_t)l4;
        r.f_udp = fudp ? (int32_t)l4 : -1;
        push(0, PKT_HDR_ETHER, 0);
        if (v >= 1) push(1, PKT_HDR_VLAN, 14);
        if (v >= 2) push(2, PKT_HDR_VLAN, 18);
        push(1 + v, PKT_HDR_IPV4, 14u + 4u * v);
        push(2 + v, fudp ? PKT_HDR_UDP : PKT_HDR_TCP, l4);
    };
    if constexpr (!STAGED) stage_window<NCH>(lds, t, chunk);
    PacketView pv_own = make_view(p, lds, t, off_own, len_own, NCH);

    // each lane walks and emits its own packet (no barrier: own LDS only)
    __builtin_amdgcn_wave_barrier();
    WalkResult r;
    walk<WK>(pv_own, entry_state(p.entry), active_own && !fast, push, r, T);
    if constexpr (NCH >= 4) {
        if (fast) fast_result(r, fv);
    }
    PKT_STAMP(2);
    if (p.nh_max) {  // wave-uniform: the used slot rows of the batch, for a gather of its chain
        const uint32_t m = wave_max_u32((active_own && r.status == PKT_OK) ? r.n : 0u);
        if ((t & 63u) == 0 && m) atomicMax(p.nh_max + (blockIdx.x & (kMaxSpread - 1)), m);
    }
    if (active_own) {
        if constexpr (LATE != L_EARLY) {
            // The column bases are loaded here, after the walk, by scalar loads from the kernel
            // arguments (an opaque copy of their address keeps the loads from being hoisted to the
            // kernel start), and re-marked as global pointers so every store stays a global store.
            // Loaded at the start instead, the 49 bases of the all-columns kernel held 106 SGPRs
            // through the walk and spilled 48 to VGPR lanes (~96 lane instructions per wave); round
            // 3's late load through a generic pointer made every column access a flat access, 6x
            // slower (profiles/ab/r03j_late_column_pointers.txt).
            // (parse_kernel's only argument is the KParams, parse_multi_kernel's the MultiParams
            // whose first member is batch 0's KParams: either starts the kernarg segment)
            const uint64_t kseg = reinterpret_cast<uint64_t>(__builtin_amdgcn_kernarg_segment_ptr());
            uint64_t ka = kseg + offsetof(KParams, out);
            asm volatile("" : "+s"(ka));
            const void* const KARG_AS* kc = reinterpret_cast<const void* const KARG_AS*>(ka);
            int64_t delta = 0;
            if constexpr (LATE == L_MULTI) {
                // (mb is wave-uniform, but the integer division that made it leaves it in a VGPR)
                const uint32_t mbs = __builtin_amdgcn_readfirstlane(mb);
                uint64_t kd = kseg + offsetof(MultiParams, per) + (uint64_t)mbs * sizeof(MultiBatch) +
                              offsetof(MultiBatch, out_delta);
                asm volatile("" : "+s"(kd));
                delta = *reinterpret_cast<const int64_t KARG_AS*>(kd);
            }
            (void)kc;
            // column ranges of the groups in pkt_out_t order (group_masks)
            emit_group_late<GM, G_CHAIN, 0, 7, LATE>(kseg, delta, i_own, len_own, pv_own, r);
            emit_group_late<GM, G_ETHER, 7, 10, LATE>(kseg, delta, i_own, len_own, pv_own, r);
            emit_group_late<GM, G_VLAN, 10, 14, LATE>(kseg, delta, i_own, len_own, pv_own, r);
            emit_group_late<GM, G_IPV4, 14, 27, LATE>(kseg, delta, i_own, len_own, pv_own, r);
            emit_group_late<GM, G_IPV6, 27, 35, LATE>(kseg, delta, i_own, len_own, pv_own, r);
            emit_group_late<GM, G_TCP, 35, 45, LATE>(kseg, delta, i_own, len_own, pv_own, r);
            emit_group_late<GM, G_UDP, 45, kNumCols, LATE>(kseg, delta, i_own, len_own, pv_own, r);
        } else {
            emit_chain<GM>(out, i_own, len_own, r);
            emit_fields<GM>(out, i_own, pv_own, r, r.status == PKT_OK);
        }
    }
#if PKTGPU_STAMPS
    PKT_STAMP(3);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    PKT_STAMP(4);
    if ((t & 63u) == 0 && g_pkt_stamps) {
        uint32_t hw, xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        uint64_t* d = g_pkt_stamps + ((uint64_t)blockIdx.x * kWavesPerBlock + (t >> 6)) * 8u;
        for (int k = 0; k < 5; k++) d[k] = pkt_st[k];
        d[5] = hw;
        d[6] = xcc & 15u;  // s_memtime counts per XCD: stamps compare within one XCD only
    }
#endif
}

// ---- span staging (indexed batches: the records of a pcap lie back to back) ----
// The 64 records of a wave usually occupy ONE contiguous byte range of the slab.  The wave copies
// that range [lo & ~15, hi) into its LDS region by LDS-DMA (global_load_lds_dwordx4: 1 KiB of
// consecutive bytes per wave-instruction, fully coalesced, no VGPRs) and every lane then walks its
// record entirely out of LDS: no per-lane window, no global-memory reads for deep tunnels, and
// each HBM line is fetched once.  A wave whose range exceeds the region (records far apart or
// long) stages per-lane windows into the same region instead (the parse_kernel staging).
#define LDS_AS __attribute__((address_space(3)))
#ifndef PKTGPU_SPAN_CAP
#define PKTGPU_SPAN_CAP 16384u  // bytes of range one wave stages (a multiple of 1024)
#endif
static_assert(PKTGPU_SPAN_CAP % 1024u == 0, "span cap: whole 1 KiB LDS-DMA pieces");
constexpr uint32_t kSpanBlock = 64;  // one wave per block: one LDS region per block
__host__ __device__ constexpr uint32_t span_region(int nch) {
    // the range, or the fallback's 64 packed windows; +16: the walk's dword over-read
    return ((PKTGPU_SPAN_CAP > 64u * lane_stride(nch) ? PKTGPU_SPAN_CAP : 64u * lane_stride(nch)) + 16u + 15u) & ~15u;
}

__device__ __forceinline__ uint64_t wave_uniform64(uint64_t v) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}

template <int NCH, uint32_t GM, int WK>
__global__ __launch_bounds__(kSpanBlock) void parse_span_kernel(KParams p) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const uint32_t lane = threadIdx.x;
    uint32_t n_eff = p.n, b0 = blockIdx.x * kSpanBlock;
    if (p.n_dev) {  // wave-uniform: the count the device produced (scalar load)
        const uint64_t nd = *p.n_dev;
        n_eff = nd < (uint64_t)n_eff ? (uint32_t)nd : n_eff;
        if (p.i0_dev) b0 += (uint32_t)*p.i0_dev;  // the launch starts at a device-produced index
        if (b0 >= n_eff) return;  // the whole wave (= block) is past the count
    }
    const DispatchLds* T = tables<WK>(lds, span_region(NCH), lane, kSpanBlock);
    const uint32_t i = b0 + lane;  // within this launch
    const bool active = i < n_eff;
    uint64_t off = 0;
    uint32_t len = 0;
    if (active) packet_range(p, i, off, len);
    // the wave's byte range [lo, hi) (butterfly min/max; lane 0 is active: blocks whose first packet
    // lies past the count have returned above)
    uint64_t lo = active ? off : ~(uint64_t)0, hi = active ? off + len : 0;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const uint64_t l2 = __shfl_xor(lo, m, 64), h2 = __shfl_xor(hi, m, 64);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
    }
    const uint64_t a0 = wave_uniform64(lo) & ~(uint64_t)15;
    const uint64_t hi_u = wave_uniform64(hi);
    const uint64_t bytes = hi_u > a0 ? hi_u - a0 : 0;
    const uint64_t last16 = ((p.slab_len + 15) & ~(uint64_t)15) - 16;
    PacketView pv;
    if (bytes <= PKTGPU_SPAN_CAP) {  // wave-uniform
        const uint32_t npiece = (uint32_t)((bytes + 1023) >> 10);
        for (uint32_t k = 0; k < npiece; k++) {
            uint64_t o = a0 + ((uint64_t)k << 10) + lane * 16u;
            o = o > last16 ? last16 : o;  // bytes past the slab end lie beyond every record
            __builtin_amdgcn_global_load_lds(reinterpret_cast<const void*>(p.slab + o),
                                             (LDS_AS void*)(lds + (k << 10)), 16, 0, 0);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t rel = active ? (uint32_t)(off - a0) : 0u;
        pv.lw = lds + (rel & ~3u);
        pv.slab = p.slab;
        pv.off = off;
        pv.last4 = ((p.slab_len + 15) & ~(uint64_t)15) - 4;
        pv.shift = rel & 3u;
        pv.win_lo = 0;
        pv.win_end = (npiece << 10) - rel;  // >= len: the whole record is in LDS
        pv.len = len;
    } else {
        u32x4 chunk[NCH];
        const uint64_t c0 = off & ~(uint64_t)15;
#pragma unroll
        for (int c = 0; c < NCH; c++) {
            uint64_t o = c0 + 16u * (uint32_t)c;
            o = o > last16 ? last16 : o;
            chunk[c] = *reinterpret_cast<const u32x4*>(p.slab + o);
        }
        stage_window<NCH>(lds, lane, chunk);
        pv = make_view(p, lds, lane, off, len, NCH);
    }
    const pkt_out_t& out = p.out;
    const uint64_t ns = p.n_slot_stride;
    auto push = [&](uint32_t slot, uint32_t ty, uint32_t o) { push_slot<GM>(out, ns, slot, i, ty, o); };
    WalkResult r;
    walk<WK>(pv, entry_state(p.entry), active, push, r, T);
    if (p.nh_max) {
        const uint32_t m = wave_max_u32((active && r.status == PKT_OK) ? r.n : 0u);
        if (lane == 0 && m) atomicMax(p.nh_max + (blockIdx.x & (kMaxSpread - 1)), m);
    }
    if (!active) return;
    // the column bases group by group, loaded after the walk (parse_kernel's late loads: the kernel's
    // only argument is the KParams, so the kernarg segment starts with it)
    const uint64_t kseg = reinterpret_cast<uint64_t>(__builtin_amdgcn_kernarg_segment_ptr());
    emit_group_late<GM, G_CHAIN, 0, 7, L_SINGLE>(kseg, 0, i, len, pv, r);
    emit_group_late<GM, G_ETHER, 7, 10, L_SINGLE>(kseg, 0, i, len, pv, r);
    emit_group_late<GM, G_VLAN, 10, 14, L_SINGLE>(kseg, 0, i, len, pv, r);
    emit_group_late<GM, G_IPV4, 14, 27, L_SINGLE>(kseg, 0, i, len, pv, r);
    emit_group_late<GM, G_IPV6, 27, 35, L_SINGLE>(kseg, 0, i, len, pv, r);
    emit_group_late<GM, G_TCP, 35, 45, L_SINGLE>(kseg, 0, i, len, pv, r);
    emit_group_late<GM, G_UDP, 45, kNumCols, L_SINGLE>(kseg, 0, i, len, pv, r);
}

// How a launch stages packet bytes: per-lane windows (one tile per block) or wave spans.
// (Round 3's pipelined windows — persistent waves loading the next tile's windows into VGPRs while
// walking the current one — were slower on every measured batch, C4 96.7 vs 89.9 us isolated,
// profiles/ab/r03b_c4_staging3_pipelined_windows.txt, and correct only while every instantiation
// stayed spill-free; removed in round 4.)
enum LaunchMode { M_TILE = 0, M_SPAN = 2 };

template <int NCH, uint32_t GM, int WK>
hipError_t launch_mode(const KParams& kp, int mode, hipStream_t s, const MultiParams* mp, uint32_t gn) {
    if (mp) {  // several batches, one launch (windows only)
        hipLaunchKernelGGL((parse_multi_kernel<NCH, GM, WK>), dim3(mp->bpb * mp->k), dim3(kBlock),
                           with_tables(window_lds(NCH), WK), s, *mp);
        return hipGetLastError();
    }
    if (mode == M_SPAN) {
        hipLaunchKernelGGL((parse_span_kernel<NCH, GM, WK>), dim3((unsigned)((gn + kSpanBlock - 1) / kSpanBlock)),
                           dim3(kSpanBlock), with_tables(span_region(NCH), WK), s, kp);
    } else {
        const size_t lds = with_tables(window_lds(NCH), WK);
        hipLaunchKernelGGL((parse_kernel<NCH, GM, WK>), dim3((unsigned)((gn + kBlock - 1) / kBlock)), dim3(kBlock),
                           lds, s, kp);
    }
    return hipGetLastError();
}

// Kernels are compiled per fully-requested column-group set; the lockstep walk (mixed traffic)
// only for the chain-only, all-columns and per-column-check sets.
template <int NCH>
hipError_t launch_gm(const KParams& kp, uint32_t gm, int mode, int wk, hipStream_t s, const MultiParams* mp,
                     uint32_t gn) {
    // lockstep (indexed batches; non-temporal column stores): compiled for the windows of 6, 7, 9
    // and 17 chunks only (window requests of <= 80, 96, 128 and 256 B; parse_impl widens the rest)
    if constexpr (NCH >= 6) if (wk == 1) {
        switch (gm) {
            case G_CHAIN: return launch_mode<NCH, G_CHAIN | G_NT, 1>(kp, mode, s, mp, gn);
            case G_ALL: return launch_mode<NCH, G_ALL | G_NT, 1>(kp, mode, s, mp, gn);
            default: return launch_mode<NCH, G_RUNTIME | G_NT, 1>(kp, mode, s, mp, gn);
        }
    }
    switch (gm) {
        case G_CHAIN: return launch_mode<NCH, G_CHAIN, 0>(kp, mode, s, mp, gn);
        case G_CHAIN | G_ETHER | G_IPV4 | G_UDP: return launch_mode<NCH, G_CHAIN | G_ETHER | G_IPV4 | G_UDP, 0>(kp, mode, s, mp, gn);
        case G_CHAIN | G_ETHER | G_VLAN | G_IPV4 | G_TCP | G_UDP:
            return launch_mode<NCH, G_CHAIN | G_ETHER | G_VLAN | G_IPV4 | G_TCP | G_UDP, 0>(kp, mode, s, mp, gn);
        case G_ALL: return launch_mode<NCH, G_ALL, 0>(kp, mode, s, mp, gn);
        default: return launch_mode<NCH, G_RUNTIME, 0>(kp, mode, s, mp, gn);
    }
}

// Which groups are fully requested (all columns non-NULL) and which partly.
void group_masks(const pkt_out_t& o, uint32_t& full, uint32_t& any) {
    const void* const* cols = reinterpret_cast<const void* const*>(&o);
    // column ranges of each group in pkt_out_t order (see include/pktgpu.h)
    static const struct { uint32_t g; int lo, hi; } R[] = {
        {G_CHAIN, 0, 7}, {G_ETHER, 7, 10}, {G_VLAN, 10, 14}, {G_IPV4, 14, 27},
        {G_IPV6, 27, 35}, {G_TCP, 35, 45}, {G_UDP, 45, kNumCols}};
    full = any = 0;
    for (const auto& g : R) {
        bool all = true, some = false;
        for (int c = g.lo; c < g.hi; c++) {
            all &= cols[c] != nullptr;
            some |= cols[c] != nullptr;
        }
        if (all) full |= g.g;
        if (some) any |= g.g;
    }
}

template <class T>
T* adv(T* p, uint64_t k) { return p ? p + k : p; }

// The largest n_hdrs of a batch: how many slot rows of hdr_type / hdr_off hold data.  16 bytes per
// thread (grid-strided), a wave max, one atomicMax per wave that saw a non-zero count.
__global__ __launch_bounds__(256) void max_hdrs_kernel(const uint8_t* nh, uint64_t n, uint32_t* out) {
    uint32_t m = 0;
    const uint64_t step = (uint64_t)gridDim.x * 256u * 16u;
    const bool al = ((uintptr_t)nh & 15) == 0;
    for (uint64_t i = ((uint64_t)blockIdx.x * 256u + threadIdx.x) * 16u; i < n; i += step) {
        if (al && i + 16 <= n) {
            const uint4 v = *reinterpret_cast<const uint4*>(nh + i);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 4; k++)
                m = max(max(m, w[k] >> 24), max(max(w[k] & 0xFFu, (w[k] >> 8) & 0xFFu), (w[k] >> 16) & 0xFFu));
        } else {
            for (uint64_t k = i; k < i + 16 && k < n; k++) m = max(m, (uint32_t)nh[k]);
        }
    }
#pragma unroll
    for (int sft = 32; sft >= 1; sft >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, sft, 64));
    if ((threadIdx.x & 63) == 0 && m) atomicMax(out + (blockIdx.x & (kMaxSpread - 1)), m);
}

// Queue the reduction of n_hdrs[0, n) into scratch word `w` and its copy to the host mirror on `s`.
hipError_t max_hdrs_async(pkt_ctx* ctx, const uint8_t* nh, uint64_t n, int w, hipStream_t s) {
    hipError_t e = hipMemsetAsync(ctx->mx.dgroup(w), 0, MaxScratch::kSpread * sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    if (n) {
        const unsigned grid = (unsigned)std::min<uint64_t>((n + 4095) / 4096, 1024);
        hipLaunchKernelGGL(max_hdrs_kernel, dim3(grid), dim3(256), 0, s, nh, n, ctx->mx.dgroup(w));
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipMemcpyAsync(ctx->mx.hgroup(w), ctx->mx.dgroup(w), MaxScratch::kSpread * sizeof(uint32_t),
                          hipMemcpyDeviceToHost, s);
}

// Validate and launch one parse (ParseOpts, pktgpu_ctx.hpp).  mp (pkt_parse_batches only): the batches of
// one multi-batch launch, `b` / `out` being batch 0's; the launch fills mp->base.
int parse_impl(pkt_ctx_t* ctx, const pkt_batch_t* b, int entry, const pkt_out_t* out, void* stream,
               const ParseOpts& po, MultiParams* mp = nullptr) {
    if (!ctx || !b || !out) return fail(ctx, PKT_ERR_INVALID_ARG, "null argument");
    if (entry < 0 || entry >= PKT_ENTRY_COUNT) return fail(ctx, PKT_ERR_INVALID_ARG, "bad entry");
    if (b->n == 0) return PKT_SUCCESS;
    if (!b->slab) return fail(ctx, PKT_ERR_INVALID_ARG, "null slab");
    int rc = check_batch_slab16(ctx, b);
    if (rc == PKT_SUCCESS) rc = check_batch_index(ctx, b);
    if (rc != PKT_SUCCESS) return rc;
    if (out->ipv6_src && ((uintptr_t)out->ipv6_src & 15)) return fail(ctx, PKT_ERR_INVALID_ARG, "ipv6_src not 16-byte aligned");
    if (out->ipv6_dst && ((uintptr_t)out->ipv6_dst & 15)) return fail(ctx, PKT_ERR_INVALID_ARG, "ipv6_dst not 16-byte aligned");
    if (b->slab_len == 0) return fail(ctx, PKT_ERR_INVALID_ARG, "slab_len 0");
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");

    // Window: bytes of each packet staged in LDS.  Fixed stride: the slot (up to 128 B);
    // indexed: 128 B.  Unaligned packet starts need one more chunk.
    uint32_t w = ctx->window;
    // Auto window: the stride up to 64 bytes for fixed-stride slabs (Ether[/Vlan x2]/IPv4/TCP ends at
    // byte 62); 80 bytes for indexed batches (96 from the record's 16-byte-aligned start: every
    // header of 16 of the 22 reference templates, the rest read past it through L2).  C4 per 2^20
    // records, same box, 2 streams: 80 B 46.6 (chain) / 68.1 us (all columns), 64 B 49.4 / 75.8,
    // 96 B 49.6 / 69.1, 128 B 59.7 / 77.4 — wider windows read fewer lines twice but hold fewer
    // waves per CU (LDS), round 3.  (Round 4: windows packed from the record's first
    // byte — 80 or 96 packet bytes in 84 or 100 B of LDS per record, 7 or 6 blocks per CU — were
    // slower than this layout in every combination: C4 all columns 72.6-74.1 vs 69.9 us, chain
    // 52.6-57.7 vs 50.4 us per 2-stream step; the unaligned LDS stores of the staging cost more than
    // the occupancy or the lines they save, profiles/ab/r04c_c4_packed_windows.txt.)
    if (w == 0) w = b->offsets ? 80u : std::min<uint32_t>(std::max<uint32_t>(b->stride, 16u), 64u);
    w = std::min<uint32_t>(std::max<uint32_t>((w + 15) & ~15u, 16u), 256u);
    bool aligned = !b->offsets && (b->stride % 16 == 0);
    int nch = (int)(w / 16) + (aligned ? 0 : 1);

    uint32_t full, any;
    group_masks(*out, full, any);
    const uint32_t gm = (full == any) ? full : G_RUNTIME;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    // Staging: wave spans when asked; per-lane windows otherwise (auto: spans measured slower on
    // device-resident C3 and C4).
    const int mode = (po.staging ? po.staging : ctx->staging) == 2 ? M_SPAN : M_TILE;
    // Walk: lockstep for indexed batches (pcap replays mix chains within a wave), waterfall for
    // fixed-stride slabs (one layout per wave), unless the ctx says otherwise.
    const int wk = ctx->walk == 2 ? 1 : ctx->walk == 1 ? 0 : (b->offsets ? 1 : 0);
    if (wk == 1 && nch < 6) nch = 6;  // the narrowest lockstep build
    for (uint64_t i0 = 0; i0 < b->n && e == hipSuccess; i0 += kLaunchChunk) {
        const uint64_t cnt = std::min<uint64_t>(kLaunchChunk, b->n - i0);
        KParams kp;
        kp.slab = b->slab;
        kp.slab_len = b->slab_len;
        kp.offsets = adv(b->offsets, i0);
        kp.lens = adv(b->lens, i0);
        kp.off_bias = po.off_bias;
        kp.i0 = i0;
        kp.n_slot_stride = po.slot_stride ? po.slot_stride : b->n;  // the slot columns' row stride
        kp.stride = b->stride;
        kp.n = (uint32_t)cnt;
        kp.entry = entry;
        kp.fast = ctx->fast && (entry == PKT_ENTRY_PARSE || entry == PKT_ENTRY_ETHERNET);
        kp.nh_max = po.nh_max;
        kp.n_dev = po.n_dev;  // (one launch: n_dev is only passed for batches of n <= kLaunchChunk)
        kp.i0_dev = po.n_dev ? po.i0_dev : nullptr;
        pkt_out_t o = *out;
        uint8_t** oc = reinterpret_cast<uint8_t**>(&o);
        for (int c = 0; c < kNumCols; c++)
            if (oc[c]) oc[c] += i0 * kColSize[c];
        kp.out = o;
        if (mp) mp->base = kp;  // batch 0 of a multi-batch launch (n <= kLaunchChunk: one chunk)
        // the launch's grid: kp.n packets, or grid_n when the range starts at a device-produced index
        const uint32_t gn = (kp.n_dev && po.grid_n) ? (uint32_t)std::min<uint64_t>(po.grid_n, cnt) : kp.n;
        const int md = mp ? M_TILE : mode;
        // compiled window widths (chunks): a request between two is served by the wider one
        if (nch <= 2) e = launch_gm<2>(kp, gm, md, wk, s, mp, gn);
        else if (nch <= 4) e = launch_gm<4>(kp, gm, md, wk, s, mp, gn);
        else if (nch <= 5) e = launch_gm<5>(kp, gm, md, wk, s, mp, gn);
        else if (nch <= 6) e = launch_gm<6>(kp, gm, md, wk, s, mp, gn);
        else if (nch <= 7 && wk == 1) e = launch_gm<7>(kp, gm, md, wk, s, mp, gn);
        else if (nch <= 9) e = launch_gm<9>(kp, gm, md, wk, s, mp, gn);
        else e = launch_gm<17>(kp, gm, md, wk, s, mp, gn);
    }
    if (e != hipSuccess) return hip_fail(ctx, e, "parse_kernel launch");
    return PKT_SUCCESS;
}

}  // namespace

// ---- the internal entry points (pktgpu_ctx.hpp) ----
int pktgpu_parse(pkt_ctx_t* ctx, const pkt_batch_t* b, int entry, const pkt_out_t* out, void* stream,
                 const ParseOpts& opts) {
    return parse_impl(ctx, b, entry, out, stream, opts);
}

hipError_t pktgpu_ensure_max_scratch(pkt_ctx_t* ctx) {
    if (ctx->mx.dev) return hipSuccess;
    static_assert(MaxScratch::kSpread == (int)kMaxSpread, "one spread");
    constexpr size_t bytes = MaxScratch::kGroups * MaxScratch::kSpread * sizeof(uint32_t);
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&ctx->mx.dev), bytes);
    if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void**>(&ctx->mx.host), bytes, hipHostMallocDefault);
    if (e != hipSuccess) {
        (void)hipFree(ctx->mx.dev);
        ctx->mx.dev = nullptr;
        ctx->mx.host = nullptr;
    }
    return e;
}

int pktgpu_parse_counted(pkt_ctx_t* ctx, const pkt_batch_t* b, int entry, const pkt_out_t* out, void* stream,
                         const uint64_t* count_dev, uint64_t slot_stride) {
    if (b && b->n && b->slab_len < 16) return fail(ctx, PKT_ERR_INVALID_ARG, "slab_len < 16");
    if (count_dev && b && b->n > kLaunchChunk) return fail(ctx, PKT_ERR_INVALID_ARG, "device count over 2^26 packets");
    ParseOpts po;
    po.slot_stride = slot_stride;
    po.n_dev = count_dev;
    return parse_impl(ctx, b, entry, out, stream, po);
}

// (the reduction: a wave max + one atomicMax per wave, fused into the parse kernel)
int pktgpu_parse_rows_async(pkt_ctx_t* ctx, const pkt_batch_t* b, int entry, const pkt_out_t* out, void* stream,
                            const uint32_t** rows_host) {
    if (!ctx || !rows_host) return fail(ctx, PKT_ERR_INVALID_ARG, "null argument");
    if (b && b->n && b->slab_len < 16) return fail(ctx, PKT_ERR_INVALID_ARG, "slab_len < 16");
    hipError_t e = hipSetDevice(ctx->device);
    if (e == hipSuccess) e = pktgpu_ensure_max_scratch(ctx);
    if (e != hipSuccess) return hip_fail(ctx, e, "parse rows scratch");
    const int w = MaxScratch::kGroups - 1;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if ((e = hipMemsetAsync(ctx->mx.dgroup(w), 0, MaxScratch::kSpread * sizeof(uint32_t), s)) != hipSuccess)
        return hip_fail(ctx, e, "hipMemsetAsync");
    ParseOpts po;
    po.nh_max = ctx->mx.dgroup(w);
    const int rc = parse_impl(ctx, b, entry, out, stream, po);
    if (rc != PKT_SUCCESS) return rc;
    if ((e = hipMemcpyAsync(ctx->mx.hgroup(w), ctx->mx.dgroup(w), MaxScratch::kSpread * sizeof(uint32_t),
                            hipMemcpyDeviceToHost, s)) != hipSuccess)
        return hip_fail(ctx, e, "hipMemcpyAsync (rows)");
    *rows_host = ctx->mx.hgroup(w);
    return PKT_SUCCESS;
}

extern "C" {

#if PKTGPU_STAMPS
// Diagnostic build only: where the parse kernel writes its per-wave stamps (8 u64 per wave:
// 5 s_memtime stamps, HW_ID, batch size).  NULL = none.
int pkt_debug_stamps(void* dev_buf) {
    return hipMemcpyToSymbol(HIP_SYMBOL(g_pkt_stamps), &dev_buf, sizeof(dev_buf)) == hipSuccess ? PKT_SUCCESS
                                                                                           : PKT_ERR_HIP;
}
#endif

int pkt_chain_max_hdrs(pkt_ctx_t* ctx, const uint8_t* n_hdrs, uint64_t n, uint32_t* max_out, void* stream) {
    if (!ctx || !max_out || (n && !n_hdrs)) return fail(ctx, PKT_ERR_INVALID_ARG, "null argument");
    hipError_t e = hipSetDevice(ctx->device);
    if (e == hipSuccess) e = pktgpu_ensure_max_scratch(ctx);
    if (e != hipSuccess) return hip_fail(ctx, e, "pkt_chain_max_hdrs scratch");
    const int w = MaxScratch::kGroups - 1;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if ((e = max_hdrs_async(ctx, n_hdrs, n, w, s)) != hipSuccess) return hip_fail(ctx, e, "max_hdrs_kernel");
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return hip_fail(ctx, e, "hipStreamSynchronize");
    *max_out = std::min<uint32_t>(ctx->mx.host_max(w), PKT_MAX_HDRS);
    return PKT_SUCCESS;
}

int pkt_parse_batch(pkt_ctx_t* ctx, const pkt_batch_t* b, int entry, const pkt_out_t* out, void* stream) {
    // the kernel reads whole 16-byte chunks, clamped to the last one of the slab
    if (b && b->n && b->slab_len < 16) return fail(ctx, PKT_ERR_INVALID_ARG, "slab_len < 16");
    return parse_impl(ctx, b, entry, out, stream, ParseOpts{});
}

int pkt_parse_batches(pkt_ctx_t* ctx, const pkt_batch_t* batches, uint32_t nbatch, int entry, const pkt_out_t* outs,
                      void* stream) {
    if (!ctx || (nbatch && (!batches || !outs))) return fail(ctx, PKT_ERR_INVALID_ARG, "null argument");
    // One launch when the batches share size and layout and their outputs sit at one common byte
    // distance from batch 0's (per column); otherwise one pkt_parse_batch each (same results).
    bool one = nbatch >= 2 && nbatch <= (uint32_t)kMaxMulti && ctx->staging != 2;
    const pkt_batch_t& b0 = batches[0];
    const void* const* c0 = nbatch ? reinterpret_cast<const void* const*>(&outs[0]) : nullptr;
    MultiParams mp;
    for (uint32_t k = 0; k < nbatch && one; k++) {
        const pkt_batch_t& b = batches[k];
        one = b.n == b0.n && b.n > 0 && b.n <= kLaunchChunk && b.stride == b0.stride &&
              (b.offsets == nullptr) == (b0.offsets == nullptr) && (b.lens == nullptr) == (b0.lens == nullptr) &&
              b.slab && ((uintptr_t)b.slab & 15) == 0 && b.slab_len >= 16;
        const void* const* ck = reinterpret_cast<const void* const*>(&outs[k]);
        int64_t delta = 0;
        bool have = false;
        for (int c = 0; c < kNumCols && one; c++) {
            if ((ck[c] == nullptr) != (c0[c] == nullptr)) one = false;
            if (!ck[c]) continue;
            const int64_t d = (int64_t)((uintptr_t)ck[c] - (uintptr_t)c0[c]);
            if (have && d != delta) one = false;
            delta = d;
            have = true;
        }
        // batch k's IPv6 address columns are batch 0's + delta: the 16-byte alignment parse_impl
        // checks for batch 0 holds for every batch only if delta keeps it (else one call per batch,
        // each validated)
        if ((c0[kColIpv6Src] || c0[kColIpv6Dst]) && (delta & 15) != 0) one = false;
        if (one) mp.per[k] = MultiBatch{b.slab, b.slab_len, b.offsets, b.lens, delta};
    }
    if (!one) {
        for (uint32_t k = 0; k < nbatch; k++) {
            const int rc = pkt_parse_batch(ctx, &batches[k], entry, &outs[k], stream);
            if (rc != PKT_SUCCESS) return rc;
        }
        return PKT_SUCCESS;
    }
    mp.k = nbatch;
    mp.bpb = (uint32_t)((b0.n + kBlock - 1) / kBlock);
    return parse_impl(ctx, &b0, entry, &outs[0], stream, ParseOpts{}, &mp);
}

}  // extern "C"
