// pktgpu_fwd.hpp — what the two halves of pkt_fwd_* share: the per-packet decision (the search for the IP and the
// Ether entry, the status each step gives), the checksum arithmetic, the padded adjacency entry and the argument
// validation.  pktgpu_fwd.hip holds pkt_fwd_create / _destroy / _batch and the kernel; pktgpu_host.cpp holds
// pkt_fwd_host's sequential loop (it compiles under g++ alone).  Both call the same inline code, the way
// pktgpu_lpm.hpp shares the lpm walk, so the CPU tests cover the whole decision.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>

#include "pktgpu_batch.hpp"
#include "pktgpu_lpm.hpp"

static_assert(sizeof(pkt_fwd_adj_t) == 20, "fwd ABI struct");

constexpr uint32_t kFwdFlags = PKT_FWD_KEEP_L2 | PKT_FWD_NO_WRITE;
constexpr uint32_t kFwdNoEther = 0xFFFFFFFFu;  // FwdFind::eth when no Ether entry precedes the IP entry

// An adjacency as the lookups read it: 32 bytes, two aligned 16-byte loads.  w[0..2] = dmac | smac as they lie in
// the packet (little-endian dwords of the 12 bytes), w[3] = port; w[4] = mtu | action << 16, w[5..7] = 0.
struct alignas(16) FwdAdj {
    uint32_t w[8];
};

inline FwdAdj fwd_pack(const pkt_fwd_adj_t& a) {
    FwdAdj o{};
    uint8_t mac[12];
    memcpy(mac, a.dmac, 6);
    memcpy(mac + 6, a.smac, 6);
    for (uint32_t k = 0; k < 12; k++) o.w[k >> 2] |= (uint32_t)mac[k] << (8u * (k & 3u));
    o.w[3] = a.port;
    o.w[4] = (uint32_t)a.mtu | (uint32_t)a.action << 16;
    return o;
}

// ---- steps 2 and 3: the IP entry (pkt_flow_key_batch's search) and the Ether entry with the greatest index below it.
// The caller feeds the list's entries in order (fwd_find_step ignores an entry that is neither IP nor Ether, so
// its offset need not be read).
struct FwdFind {
    uint32_t ipt = 0, ipo = 0;     // the chosen IP entry's type (0: none) and offset
    uint32_t eth = kFwdNoEther;    // the offset of the last Ether entry before it
    uint32_t cur = kFwdNoEther;    // the last Ether entry so far
    uint32_t seen = 0;             // IP entries so far
};

PKT_HD bool fwd_is_ip(uint32_t t) { return t == PKT_HDR_IPV4 || t == PKT_HDR_IPV6; }
PKT_HD bool fwd_wants(uint32_t t) { return fwd_is_ip(t) || t == PKT_HDR_ETHER; }

PKT_HD void fwd_find_step(FwdFind& f, uint32_t which, uint32_t ty, uint32_t of) {
    const bool ip = fwd_is_ip(ty);
    const bool take = ip && (which == PKT_FLOW_LAST || f.seen == which);
    f.ipt = take ? ty : f.ipt;
    f.ipo = take ? of : f.ipo;
    f.eth = take ? f.cur : f.eth;
    f.seen += ip ? 1u : 0u;
    f.cur = ty == PKT_HDR_ETHER ? of : f.cur;
}

// the status steps 2 and 3 give (PKT_FWD_OK: both headers lie inside the packet's `len` bytes)
PKT_HD uint32_t fwd_find_status(const FwdFind& f, uint32_t len, bool keep_l2) {
    if (!f.ipt) return PKT_FWD_NO_IP;
    if (f.ipo + (f.ipt == PKT_HDR_IPV4 ? 20u : 40u) > len) return PKT_FWD_SPAN;
    if (keep_l2) return PKT_FWD_OK;
    if (f.eth == kFwdNoEther) return PKT_FWD_NO_ETHER;
    if (f.eth + 14u > len) return PKT_FWD_SPAN;
    return PKT_FWD_OK;
}

// ---- steps 4 to 7 from the IP header's first 12 bytes, h[k] = bytes 4k .. 4k + 3 as a little-endian dword
struct FwdIp {
    uint32_t t;      // ttl / hop limit
    uint32_t l3len;  // IPv4 bytes 2..3, or 40 + IPv6 bytes 4..5
};

PKT_HD uint32_t fwd_be16(uint32_t lo_byte_first) { return (lo_byte_first & 0xFFu) << 8 | (lo_byte_first >> 8 & 0xFFu); }

PKT_HD FwdIp fwd_ip_fields(const uint32_t h[3], bool v4) {
    if (v4) return FwdIp{h[2] & 0xFFu, fwd_be16(h[0] >> 16)};
    return FwdIp{h[1] >> 24, 40u + fwd_be16(h[1])};
}

// steps 5 (from the adjacency's action on) to 7; w4 = FwdAdj::w[4]
PKT_HD uint32_t fwd_adj_status(uint32_t w4, uint32_t l3len) {
    const uint32_t action = w4 >> 16 & 0xFFu, mtu = w4 & 0xFFFFu;
    if (action == PKT_FWD_ACT_DROP) return PKT_FWD_DROP;
    if (action == PKT_FWD_ACT_PUNT) return PKT_FWD_PUNT;
    if (mtu && l3len > mtu) return PKT_FWD_MTU;
    return PKT_FWD_OK;
}

// RFC 1624 eq. 3 for the ttl's decrement: hc = the stored checksum, m = IPv4 bytes 8..9 (ttl, protocol), both as
// big-endian words.  Not Packet::ipv4_checksum: nothing is summed again, so a wrong checksum stays wrong by as much.
PKT_HD uint32_t fwd_csum_update(uint32_t hc, uint32_t m) {
    const uint32_t m2 = (m - 0x0100u) & 0xFFFFu;
    uint32_t s = (~hc & 0xFFFFu) + (~m & 0xFFFFu) + m2;
    s = (s & 0xFFFFu) + (s >> 16);
    s = (s & 0xFFFFu) + (s >> 16);
    return ~s & 0xFFFFu;
}

// IPv4 bytes 8..11 after the rewrite, as the little-endian dword h[2] holds them: ttl - 1, protocol, HC'
PKT_HD uint32_t fwd_v4_word(uint32_t h2) {
    const uint32_t hc = fwd_csum_update(fwd_be16(h2 >> 16), fwd_be16(h2));
    return ((h2 & 0xFFu) - 1u) | (h2 & 0xFF00u) | (hc >> 8) << 16 | (hc & 0xFFu) << 24;
}

// ---- the refusals both entry points share: the text (after "pkt_fwd_create: " / "pkt_fwd_batch: " / ...), or nullptr
inline const char* fwd_adj_error(const pkt_fwd_adj_t* adj, uint32_t nadj) {
    if (nadj > PKT_FWD_MAX_ADJ) return "nadj above PKT_FWD_MAX_ADJ";
    if (nadj && !adj) return "null adj";
    for (uint32_t k = 0; k < nadj; k++) {
        if (adj[k].action > PKT_FWD_ACT_PUNT) return "an action above PKT_FWD_ACT_PUNT";
        if (adj[k].zero) return "non-zero `zero`";
    }
    return nullptr;
}

// device: pkt_fwd_batch (the slab's alignment rule, a device lpm handle on `device_id`); else pkt_fwd_host.
// n == 0 is the caller's to take after this returns nullptr and before the rules that hold for n > 0 alone
// (fwd_batch_error).
inline const char* fwd_call_error(const pkt_batch_t* b, const pkt_chain_t* chain, uint32_t which_ip, uint32_t flags,
                                  const pkt_lpm_t* lpm, const uint32_t* nexthop, const uint64_t* hits,
                                  const uint64_t* bytes, bool device, int device_id) {
    if (!b || !chain) return "null argument";
    if (b->n >= (1ull << 32)) return "n >= 2^32";
    if (flags & ~kFwdFlags) return "unknown flag bits";
    if (which_ip >= PKT_MAX_HDRS && which_ip != PKT_FLOW_LAST) return "which_ip is neither below 16 nor PKT_FLOW_LAST";
    if (lpm && nexthop) return "both lpm and nexthop";
    if (!lpm && !nexthop && b->n) return "neither lpm nor nexthop";
    if (lpm && device && !lpm->ops) return "lpm is a host handle";
    if (lpm && device && lpm->device != device_id) return "lpm was created on another device";
    if (lpm && !device && lpm->ops) return "lpm is a device handle";
    if (((uintptr_t)hits | (uintptr_t)bytes) & 7) return "hits / bytes not 8-byte aligned";
    return nullptr;
}

inline const char* fwd_batch_error(const pkt_batch_t* b, const pkt_chain_t* chain, bool device) {
    if (!chain->n_hdrs || !chain->hdr_type || !chain->hdr_off) return "null chain column";
    const char* msg = device ? batch_slab16_error(b) : batch_null_slab(b) ? "null slab" : nullptr;
    return msg ? msg : batch_index_error(b);
}
