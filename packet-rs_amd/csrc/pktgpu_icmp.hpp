// pktgpu_icmp.hpp — what the two halves of pkt_icmp_err_* share: the find step (pkt_frag_batch's IP entry plus
// pkt_fwd_batch's Ether entry, with their indices), the reason table, the per-packet decision of include/pktgpu.h
// step by step, the output's length, the two header builders with their RFC 1071 sums, and the argument validation.
// pktgpu_icmp.hip holds pkt_icmp_err_batch / _async / _result and the kernels; pktgpu_host.cpp holds
// pkt_icmp_err_host's sequential loops (it compiles under g++ alone).  Both call the same inline code, the
// pktgpu_frag.hpp pattern, so the CPU tests cover the whole decision and both headers.
#pragma once
#include <cstdint>

#include "pktgpu_batch.hpp"
#include "pktgpu_frag.hpp"
#include "pktgpu_outbatch.hpp"

static_assert(sizeof(pkt_icmp_cfg_t) == 28, "icmp ABI struct");

constexpr uint32_t kIcmpFlags = PKT_ICMPE_NO_WRITE;
constexpr uint32_t kIcmpNoEther = 0xFFFFFFFFu;

// The reasons' (type, code) pairs, the one table of include/pktgpu.h: type4 | code4 << 8 | type6 << 16 | code6 << 24
// (0 for a reason that asks for nothing).
PKT_HD uint32_t icmp_type_code(uint32_t r) {
    switch (r) {
        case PKT_ICMP_R_TIME_EXCEEDED: return 11u | 0u << 8 | 3u << 16 | 0u << 24;
        case PKT_ICMP_R_TOO_BIG: return 3u | 4u << 8 | 2u << 16 | 0u << 24;
        case PKT_ICMP_R_NET_UNREACH: return 3u | 0u << 8 | 1u << 16 | 0u << 24;
        case PKT_ICMP_R_HOST_UNREACH: return 3u | 1u << 8 | 1u << 16 | 3u << 24;
        case PKT_ICMP_R_PROHIBITED: return 3u | 13u << 8 | 1u << 16 | 1u << 24;
        case PKT_ICMP_R_PORT_UNREACH: return 3u | 3u << 8 | 1u << 16 | 4u << 24;
        default: return 0;
    }
}

PKT_HD uint32_t icmp_bswap32(uint32_t x) { return x << 24 | (x & 0xFF00u) << 8 | (x >> 8 & 0xFF00u) | x >> 24; }

// The cfg as the decision and the builders read it: the addresses as big-endian words (s6[0] = bytes 0..3), the
// defaults filled in.  The map travels with it: the kernel takes the whole struct by value.
struct IcmpCfg {
    uint32_t s4, s6[4];
    uint32_t max4, max6, ident, ttl, tos;
    uint32_t has_map;
    uint8_t map[256];
};

inline IcmpCfg icmp_cfg(const pkt_icmp_cfg_t& c, const uint8_t* map) {
    IcmpCfg o{};
    o.s4 = (uint32_t)c.src4[0] << 24 | (uint32_t)c.src4[1] << 16 | (uint32_t)c.src4[2] << 8 | c.src4[3];
    for (uint32_t k = 0; k < 4; k++)
        o.s6[k] = (uint32_t)c.src6[4 * k] << 24 | (uint32_t)c.src6[4 * k + 1] << 16 | (uint32_t)c.src6[4 * k + 2] << 8 |
                  c.src6[4 * k + 3];
    o.max4 = c.max4 ? c.max4 : 576u;
    o.max6 = c.max6 ? c.max6 : 1280u;
    o.ident = c.ident;
    o.ttl = c.ttl ? c.ttl : 64u;
    o.tos = c.tos;
    o.has_map = map ? 1u : 0u;
    if (map)
        for (uint32_t k = 0; k < 256; k++) o.map[k] = map[k];
    return o;
}

// steps 3 and 4's search: pkt_frag_batch's IP entry (frag_find_step) and the Ether entry with the greatest index below
// it (fwd_find_step's rule), each with its index.  The caller feeds the list's entries in order; an entry that is
// neither IP nor Ether is ignored, so its offset need not be read.
struct IcmpFind {
    uint32_t ipt = 0, ipo = 0, e_ip = 0;           // the chosen IP entry's type (0: none), offset and index
    uint32_t eth = kIcmpNoEther, e_eth = 0;        // the last Ether entry before it: offset and index
    uint32_t cur = kIcmpNoEther, e_cur = 0;        // the last Ether entry so far
    uint32_t seen = 0;                             // IP entries so far
};

PKT_HD void icmp_find_step(IcmpFind& f, uint32_t which, uint32_t j, uint32_t ty, uint32_t of) {
    const bool ip = fwd_is_ip(ty);
    const bool take = ip && (which == PKT_FLOW_LAST || f.seen == which);
    f.ipt = take ? ty : f.ipt;
    f.ipo = take ? of : f.ipo;
    f.e_ip = take ? j : f.e_ip;
    f.eth = take ? f.cur : f.eth;
    f.e_eth = take ? f.e_cur : f.e_eth;
    f.seen += ip ? 1u : 0u;
    const bool et = ty == PKT_HDR_ETHER;
    f.cur = et ? of : f.cur;
    f.e_cur = et ? j : f.e_cur;
}

// steps 3 and 4: PKT_ICMPE_NO_IP / _SPAN / _NO_ETHER, or PKT_ICMPE_SENT for "go on with icmp_decide"
PKT_HD uint32_t icmp_find_status(const IcmpFind& f, uint32_t len) {
    if (!f.ipt) return PKT_ICMPE_NO_IP;
    if (f.ipo + (f.ipt == PKT_HDR_IPV4 ? 20u : 40u) > len) return PKT_ICMPE_SPAN;
    if (f.eth == kIcmpNoEther) return PKT_ICMPE_NO_ETHER;
    if (f.eth + 14u > f.ipo) return PKT_ICMPE_SPAN;
    return PKT_ICMPE_SENT;
}

// steps 1 and 2 from the select byte and the reason
PKT_HD uint32_t icmp_reason_status(uint32_t sel, uint32_t r) {
    if (!sel || r == PKT_ICMP_R_NONE) return PKT_ICMPE_SKIPPED;
    if (r > PKT_ICMP_R_PORT_UNREACH) return PKT_ICMPE_BAD_REASON;
    return PKT_ICMPE_SENT;
}

// A source packet's plan: what the build step needs, none of it read from the packet again except the prefix and the
// quote.  32 bytes in the device's scratch (icmp_pack / icmp_unpack).
struct IcmpPlan {
    uint32_t st;        // pkt_icmpe_status_t
    uint32_t v4;        // the IP entry is IPv4
    uint32_t eth, ipo;  // the Ether and the IP entry's offsets
    uint32_t e_eth, e_ip;
    uint32_t q;         // Q, the quote's bytes
    uint32_t type, code;
    uint32_t mtu;       // TOO_BIG's, else 0
    uint32_t sa[4];     // the source packet's source address as it lies in memory (little-endian dwords; IPv4: sa[0])
};

PKT_HD uint32_t icmp_hlen(const IcmpPlan& p) { return p.v4 ? 20u : 40u; }
PKT_HD uint32_t icmp_out_len(const IcmpPlan& p) { return p.ipo - p.eth + icmp_hlen(p) + 8u + p.q; }

// steps 5 to 11 for a packet whose entries are found (icmp_find_status said SENT) and whose reason r is 1..6.
// h[k] = the IP entry's bytes 4k .. 4k + 3 as a little-endian dword: k < 5 for IPv4, k < 7 for IPv6 (bytes 0..27).
// tb = the byte at ip_off + H if that lies inside the packet's len bytes (else anything); ed0 = the Ether
// destination's first byte; m = the packet's mtu.
PKT_HD void icmp_decide(IcmpPlan& p, const IcmpFind& f, uint32_t len, uint32_t r, const uint32_t h[7], uint32_t tb,
                        uint32_t ed0, uint32_t m, const IcmpCfg& cfg) {
    const bool v4 = f.ipt == PKT_HDR_IPV4;
    p.v4 = v4 ? 1u : 0u;
    p.eth = f.eth, p.ipo = f.ipo, p.e_eth = f.e_eth, p.e_ip = f.e_ip;
    const uint32_t H = v4 ? 20u : 40u;
    const bool nosrc = v4 ? cfg.s4 == 0 : (cfg.s6[0] | cfg.s6[1] | cfg.s6[2] | cfg.s6[3]) == 0;
    if (nosrc) {
        p.st = PKT_ICMPE_NO_SRC;
        return;
    }
    const uint32_t L = v4 ? fwd_be16(h[0] >> 16) : 40u + fwd_be16(h[1]);
    if (v4 ? ((h[0] & 0xFFu) != 0x45u || L < 20u) : ((h[0] >> 4 & 0xFu) != 6u)) {
        p.st = PKT_ICMPE_BAD_HDR;
        return;
    }
    if (v4 && (fwd_be16(h[1] >> 16) & 0x1FFFu) != 0) {
        p.st = PKT_ICMPE_FRAGMENT;
        return;
    }
    const uint32_t s0 = (v4 ? h[3] : h[2]) & 0xFFu;
    const bool badsrc = v4 ? (s0 == 0 || s0 == 127u || s0 >= 224u) : ((h[2] | h[3] | h[4] | h[5]) == 0 || s0 == 0xFFu);
    if (badsrc) {
        p.st = PKT_ICMPE_BAD_SRC;
        return;
    }
    const uint32_t d0 = (v4 ? h[4] : h[6]) & 0xFFu;
    const bool mc = (ed0 & 1u) || (v4 ? d0 >= 224u : d0 == 0xFFu);
    if (mc && !(!v4 && r == PKT_ICMP_R_TOO_BIG)) {
        p.st = PKT_ICMPE_MCAST;
        return;
    }
    const uint32_t proto = v4 ? h[2] >> 8 & 0xFFu : h[1] >> 16 & 0xFFu;
    const uint32_t end = f.ipo + L < len ? f.ipo + L : len;
    if (proto == (v4 ? 1u : 58u)) {
        const bool missing = f.ipo + H >= end;
        const uint32_t t = tb & 0xFFu;
        const bool err = v4 ? (t == 3u || t == 4u || t == 5u || t == 11u || t == 12u) : (t < 128u || t == 137u);
        if (missing || err) {
            p.st = PKT_ICMPE_ICMP_ERR;
            return;
        }
    }
    p.st = PKT_ICMPE_SENT;
    const uint32_t avail = end - f.ipo, room = (v4 ? cfg.max4 : cfg.max6) - H - 8u;
    p.q = avail < room ? avail : room;
    const uint32_t tc = icmp_type_code(r);
    p.type = v4 ? tc & 0xFFu : tc >> 16 & 0xFFu;
    p.code = v4 ? tc >> 8 & 0xFFu : tc >> 24;
    p.mtu = r == PKT_ICMP_R_TOO_BIG ? m : 0u;
    p.sa[0] = v4 ? h[3] : h[2];
    p.sa[1] = v4 ? 0u : h[3];
    p.sa[2] = v4 ? 0u : h[4];
    p.sa[3] = v4 ? 0u : h[5];
}

// the two halves of a big-endian word, added
PKT_HD uint32_t icmp_halves(uint32_t w) { return (w >> 16) + (w & 0xFFFFu); }
PKT_HD uint32_t icmp_fold(uint32_t s) {
    s = (s & 0xFFFFu) + (s >> 16);
    s = (s & 0xFFFFu) + (s >> 16);
    return s;
}

// Output q's IP and ICMP header as it lies in memory: w[k] = bytes 4k .. 4k + 3 as a little-endian dword, 7 words
// under IPv4 and 12 under IPv6 (the rest zero), with the ICMP checksum field zero.  Returns the ICMP message's RFC
// 1071 sum without the quote: the ICMP header's words and, under IPv6, the pseudo-header.
PKT_HD uint32_t icmp_headers(const IcmpPlan& p, uint64_t q, const IcmpCfg& cfg, uint32_t w[12]) {
    uint32_t W[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t part;
    if (p.v4) {
        W[0] = 0x45u << 24 | cfg.tos << 16 | (28u + p.q);
        W[1] = ((cfg.ident + (uint32_t)q) & 0xFFFFu) << 16;
        W[2] = cfg.ttl << 24 | 1u << 16;
        W[3] = cfg.s4;
        W[4] = icmp_bswap32(p.sa[0]);
        uint32_t s = 0;
        for (uint32_t k = 0; k < 5; k++) s += icmp_halves(W[k]);
        W[2] |= ~icmp_fold(s) & 0xFFFFu;
        W[5] = p.type << 24 | p.code << 16;
        W[6] = p.mtu & 0xFFFFu;
        part = icmp_halves(W[5]) + icmp_halves(W[6]);
    } else {
        W[0] = 6u << 28 | cfg.tos << 20;
        W[1] = (8u + p.q) << 16 | 58u << 8 | cfg.ttl;
        part = 8u + p.q + 58u;
        for (uint32_t k = 0; k < 4; k++) {
            W[2 + k] = cfg.s6[k];
            W[6 + k] = icmp_bswap32(p.sa[k]);
            part += icmp_halves(W[2 + k]) + icmp_halves(W[6 + k]);
        }
        W[10] = p.type << 24 | p.code << 16;
        W[11] = p.mtu;
        part += icmp_halves(W[10]) + icmp_halves(W[11]);
    }
    for (uint32_t k = 0; k < 12; k++) w[k] = icmp_bswap32(W[k]);
    return part;
}

// The ICMP checksum field from the headers' part and the quote's RFC 1071 sum (any 32-bit partial sum of its
// big-endian 16-bit words): a computed 0 is 0xFFFF under IPv6 and 0 under IPv4.
PKT_HD uint32_t icmp_csum(const IcmpPlan& p, uint32_t part, uint32_t quote) {
    const uint32_t c = ~icmp_fold(icmp_fold(part) + icmp_fold(quote)) & 0xFFFFu;
    return !p.v4 && c == 0 ? 0xFFFFu : c;
}

// ---- the refusals both entry points share: the text (after "pkt_icmp_err_batch: "), or nullptr; the contract's own last.
// device: pkt_icmp_err_batch (the slab's alignment rule); else pkt_icmp_err_host.
inline const char* icmp_call_error(const pkt_batch_t* b, const pkt_chain_t* chain, uint32_t which_ip, uint32_t flags,
                                   const pkt_icmp_cfg_t* cfg, uint32_t code_all, const uint16_t* mtu, uint32_t mtu_all,
                                   const uint8_t* dst, uint64_t out_cap, const uint64_t* out_off, const uint32_t* out_len,
                                   const uint64_t* hits, bool device) {
    if (!b || !chain) return "null argument";
    if (!cfg) return "null cfg";
    if (b->n >= (1ull << 32)) return "n >= 2^32";
    if (flags & ~kIcmpFlags) return "unknown flag bits";
    if (which_ip >= PKT_MAX_HDRS && which_ip != PKT_FLOW_LAST) return "which_ip is neither below 16 nor PKT_FLOW_LAST";
    bool any = false;
    for (uint32_t k = 0; k < 4; k++) any = any || cfg->src4[k];
    for (uint32_t k = 0; k < 16; k++) any = any || cfg->src6[k];
    if (!any) return "cfg has neither an IPv4 nor an IPv6 source address";
    if (cfg->max4 && cfg->max4 < 56u) return "max4 below 56";
    if (cfg->max6 && cfg->max6 < 96u) return "max6 below 96";
    if (code_all > 255u) return "code_all above 255";
    if (mtu_all > 65535u) return "mtu_all above 65535";
    if ((uintptr_t)mtu & 1) return "mtu not 2-byte aligned";
    return out_call_error(b, chain, flags & PKT_ICMPE_NO_WRITE, "null dst, out_off or out_len without PKT_ICMPE_NO_WRITE", dst,
                          out_cap, out_off, out_len, hits, device);
}
