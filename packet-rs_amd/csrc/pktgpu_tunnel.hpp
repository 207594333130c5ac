// pktgpu_tunnel.hpp — what the two halves of pkt_tunnel_* share: the table's checks and its decap lookup (built on the
// host by pkt_tunnel_create / _create_host, read-only afterwards), the chain search, the per-packet decisions of
// include/pktgpu.h step by step for encap and decap, the plan both leave, the outer header words with their RFC 1071
// sums, the out_chain rows and the refusals with their texts.  pktgpu_tunnel.hip holds pkt_tunnel_create, the
// _batch / _async / _result entries and the kernels; pktgpu_host.cpp holds pkt_tunnel_create_host, _destroy,
// _last_error and the sequential loops of pkt_tunnel_encap_host / _decap_host (it compiles under g++ alone).  Both
// call the same inline code, the pktgpu_icmp.hpp pattern: the device and the host path differ only in how bytes move.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "pktgpu_batch.hpp"
#include "pktgpu_frag.hpp"
#include "pktgpu_outbatch.hpp"

static_assert(sizeof(pkt_tunnel_entry_t) == 64, "tunnel ABI struct");
static_assert(PKT_TUN_NONE == PKT_FRAG_NONE, "one NONE");

constexpr uint32_t kTunCallFlags = PKT_TUN_NO_WRITE;
constexpr uint32_t kTunEntryFlags =
    PKT_TUN_F_KEY | PKT_TUN_F_DF | PKT_TUN_F_INHERIT_TOS | PKT_TUN_F_UDP_CSUM | PKT_TUN_F_ANY_REMOTE;
constexpr uint32_t kTunNoRead = 0xFFFFFFFFu;

// An entry as the kernels read it: the 64 bytes of pkt_tunnel_entry_t as sixteen little-endian dwords, four aligned
// 16-byte loads.  w[0] = kind | ipver << 8 | ttl << 16 | tos << 24, w[1] = flags, w[2] = id, w[3] = sport_lo |
// sport_hi << 16, w[4..7] = src and w[8..11] = dst as they lie in a packet, w[12..14] = eth_dst | eth_src likewise.
struct alignas(16) TunEnt {
    uint32_t w[16];
};
static_assert(sizeof(TunEnt) == sizeof(pkt_tunnel_entry_t), "TunEnt is the entry's bytes");

PKT_HD uint32_t tun_kind(const TunEnt& e) { return e.w[0] & 0xFFu; }
PKT_HD uint32_t tun_ipver(const TunEnt& e) { return e.w[0] >> 8 & 0xFFu; }
PKT_HD uint32_t tun_ttl(const TunEnt& e) { return (e.w[0] >> 16 & 0xFFu) ? (e.w[0] >> 16 & 0xFFu) : 64u; }
PKT_HD uint32_t tun_tos(const TunEnt& e) { return e.w[0] >> 24; }
PKT_HD uint32_t tun_flags(const TunEnt& e) { return e.w[1]; }
// the id an entry is matched by: the VNI, the GRE key when it carries one, else 0
PKT_HD uint32_t tun_match_id(const TunEnt& e) {
    const uint32_t k = tun_kind(e);
    return k == PKT_TUN_VXLAN || (k == PKT_TUN_GRE && (e.w[1] & PKT_TUN_F_KEY)) ? e.w[2] : 0u;
}

PKT_HD uint32_t tun_bswap32(uint32_t x) { return x << 24 | (x & 0xFF00u) << 8 | (x >> 8 & 0xFF00u) | x >> 24; }
PKT_HD uint32_t tun_halves(uint32_t w) { return (w >> 16) + (w & 0xFFFFu); }
PKT_HD uint32_t tun_fold(uint32_t s) {
    s = (s & 0xFFFFu) + (s >> 16);
    s = (s & 0xFFFFu) + (s >> 16);
    return s;
}

// ---- the decap lookup: open addressing with linear probing over the entries' decap keys.  slots[k] = entry index + 1,
// 0 = empty; nslots a power of two, at least twice the entries, so a probe always ends at an empty slot.
struct TunView {
    const TunEnt* ent;
    const uint32_t* slots;
    uint32_t n, mask;  // entries; nslots - 1
};

// A decap key: what a packet shows (kind, outer version, GRE key present, local = its destination, remote = its source
// or the wildcard, id).  a[] / b[]: the addresses as they lie in a packet (little-endian dwords; IPv4: [0], rest 0).
struct TunKey {
    uint32_t kind, ipver, has_key, wild, id;
    uint32_t local[4], remote[4];
};

PKT_HD uint32_t tun_key_hash(const TunKey& k) {
    uint32_t h = 0x811C9DC5u ^ (k.kind | k.ipver << 8 | k.has_key << 16 | k.wild << 17);
    h = (h ^ k.id) * 0x01000193u;
    for (uint32_t j = 0; j < 4; j++) h = (h ^ k.local[j]) * 0x01000193u, h ^= h >> 15;
    if (!k.wild)
        for (uint32_t j = 0; j < 4; j++) h = (h ^ k.remote[j]) * 0x01000193u, h ^= h >> 13;
    return h * 0x9E3779B1u;
}

// the key an entry is found by (local = its src, remote = its dst unless ANY_REMOTE)
PKT_HD TunKey tun_entry_key(const TunEnt& e) {
    TunKey k;
    k.kind = tun_kind(e), k.ipver = tun_ipver(e);
    k.has_key = k.kind == PKT_TUN_GRE && (e.w[1] & PKT_TUN_F_KEY) ? 1u : 0u;
    k.wild = e.w[1] & PKT_TUN_F_ANY_REMOTE ? 1u : 0u;
    k.id = tun_match_id(e);
    const uint32_t nw = k.ipver == 4 ? 1u : 4u;
    for (uint32_t j = 0; j < 4; j++) {
        k.local[j] = j < nw ? e.w[4 + j] : 0u;
        k.remote[j] = j < nw && !k.wild ? e.w[8 + j] : 0u;
    }
    return k;
}

PKT_HD bool tun_key_eq(const TunKey& a, const TunKey& b) {
    bool eq = a.kind == b.kind && a.ipver == b.ipver && a.has_key == b.has_key && a.wild == b.wild && a.id == b.id;
    for (uint32_t j = 0; j < 4; j++) eq = eq && a.local[j] == b.local[j] && a.remote[j] == b.remote[j];
    return eq;
}

// the entry with key k, or PKT_TUN_NONE
PKT_HD uint32_t tun_find(const TunView& v, const TunKey& k) {
    uint32_t pos = tun_key_hash(k) & v.mask;
    for (uint32_t probes = 0; probes <= v.mask; probes++, pos = (pos + 1u) & v.mask) {
        const uint32_t s = v.slots[pos];
        if (!s) return PKT_TUN_NONE;
        if (tun_key_eq(tun_entry_key(v.ent[s - 1u]), k)) return s - 1u;
    }
    return PKT_TUN_NONE;
}

// the exact key first, then the ANY_REMOTE one
PKT_HD uint32_t tun_lookup(const TunView& v, TunKey k) {
    k.wild = 0;
    const uint32_t t = tun_find(v, k);
    if (t != PKT_TUN_NONE) return t;
    k.wild = 1;
    for (uint32_t j = 0; j < 4; j++) k.remote[j] = 0;
    return tun_find(v, k);
}

// ---- the table's refusals and its lookup image (host code).  The text follows "pkt_tunnel_create: ".
struct TunImage {
    std::vector<TunEnt> ent;
    std::vector<uint32_t> slots;
};

inline int tun_compile(const pkt_tunnel_entry_t* entries, uint32_t n, TunImage& img, std::string& err) {
    const auto refuse = [&](const std::string& msg) {
        err = "pkt_tunnel_create: " + msg;
        return PKT_ERR_INVALID_ARG;
    };
    if (!entries) return refuse("null entries");
    if (n == 0 || n > PKT_TUN_MAX_ENTRIES) return refuse("count is 0 or above PKT_TUN_MAX_ENTRIES");
    for (uint32_t i = 0; i < n; i++) {
        const pkt_tunnel_entry_t& e = entries[i];
        const std::string at = "entry " + std::to_string(i) + ": ";
        if (e.kind > PKT_TUN_IPIP) return refuse(at + "unknown kind");
        if (e.ipver != 4 && e.ipver != 6) return refuse(at + "ipver is neither 4 nor 6");
        if (e.flags & ~kTunEntryFlags) return refuse(at + "unknown flag bits");
        if (e.kind == PKT_TUN_VXLAN && e.id > 0xFFFFFFu) return refuse(at + "VNI above 2^24 - 1");
        if (e.sport_lo > e.sport_hi) return refuse(at + "sport_lo above sport_hi");
        if ((e.flags & PKT_TUN_F_KEY) && e.kind != PKT_TUN_GRE) return refuse(at + "PKT_TUN_F_KEY on an entry that is not GRE");
        if ((e.flags & PKT_TUN_F_UDP_CSUM) && e.kind != PKT_TUN_VXLAN)
            return refuse(at + "PKT_TUN_F_UDP_CSUM on an entry that is not VXLAN");
        if (e.zero) return refuse(at + "non-zero `zero`");
    }
    img.ent.resize(n);
    memcpy(static_cast<void*>(img.ent.data()), entries, (size_t)n * sizeof(TunEnt));
    uint32_t nslots = 16;
    while (nslots < 2u * n) nslots <<= 1;
    img.slots.assign(nslots, 0u);
    const TunView v{img.ent.data(), img.slots.data(), n, nslots - 1u};
    for (uint32_t i = 0; i < n; i++) {
        const TunKey k = tun_entry_key(img.ent[i]);
        const uint32_t had = tun_find(v, k);
        if (had != PKT_TUN_NONE)
            return refuse("entries " + std::to_string(had) + " and " + std::to_string(i) + " have the same decap key");
        uint32_t pos = tun_key_hash(k) & v.mask;
        while (img.slots[pos]) pos = (pos + 1u) & v.mask;
        img.slots[pos] = i + 1u;
    }
    return PKT_SUCCESS;
}

// The handle.  A host handle keeps the image; a device handle keeps one device allocation holding both arrays.
struct pkt_tunnel {
    bool device = false;
    int device_id = 0;
    void* dev_buf = nullptr;
    int (*destroy)(pkt_tunnel*) = nullptr;  // the device handle's release (pktgpu_tunnel.hip)
    TunImage img;
    TunView v{};
    mutable std::string err;
};

// ---- the chain search.  The caller feeds the list's entries j < min(n_hdrs, PKT_MAX_HDRS) in order.  It keeps the
// chosen IP entry (pkt_fwd_batch's rule: which_ip counts IPv4 and IPv6 entries together, PKT_FLOW_LAST the last), the
// type of the entry before it, the three entries behind it, and the list's first IP entry.
struct TunFind {
    uint32_t ipt = 0, ipo = 0, e = 0;  // the chosen IP entry's type (0: none), offset and index
    uint32_t prev = 0, last = 0;       // the type of the entry before it (0: it is entry 0); of the entry before j
    uint32_t t1 = 0, o1 = 0, t2 = 0, o2 = 0, t3 = 0;  // the entries at e + 1, e + 2, e + 3 (type 0: none)
    uint32_t f_ipt = 0, f_ipo = 0;     // the first IP entry of the list
    uint32_t seen = 0;
};

PKT_HD void tun_find_step(TunFind& f, uint32_t which, uint32_t j, uint32_t ty, uint32_t of) {
    const bool ip = fwd_is_ip(ty);
    const bool take = ip && (which == PKT_FLOW_LAST || f.seen == which);
    const uint32_t d = f.ipt && !take ? j - f.e : 0u;
    f.t1 = take ? 0u : d == 1u ? ty : f.t1;
    f.o1 = d == 1u ? of : f.o1;
    f.t2 = take ? 0u : d == 2u ? ty : f.t2;
    f.o2 = d == 2u ? of : f.o2;
    f.t3 = take ? 0u : d == 3u ? ty : f.t3;
    f.prev = take ? f.last : f.prev;
    f.ipt = take ? ty : f.ipt;
    f.ipo = take ? of : f.ipo;
    f.e = take ? j : f.e;
    const bool first = ip && !f.f_ipt;
    f.f_ipt = first ? ty : f.f_ipt;
    f.f_ipo = first ? of : f.f_ipo;
    f.seen += ip ? 1u : 0u;
    f.last = ty;
}

// ---- the plan: what the build step needs of a source packet, none of it read from the packet again but the bytes
// it copies.  An output is  source [0, P) (its ethertype bytes P - 2, P - 1 set when `patch`)  |  hl header bytes
// (encap)  |  source [P + S, P + S + I).  Its rows: the source's rows [0, keep), `add` outer rows (encap), the
// source's rows [rskip, nh) with hdr_off + hl - S.  32 bytes in the device's scratch.
struct TunPlan {
    uint32_t st;
    uint32_t keep, rskip, nh, add;
    uint32_t patch, et6;  // set the ethertype before P: to 0x86DD (et6) or 0x0800
    uint32_t hl, cs;      // header bytes; the UDP checksum is computed
    uint32_t P, S, I;
    uint32_t tos, sport, in6;  // encap: the outer tos, the UDP source port, the inner packet is IPv6
    uint32_t t;           // encap: the entry
};

PKT_HD uint32_t tun_out_len(const TunPlan& p) { return p.P + p.hl + p.I; }

PKT_HD void tun_plan_pack(const TunPlan& p, uint32_t a[4], uint32_t b[4]) {
    a[0] = p.st | p.keep << 4 | p.rskip << 9 | p.nh << 14 | p.add << 19 | p.patch << 22 | p.et6 << 23 | p.hl << 24 | p.cs << 31;
    a[1] = p.P | p.S << 16;
    a[2] = p.I | p.tos << 16 | p.in6 << 24;
    a[3] = p.t;
    b[0] = p.sport, b[1] = b[2] = b[3] = 0;
}
PKT_HD TunPlan tun_plan_unpack(const uint32_t a[4], const uint32_t b[4]) {
    TunPlan p;
    p.st = a[0] & 15u, p.keep = a[0] >> 4 & 31u, p.rskip = a[0] >> 9 & 31u, p.nh = a[0] >> 14 & 31u;
    p.add = a[0] >> 19 & 7u, p.patch = a[0] >> 22 & 1u, p.et6 = a[0] >> 23 & 1u, p.hl = a[0] >> 24 & 127u, p.cs = a[0] >> 31;
    p.P = a[1] & 0xFFFFu, p.S = a[1] >> 16;
    p.I = a[2] & 0xFFFFu, p.tos = a[2] >> 16 & 0xFFu, p.in6 = a[2] >> 24 & 1u;
    p.t = a[3];
    p.sport = b[0];
    return p;
}

PKT_HD bool tun_is_l2tag(uint32_t ty) { return ty == PKT_HDR_ETHER || ty == PKT_HDR_VLAN || ty == PKT_HDR_MPLS; }
PKT_HD bool tun_has_etype(uint32_t ty) { return ty == PKT_HDR_ETHER || ty == PKT_HDR_VLAN; }

// the outer header bytes an entry adds: Ether 14 (VXLAN), IP 20 / 40, UDP + VXLAN 16, GRE 4 + 4 with a key
PKT_HD uint32_t tun_hdr_len(const TunEnt& e) {
    const uint32_t k = tun_kind(e), H = tun_ipver(e) == 4 ? 20u : 40u;
    if (k == PKT_TUN_VXLAN) return 14u + H + 16u;
    if (k == PKT_TUN_GRE) return H + 4u + (e.w[1] & PKT_TUN_F_KEY ? 4u : 0u);
    return H;
}

// ---- encap.  Steps 3 to 5 of the contract from the search alone: PKT_TUNE_OK for "go on", and `rd`, the packet offset
// whose 8 bytes tun_encap_decide wants as h[] (kTunNoRead: none).  Steps 1 and 2 are the caller's.
PKT_HD uint32_t tun_encap_find_status(const TunFind& f, const TunEnt& e, uint32_t len, uint32_t& rd) {
    rd = kTunNoRead;
    if (tun_kind(e) == PKT_TUN_VXLAN) {
        if ((e.w[1] & PKT_TUN_F_INHERIT_TOS) && f.f_ipt && f.f_ipo + 2u <= len) rd = f.f_ipo;
        return PKT_TUNE_OK;
    }
    if (!f.ipt) return PKT_TUNE_NO_IP;
    if (f.ipo + (f.ipt == PKT_HDR_IPV4 ? 20u : 40u) > len) return PKT_TUNE_SPAN;
    if (f.e != 0 && !tun_is_l2tag(f.prev)) return PKT_TUNE_BAD_L2;
    if (f.e != 0 && tun_has_etype(f.prev) && f.ipo < 2u) return PKT_TUNE_SPAN;
    rd = f.ipo;
    return PKT_TUNE_OK;
}

// the tos / traffic class of an IP header from its first dword as it lies in memory
PKT_HD uint32_t tun_ip_tos(uint32_t h0, bool v4) { return v4 ? h0 >> 8 & 0xFFu : ((h0 & 0xFu) << 4 | (h0 >> 12 & 0xFu)); }

// Steps 6 to 10 for a packet whose search said OK.  h[k] = the bytes 4k .. 4k + 3 at `rd` as a little-endian dword
// (k < 2; anything when rd was kTunNoRead); nh = min(n_hdrs, PKT_MAX_HDRS); ent = the packet's entropy (0: none).
PKT_HD void tun_encap_decide(TunPlan& p, const TunFind& f, const TunEnt& e, uint32_t t, uint32_t nh, uint32_t len,
                             uint32_t rd, const uint32_t h[2], uint32_t ent) {
    const uint32_t kind = tun_kind(e), fl = e.w[1], hl = tun_hdr_len(e);
    const bool o4 = tun_ipver(e) == 4;
    p.t = t, p.nh = nh, p.hl = hl, p.S = 0;
    p.tos = tun_tos(e);
    p.patch = p.et6 = p.cs = p.in6 = 0;
    p.sport = 0;
    if (kind == PKT_TUN_VXLAN) {
        if (rd != kTunNoRead) p.tos = tun_ip_tos(h[0], f.f_ipt == PKT_HDR_IPV4);
        p.P = 0, p.I = len, p.keep = 0, p.rskip = 0, p.add = 4;
        p.cs = fl & PKT_TUN_F_UDP_CSUM ? 1u : 0u;
        const uint32_t lo = e.w[3] & 0xFFFFu, hi = e.w[3] >> 16;
        p.sport = lo + ent % (hi - lo + 1u);
        if ((o4 ? 36u : 16u) + len > 65535u) {
            p.st = PKT_TUNE_TOO_BIG;
            return;
        }
    } else {
        const bool v4 = f.ipt == PKT_HDR_IPV4;
        const uint32_t L = v4 ? fwd_be16(h[0] >> 16) : 40u + fwd_be16(h[1]);
        if (v4 ? ((h[0] & 0xFFu) != 0x45u || L < 20u) : ((h[0] >> 4 & 0xFu) != 6u)) {
            p.st = PKT_TUNE_BAD_HDR;
            return;
        }
        if (f.ipo + L > len) {
            p.st = PKT_TUNE_TRUNC;
            return;
        }
        if (fl & PKT_TUN_F_INHERIT_TOS) p.tos = tun_ip_tos(h[0], v4);
        p.in6 = v4 ? 0u : 1u;
        p.P = f.ipo, p.I = L, p.keep = f.e, p.rskip = f.e;
        p.add = kind == PKT_TUN_IPIP ? 1u : fl & PKT_TUN_F_KEY ? 3u : 2u;
        p.patch = f.e != 0 && tun_has_etype(f.prev) ? 1u : 0u;
        p.et6 = o4 ? 0u : 1u;
        if (hl - (o4 ? 0u : 40u) + L > 65535u) {
            p.st = PKT_TUNE_TOO_BIG;
            return;
        }
    }
    if (nh + p.add > PKT_MAX_HDRS) {
        p.st = PKT_TUNE_DEPTH;
        return;
    }
    p.st = PKT_TUNE_OK;
}

// Output q's outer header as it lies in memory: d[k] = header bytes 4k .. 4k + 3 as a little-endian dword, hl bytes
// (the rest zero), the UDP checksum field zero.  Returns the UDP datagram's RFC 1071 sum without the inner bytes: the
// pseudo-header, the UDP header and the VXLAN header (0 for the other kinds).
PKT_HD uint32_t tun_headers(const TunPlan& p, const TunEnt& e, uint64_t q, uint32_t ident, uint32_t d[18]) {
    const uint32_t kind = tun_kind(e), fl = e.w[1];
    const bool o4 = tun_ipver(e) == 4;
    const uint32_t H = o4 ? 20u : 40u, ipl = p.hl - (kind == PKT_TUN_VXLAN ? 14u : 0u) + p.I;  // the outer IP packet's bytes
    const uint32_t proto = kind == PKT_TUN_VXLAN ? 17u : kind == PKT_TUN_GRE ? 47u : p.in6 ? 41u : 4u;
    uint32_t W[14];
    for (uint32_t k = 0; k < 14; k++) W[k] = 0;
    uint32_t nw, part = 0;
    if (o4) {
        W[0] = 0x45u << 24 | p.tos << 16 | ipl;
        W[1] = ((ident + (uint32_t)q) & 0xFFFFu) << 16 | (fl & PKT_TUN_F_DF ? 0x4000u : 0u);
        W[2] = tun_ttl(e) << 24 | proto << 16;
        W[3] = tun_bswap32(e.w[4]);
        W[4] = tun_bswap32(e.w[8]);
        uint32_t s = 0;
        for (uint32_t k = 0; k < 5; k++) s += tun_halves(W[k]);
        W[2] |= ~tun_fold(s) & 0xFFFFu;
        part = tun_halves(W[3]) + tun_halves(W[4]);
        nw = 5;
    } else {
        W[0] = 6u << 28 | p.tos << 20;
        W[1] = (ipl - 40u) << 16 | proto << 8 | tun_ttl(e);
        for (uint32_t k = 0; k < 4; k++) {
            W[2 + k] = tun_bswap32(e.w[4 + k]);
            W[6 + k] = tun_bswap32(e.w[8 + k]);
            part += tun_halves(W[2 + k]) + tun_halves(W[6 + k]);
        }
        nw = 10;
    }
    if (kind == PKT_TUN_VXLAN) {
        const uint32_t ul = ipl - H;
        W[nw] = p.sport << 16 | 4789u;
        W[nw + 1] = ul << 16;
        W[nw + 2] = 0x08000000u;
        W[nw + 3] = e.w[2] << 8;
        part += 17u + ul;
        for (uint32_t k = 0; k < 4; k++) part += tun_halves(W[nw + k]);
        nw += 4;
    } else {
        part = 0;
        if (kind == PKT_TUN_GRE) {
            W[nw] = (fl & PKT_TUN_F_KEY ? 0x20000000u : 0u) | (p.in6 ? 0x86DDu : 0x0800u);
            nw += 1;
            if (fl & PKT_TUN_F_KEY) W[nw++] = e.w[2];
        }
    }
    for (uint32_t k = 0; k < 18; k++) d[k] = 0;
    if (kind == PKT_TUN_VXLAN) {  // the Ether header's 14 bytes put the IP words at a 2-byte phase
        d[0] = e.w[12], d[1] = e.w[13], d[2] = e.w[14];
        uint32_t prevw = o4 ? 0x0008u : 0xDD86u;  // the ethertype as it lies in memory
        for (uint32_t k = 0; k < 14; k++) {
            const uint32_t x = k < nw ? tun_bswap32(W[k]) : 0u;
            d[3 + k] = prevw | x << 16;
            prevw = x >> 16;
        }
        d[17] = prevw;
    } else {
        for (uint32_t k = 0; k < 14; k++) d[k] = k < nw ? tun_bswap32(W[k]) : 0u;
    }
    return part;
}

// the header dword and the shift of the UDP checksum's two bytes (VXLAN entries: header byte 14 + H + 6)
PKT_HD uint32_t tun_csum_word(const TunEnt& e) { return tun_ipver(e) == 4 ? 10u : 15u; }

// The UDP checksum field from the headers' part and the inner bytes' RFC 1071 sum (any 32-bit partial sum of their
// big-endian 16-bit words): a computed 0 is stored as 0xFFFF.
PKT_HD uint32_t tun_udp_csum(uint32_t part, uint32_t inner) {
    const uint32_t c = ~tun_fold(tun_fold(part) + tun_fold(inner)) & 0xFFFFu;
    return c == 0 ? 0xFFFFu : c;
}

// ---- decap.  Steps 2 and 3 from the search alone (PKT_TUND_OK: the IP header's H bytes lie inside the packet).
PKT_HD uint32_t tun_decap_find_status(const TunFind& f, uint32_t len) {
    if (!f.ipt) return PKT_TUND_NO_IP;
    if (f.ipo + (f.ipt == PKT_HDR_IPV4 ? 20u : 40u) > len) return PKT_TUND_SPAN;
    return PKT_TUND_OK;
}

// Steps 4 to 12.  ip[k] = the outer IP header's bytes 4k .. 4k + 3 as a little-endian dword (k < 5 / 10), th[k] the
// same for the 16 bytes behind it (bytes past the packet's length: anything, they are not used).  *tunnel_out = the
// matched entry.
PKT_HD void tun_decap_decide(TunPlan& p, const TunFind& f, uint32_t nh, uint32_t len, const uint32_t ip[10],
                             const uint32_t th[4], const TunView& v, uint32_t& tunnel_out) {
    const bool v4 = f.ipt == PKT_HDR_IPV4;
    const uint32_t H = v4 ? 20u : 40u, at = f.ipo + H;
    tunnel_out = PKT_TUN_NONE;
    p.nh = nh, p.hl = 0, p.add = 0, p.cs = 0, p.tos = 0, p.sport = 0, p.in6 = 0, p.t = PKT_TUN_NONE;
    p.patch = p.et6 = 0;
    if (v4 ? (ip[0] & 0xFFu) != 0x45u : (ip[0] >> 4 & 0xFu) != 6u) {
        p.st = PKT_TUND_BAD_HDR;
        return;
    }
    if (v4 && (fwd_be16(ip[1] >> 16) & 0x3FFFu) != 0) {
        p.st = PKT_TUND_FRAGMENT;
        return;
    }
    uint32_t kind, T;
    if (f.t1 == PKT_HDR_UDP && f.o1 == at && f.t2 == PKT_HDR_VXLAN && f.o2 == at + 8u) {
        kind = PKT_TUN_VXLAN, T = 16;
    } else if (f.t1 == PKT_HDR_GRE && f.o1 == at) {
        kind = PKT_TUN_GRE, T = 4;
    } else if (fwd_is_ip(f.t1) && f.o1 == at) {
        kind = PKT_TUN_IPIP, T = 0;
    } else {
        p.st = PKT_TUND_NOT_TUNNEL;
        return;
    }
    if (at + T > len) {
        p.st = PKT_TUND_SPAN;
        return;
    }
    const uint32_t Lo = v4 ? fwd_be16(ip[0] >> 16) : 40u + fwd_be16(ip[1]);
    TunKey k;
    k.kind = kind, k.ipver = v4 ? 4u : 6u, k.has_key = 0, k.wild = 0, k.id = 0;
    bool in6 = f.t1 == PKT_HDR_IPV6;
    if (kind == PKT_TUN_VXLAN) {
        if (fwd_be16(th[1]) != Lo - H) {  // the UDP length
            p.st = PKT_TUND_BAD_HDR;
            return;
        }
        k.id = tun_bswap32(th[3]) >> 8;
    } else if (kind == PKT_TUN_GRE) {
        const uint32_t b0 = th[0] & 0xFFu, b1 = th[0] >> 8 & 0xFFu, proto = fwd_be16(th[0] >> 16);
        const bool rows = f.t2 == PKT_HDR_GRE_CHKSUM_OFFSET || f.t2 == PKT_HDR_GRE_SEQUENCE_NUM ||
                          f.t3 == PKT_HDR_GRE_CHKSUM_OFFSET || f.t3 == PKT_HDR_GRE_SEQUENCE_NUM;
        if ((b0 & 0xD0u) || (b1 & 7u) || (proto != 0x0800u && proto != 0x86DDu) || rows) {
            p.st = PKT_TUND_BAD_GRE;
            return;
        }
        in6 = proto == 0x86DDu;
        if (b0 & 0x20u) {
            T = 8;
            if (at + T > len) {
                p.st = PKT_TUND_SPAN;
                return;
            }
            k.has_key = 1, k.id = tun_bswap32(th[1]);
        }
    }
    for (uint32_t j = 0; j < 4; j++) {
        k.remote[j] = v4 ? (j == 0 ? ip[3] : 0u) : ip[2 + j];
        k.local[j] = v4 ? (j == 0 ? ip[4] : 0u) : ip[6 + j];
    }
    tunnel_out = tun_lookup(v, k);
    if (tunnel_out == PKT_TUN_NONE) {
        p.st = PKT_TUND_NO_MATCH;
        return;
    }
    if (f.ipo + Lo > len) {
        p.st = PKT_TUND_TRUNC;
        return;
    }
    const uint32_t I = Lo < H + T ? 0u : Lo - H - T;
    const uint32_t rows = kind == PKT_TUN_VXLAN ? 3u : kind == PKT_TUN_GRE ? (T == 8u ? 3u : 2u) : 1u;  // the outer rows from e on
    if (kind == PKT_TUN_VXLAN ? (f.e + rows >= nh || I < 14u) : I < (in6 ? 40u : 20u)) {
        p.st = PKT_TUND_NO_INNER;
        return;
    }
    p.I = I;
    p.in6 = in6 ? 1u : 0u;
    p.t = tunnel_out;
    if (kind == PKT_TUN_VXLAN) {
        p.P = 0, p.S = at + T, p.keep = 0, p.rskip = f.e + rows;
    } else {
        p.P = f.ipo, p.S = H + T, p.keep = f.e, p.rskip = f.e + rows > nh ? nh : f.e + rows;
        p.patch = f.e != 0 && tun_has_etype(f.prev) && f.ipo >= 2u ? 1u : 0u;
        p.et6 = p.in6;
    }
    p.st = PKT_TUND_OK;
}

// ---- out_chain of an OK packet: row r < tun_out_rows(p) of the output is (type, offset).  src_ty / src_of: the
// source's row j, as the caller fetches it.
PKT_HD uint32_t tun_out_rows(const TunPlan& p) { return p.keep + p.add + (p.nh - p.rskip); }

// row r is an added outer row (then ty / of are set) or the source's row *j with its offset moved by *delta
PKT_HD bool tun_out_row(const TunPlan& p, const TunEnt* e, uint32_t r, uint32_t& ty, uint32_t& of, uint32_t& j, int32_t& delta) {
    if (r < p.keep) {
        j = r, delta = 0;
        return false;
    }
    if (r < p.keep + p.add) {  // encap's outer rows
        const uint32_t a = r - p.keep, kind = tun_kind(*e), H = tun_ipver(*e) == 4 ? 20u : 40u;
        const uint32_t ipt = tun_ipver(*e) == 4 ? PKT_HDR_IPV4 : PKT_HDR_IPV6;
        if (kind == PKT_TUN_VXLAN) {
            ty = a == 0 ? (uint32_t)PKT_HDR_ETHER : a == 1 ? ipt : a == 2 ? (uint32_t)PKT_HDR_UDP : (uint32_t)PKT_HDR_VXLAN;
            of = a == 0 ? 0u : a == 1 ? 14u : a == 2 ? 14u + H : 22u + H;
        } else {
            ty = a == 0 ? ipt : a == 1 ? (uint32_t)PKT_HDR_GRE : (uint32_t)PKT_HDR_GRE_KEY;
            of = p.P + (a == 0 ? 0u : a == 1 ? H : H + 4u);
        }
        return true;
    }
    j = p.rskip + (r - p.keep - p.add);
    delta = (int32_t)p.hl - (int32_t)p.S;
    return false;
}

// ---- the refusals the entry points share: the text (after "pkt_tunnel_encap_batch: " / "pkt_tunnel_decap_batch: "),
// or nullptr; the output contract's own last.  device: the _batch entries on `device_id`; else the host twins.
inline const char* tun_call_error(const pkt_batch_t* b, const pkt_chain_t* chain, uint32_t which_ip, uint32_t flags,
                                  const pkt_tunnel* tun, const uint32_t* a32, const uint32_t* b32, const uint8_t* dst,
                                  uint64_t out_cap, const uint64_t* out_off, const uint32_t* out_len, const uint64_t* hits,
                                  bool device, int device_id) {
    if (!b || !chain) return "null argument";
    if (!tun) return "null tunnel table";
    if (device && !tun->device) return "the tunnel table is a host handle";
    if (!device && tun->device) return "the tunnel table is a device handle";
    if (device && tun->device_id != device_id) return "the tunnel table was created on another device";
    if (b->n >= (1ull << 32)) return "n >= 2^32";
    if (flags & ~kTunCallFlags) return "unknown flag bits";
    if (which_ip >= PKT_MAX_HDRS && which_ip != PKT_FLOW_LAST) return "which_ip is neither below 16 nor PKT_FLOW_LAST";
    if (((uintptr_t)a32 | (uintptr_t)b32) & 3) return "a uint32_t array is not 4-byte aligned";
    return out_call_error(b, chain, flags & PKT_TUN_NO_WRITE, "null dst, out_off or out_len without PKT_TUN_NO_WRITE", dst,
                          out_cap, out_off, out_len, hits, device);
}
