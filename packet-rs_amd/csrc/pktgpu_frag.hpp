// pktgpu_frag.hpp — what the two halves of pkt_frag_* share: the per-packet decision (the IP entry's search is
// pkt_fwd_batch's, fwd_find_step; then the status each step of include/pktgpu.h gives), a packet's output count and
// rounded bytes in closed form, the fragment's rebuilt IPv4 header with its incrementally updated checksum, and the
// argument validation.  pktgpu_frag.hip holds pkt_frag_batch / _async / _result and the kernels; pktgpu_host.cpp holds
// pkt_frag_host's sequential loops (it compiles under g++ alone).  Both call the same inline code, the
// pktgpu_fwd.hpp pattern, so the CPU tests cover the whole decision.
#pragma once
#include <cstdint>

#include "pktgpu_batch.hpp"
#include "pktgpu_fwd.hpp"
#include "pktgpu_outbatch.hpp"

constexpr uint32_t kFragFlags = PKT_FRAG_ONLY_SPLIT | PKT_FRAG_NO_WRITE;

// A source packet's plan: what the emit and copy steps need, none of it read from the packet again except the header.
struct FragPlan {
    uint32_t st;     // pkt_frag_status_t
    uint32_t nout;   // outputs: 1 (FITS, 0 with ONLY_SPLIT), k (SPLIT), else 0
    uint32_t ipo;    // SPLIT: the IP header's offset
    uint32_t per;    // SPLIT: payload bytes of every fragment but the last, a multiple of 8
    uint32_t pay;    // SPLIT: P = L - 20
    uint32_t len;    // the packet's length under the batch clamp (a FITS output's length)
    uint32_t nh;     // rows of the source's chain an output takes: min(n_hdrs, 16) for FITS, e + 1 for SPLIT
};

// step 2: the IP entry (pkt_flow_key_batch's search, as fwd_find_step makes it) and its index in the list.  The
// caller feeds the list's entries in order; an entry that is not IP is ignored, so its offset need not be read.
struct FragFind {
    uint32_t ipt = 0, ipo = 0, e = 0;  // the chosen IP entry's type (0: none), offset and index
    uint32_t seen = 0;                 // IP entries so far
};

PKT_HD void frag_find_step(FragFind& f, uint32_t which, uint32_t j, uint32_t ty, uint32_t of) {
    const bool ip = fwd_is_ip(ty);
    const bool take = ip && (which == PKT_FLOW_LAST || f.seen == which);
    f.ipt = take ? ty : f.ipt;
    f.ipo = take ? of : f.ipo;
    f.e = take ? j : f.e;
    f.seen += ip ? 1u : 0u;
}

// PKT_FRAG_NO_IP / _SPAN, or PKT_FRAG_FITS for "go on with frag_decide"
PKT_HD uint32_t frag_find_status(const FragFind& f, uint32_t len) {
    if (!f.ipt) return PKT_FRAG_NO_IP;
    if (f.ipo + (f.ipt == PKT_HDR_IPV4 ? 20u : 40u) > len) return PKT_FRAG_SPAN;
    return PKT_FRAG_FITS;
}

// what the decision leaves for the outputs: a FITS packet's single output (none with ONLY_SPLIT) takes the whole
// list, a fragment the rows up to the IP entry
PKT_HD void frag_finish(FragPlan& p, const FragFind& f, uint32_t nh, uint32_t flags) {
    if (p.st == PKT_FRAG_FITS) {
        p.nout = flags & PKT_FRAG_ONLY_SPLIT ? 0u : 1u;
        p.nh = nh;
    } else if (p.st == PKT_FRAG_SPLIT) {
        p.nh = f.e + 1u;
    }
}

// steps 3 to 10 for a packet whose IP entry (type ipt at ipo, 20 / 40 bytes inside the packet's len bytes) is found:
// h[k] = the entry's bytes 4k .. 4k + 3 as a little-endian dword, m the mtu.  st and, for SPLIT, nout / per / pay.
PKT_HD void frag_decide(FragPlan& p, uint32_t ipt, uint32_t ipo, uint32_t len, const uint32_t h[3], uint32_t m) {
    const bool v4 = ipt == PKT_HDR_IPV4;
    const uint32_t L = fwd_ip_fields(h, v4).l3len;
    p.ipo = ipo;
    if (m == 0 || L <= m) {
        p.st = PKT_FRAG_FITS;
        return;
    }
    if (!v4) {
        p.st = PKT_FRAG_IPV6;
        return;
    }
    if ((h[0] & 0xFFu) != 0x45u || L < 20u) {
        p.st = PKT_FRAG_BAD_HDR;
        return;
    }
    if (ipo + L > len) {
        p.st = PKT_FRAG_TRUNC;
        return;
    }
    if (h[1] >> 16 & 0x40u) {  // byte 6
        p.st = PKT_FRAG_DF;
        return;
    }
    if (m < 28u) {
        p.st = PKT_FRAG_MTU;
        return;
    }
    const uint32_t per = (m - 20u) & ~7u, P = L - 20u, k = (P + per - 1u) / per;
    const uint32_t o = fwd_be16(h[1] >> 16) & 0x1FFFu;
    if (o + (k - 1u) * per / 8u > 0x1FFFu) {
        p.st = PKT_FRAG_BAD_HDR;
        return;
    }
    p.st = PKT_FRAG_SPLIT;
    p.nout = k;
    p.per = per;
    p.pay = P;
}

// output j's length (j < nout) and the rounded bytes of the outputs before it
PKT_HD uint32_t frag_out_len(const FragPlan& p, uint32_t j) {
    if (p.st != PKT_FRAG_SPLIT) return p.len;
    return p.ipo + 20u + (j + 1u < p.nout ? p.per : p.pay - (p.nout - 1u) * p.per);
}
PKT_HD uint64_t frag_out_rel(const FragPlan& p, uint32_t j) {
    return p.st == PKT_FRAG_SPLIT ? (uint64_t)j * out_round16(p.ipo + 20u + p.per) : 0u;
}
// the rounded bytes of all the packet's outputs (at most 8190 * 65536: it fits 32 bits, kept in 64)
PKT_HD uint64_t frag_out_bytes(const FragPlan& p) {
    if (!p.nout) return 0;
    return frag_out_rel(p, p.nout - 1u) + out_round16(frag_out_len(p, p.nout - 1u));
}

// Fragment j's IPv4 bytes 0..11 from the source's (h, little-endian dwords as above): the total length, the flags and
// offset word, and the checksum updated over those two words by RFC 1624 eq. 3 (nothing is summed again).
PKT_HD void frag_header(const FragPlan& p, uint32_t j, const uint32_t h[3], uint32_t o[3]) {
    const uint32_t L = fwd_be16(h[0] >> 16), w = fwd_be16(h[1] >> 16), hc = fwd_be16(h[2] >> 16);
    const uint32_t L2 = frag_out_len(p, j) - p.ipo;
    const uint32_t mf = j + 1u < p.nout ? 0x2000u : w & 0x2000u;
    const uint32_t w2 = (w & 0xC000u) | mf | ((w & 0x1FFFu) + j * p.per / 8u);
    uint32_t s = (~hc & 0xFFFFu) + (~L & 0xFFFFu) + L2 + (~w & 0xFFFFu) + w2;
    s = (s & 0xFFFFu) + (s >> 16);
    s = (s & 0xFFFFu) + (s >> 16);
    const uint32_t hc2 = ~s & 0xFFFFu;
    o[0] = (h[0] & 0xFFFFu) | fwd_be16(L2) << 16;
    o[1] = (h[1] & 0xFFFFu) | fwd_be16(w2) << 16;
    o[2] = (h[2] & 0xFFFFu) | fwd_be16(hc2) << 16;
}

// ---- the refusals both entry points share: the text (after "pkt_frag_batch: "), or nullptr; the contract's own last.
// device: pkt_frag_batch (the slab's alignment rule); else pkt_frag_host.
inline const char* frag_call_error(const pkt_batch_t* b, const pkt_chain_t* chain, uint32_t which_ip, uint32_t flags,
                                   const uint16_t* mtu, uint32_t mtu_all, const uint8_t* dst, uint64_t out_cap,
                                   const uint64_t* out_off, const uint32_t* out_len, const uint64_t* hits, bool device) {
    if (!b || !chain) return "null argument";
    if (b->n >= (1ull << 32)) return "n >= 2^32";
    if (flags & ~kFragFlags) return "unknown flag bits";
    if (which_ip >= PKT_MAX_HDRS && which_ip != PKT_FLOW_LAST) return "which_ip is neither below 16 nor PKT_FLOW_LAST";
    if (mtu_all > 65535u) return "mtu_all above 65535";
    if ((uintptr_t)mtu & 1) return "mtu not 2-byte aligned";
    return out_call_error(b, chain, flags & PKT_FRAG_NO_WRITE, "null dst, out_off or out_len without PKT_FRAG_NO_WRITE", dst,
                          out_cap, out_off, out_len, hits, device);
}
