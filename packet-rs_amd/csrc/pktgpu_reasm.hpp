// pktgpu_reasm.hpp — what the two halves of pkt_reasm_* share: the per-packet classification (the IP entry's search is
// pkt_frag_batch's, frag_find_step; then the status each step of include/pktgpu.h gives), a member's key and its hash,
// the joined datagram's rebuilt IPv4 header with its incrementally updated checksum, the verdict from a datagram's
// five words, and the argument validation.  pktgpu_reasm.hip holds pkt_reasm_batch / _async / _result and the kernels;
// pktgpu_host.cpp holds pkt_reasm_host (it compiles under g++ alone), which sorts the members and walks each datagram,
// so that it checks the kernels' verdict rule and not only their arithmetic.
#pragma once
#include <cstdint>

#include "pktgpu_batch.hpp"
#include "pktgpu_flow.hpp"
#include "pktgpu_frag.hpp"
#include "pktgpu_outbatch.hpp"

constexpr uint32_t kReasmFlags = PKT_REASM_ONLY_JOINED | PKT_REASM_NO_WRITE;

// A source packet as the later steps see it, none of it read from the packet again except the s = 0 member's header.
struct ReasmRec {
    uint32_t st;        // pkt_reasm_status_t; a member carries PKT_REASM_PENDING until its datagram's verdict
    uint32_t member;    // 1: step 6 was reached
    uint32_t src, dst;  // the key: bytes 12..15 and 16..19 as little-endian dwords,
    uint32_t idp;       //   bytes 4..5 (as they lie) | protocol << 16
    uint32_t mf;        // more-fragments
    uint32_t s, len;    // the fragment's start and payload bytes; e = s + len
    uint32_t ipo;       // the IP header's offset
    uint32_t nh;        // rows of this packet's chain an output takes: min(n_hdrs, 16) for WHOLE, e + 1 for a member
    uint32_t plen;      // the packet's length under the batch clamp (a WHOLE output's length)
};

// step 2's outcome: PKT_REASM_NO_IP / _SPAN, or PKT_REASM_WHOLE for "go on with reasm_classify"
PKT_HD uint32_t reasm_find_status(const FragFind& f, uint32_t len) {
    const uint32_t fs = frag_find_status(f, len);
    return fs == PKT_FRAG_NO_IP ? PKT_REASM_NO_IP : fs == PKT_FRAG_SPAN ? PKT_REASM_SPAN : PKT_REASM_WHOLE;
}

// steps 3 to 6 for a packet whose IP entry (f, 20 / 40 bytes inside the packet's plen bytes) is found: h[k] = the
// entry's bytes 4k .. 4k + 3 as a little-endian dword (h[3], h[4] are read for an IPv4 entry only).
PKT_HD void reasm_classify(ReasmRec& r, const FragFind& f, uint32_t nh, const uint32_t h[5]) {
    r.ipo = f.ipo;
    r.nh = nh;
    const uint32_t w = fwd_be16(h[1] >> 16);
    if (f.ipt != PKT_HDR_IPV4 || (w & 0x3FFFu) == 0) {
        r.st = PKT_REASM_WHOLE;
        return;
    }
    const uint32_t L = fwd_be16(h[0] >> 16);
    r.mf = w >> 13 & 1u;
    if ((h[0] & 0xFFu) != 0x45u || L <= 20u || (r.mf && ((L - 20u) & 7u))) {
        r.st = PKT_REASM_BAD_HDR;
        return;
    }
    if (f.ipo + L > r.plen) {
        r.st = PKT_REASM_TRUNC;
        return;
    }
    r.st = PKT_REASM_PENDING;
    r.member = 1;
    r.nh = f.e + 1u;
    r.s = 8u * (w & 0x1FFFu);
    r.len = L - 20u;
    r.src = h[3], r.dst = h[4];
    r.idp = (h[1] & 0xFFFFu) | (h[2] >> 8 & 0xFFu) << 16;
}

PKT_HD bool reasm_same_key(uint32_t src, uint32_t dst, uint32_t idp, uint32_t src2, uint32_t dst2, uint32_t idp2) {
    return src == src2 && dst == dst2 && idp == idp2;
}
PKT_HD uint64_t reasm_key_hash(uint32_t src, uint32_t dst, uint32_t idp) {
    return flow_mix64(flow_mix64((uint64_t)src | (uint64_t)dst << 32) ^ idp);
}

// A datagram's verdict from what its members left: finals = members with MF clear, has0 = a member with s = 0 exists,
// hole = some MF-set member's end is no member's start, sum = the members' payload bytes, E = the (single) final
// member's end.  With len > 0 for every member this is the tiling of include/pktgpu.h (DESIGN.md §4 has the argument).
PKT_HD uint32_t reasm_verdict(uint32_t finals, bool has0, bool hole, uint64_t sum, uint32_t E) {
    if (finals != 1u || !has0 || hole || sum != E) return PKT_REASM_PENDING;
    return 20u + E > 65535u ? PKT_REASM_TOO_BIG : PKT_REASM_JOINED;
}

// The joined datagram's IPv4 bytes 0..11 from the s = 0 member's (h, little-endian dwords): the total length 20 + E,
// the flags word w0 & 0xC000, and the checksum updated over those two words as frag_header does.
PKT_HD void reasm_header(uint32_t E, const uint32_t h[3], uint32_t o[3]) {
    const uint32_t L = fwd_be16(h[0] >> 16), w = fwd_be16(h[1] >> 16), hc = fwd_be16(h[2] >> 16);
    const uint32_t L2 = 20u + E, w2 = w & 0xC000u;
    uint32_t s = (~hc & 0xFFFFu) + (~L & 0xFFFFu) + L2 + (~w & 0xFFFFu) + w2;
    s = (s & 0xFFFFu) + (s >> 16);
    s = (s & 0xFFFFu) + (s >> 16);
    const uint32_t hc2 = ~s & 0xFFFFu;
    o[0] = (h[0] & 0xFFFFu) | fwd_be16(L2) << 16;
    o[1] = (h[1] & 0xFFFFu) | fwd_be16(w2) << 16;
    o[2] = (h[2] & 0xFFFFu) | fwd_be16(hc2) << 16;
}

// ---- the refusals both entry points share: the text (after "pkt_reasm_batch: "), or nullptr; the contract's own last.
// device: pkt_reasm_batch (the slab's alignment rule); else pkt_reasm_host.
inline const char* reasm_call_error(const pkt_batch_t* b, const pkt_chain_t* chain, uint32_t which_ip, uint32_t flags,
                                    const uint8_t* dst, uint64_t out_cap, const uint64_t* out_off, const uint32_t* out_len,
                                    const uint64_t* hits, bool device) {
    if (!b || !chain) return "null argument";
    if (b->n >= (1ull << 32)) return "n >= 2^32";
    if (flags & ~kReasmFlags) return "unknown flag bits";
    if (which_ip >= PKT_MAX_HDRS && which_ip != PKT_FLOW_LAST) return "which_ip is neither below 16 nor PKT_FLOW_LAST";
    return out_call_error(b, chain, flags & PKT_REASM_NO_WRITE, "null dst, out_off or out_len without PKT_REASM_NO_WRITE", dst,
                          out_cap, out_off, out_len, hits, device);
}
