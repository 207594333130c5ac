// pktgpu_nat.hpp — what the two halves of pkt_nat_* share: the handle behind pkt_nat_t, the per-packet decision
// (nat_classify), the key packing, the entry / port arithmetic, the inbound lookup, the free map's circular
// segments and the j-th free entry in them (nat_select), the RFC 1624 update with the narrow stores (nat_rewrite),
// the create validation and the argument refusals.  pktgpu_host.cpp holds the public pkt_nat_* calls and the host
// handle, which IS the sequential model of include/pktgpu.h (it compiles under g++ alone); pktgpu_nat.hip holds
// pkt_nat_create and the device handle's calls, which the handle reaches through `ops`.  Both call the same inline
// code, so the CPU tests cover the decision and the arithmetic.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "pktgpu_batch.hpp"
#include "pktgpu_flow.hpp"

static_assert(sizeof(pkt_nat_static_t) == 16 && sizeof(pkt_nat_record_t) == 20, "nat ABI structs");

constexpr uint32_t kNatFlags = PKT_NAT_NO_WRITE;
constexpr uint64_t kNatMinSlots = 64, kNatMaxSlots = 1ull << 26;
constexpr uint32_t kNatBlk = 1024;      // pool entries per block of the free map
constexpr uint32_t kNatBlkWords = 32;   // its 32-bit words
constexpr uint32_t kNatNoSlot = 0xFFFFFFFFu;

// ---- protocol indexes and the 64-bit endpoint word: (p + 1) << 48 | addr << 16 | port, never 0
PKT_HD uint32_t nat_proto_index(uint32_t proto) { return proto == 6 ? 0u : proto == 17 ? 1u : proto == 1 ? 2u : 3u; }
PKT_HD uint32_t nat_proto_of(uint32_t p) { return p == 0 ? 6u : p == 1 ? 17u : 1u; }
PKT_HD uint64_t nat_key(uint32_t p, uint32_t addr, uint32_t port) {
    return (uint64_t)(p + 1u) << 48 | (uint64_t)addr << 16 | port;
}
PKT_HD uint32_t nat_key_p(uint64_t k) { return (uint32_t)(k >> 48) - 1u; }
PKT_HD uint32_t nat_key_addr(uint64_t k) { return (uint32_t)(k >> 16); }
PKT_HD uint32_t nat_key_port(uint64_t k) { return (uint32_t)k & 0xFFFFu; }
PKT_HD uint64_t nat_home(uint64_t key, uint64_t slots) { return flow_mix64(key) & (slots - 1); }

// What the kernels and the host loop read and write: device pointers for a device handle, host pointers for a host
// handle.  Addresses are host-order values of the wire bytes (10.0.0.1 = 0x0A000001).
struct NatView {
    // the forward index: key 0 = empty; val = p * E + e, PKT_NAT_STATIC | index, or PKT_NAT_NONE (claimed in this
    // call, or EXHAUSTED earlier: no session); first = the lowest index of the call's packets that want to create
    // the slot's session (~0 between calls)
    uint64_t* fkey;
    uint32_t* fval;
    uint32_t* ffirst;
    uint64_t slots;
    uint64_t* rev;     // [3 * E]: the inside endpoint's word, 0 = free
    uint32_t* seen;    // [3 * E]: last_seen
    uint32_t* used;    // [3 * W]: the free map, bit e % 32 of word p * W + e / 32 set = mapped
    uint32_t* cursor;  // [3]
    const uint32_t* pool;         // [naddr], in pool order
    const uint64_t* pool_sorted;  // [naddr]: addr << 32 | pool index, ascending
    const uint64_t* st_in;        // [nstatic]: the statics' inside endpoint words, in array order
    const uint64_t* st_out;       // [nstatic]: their outside endpoint words
    const uint64_t* sin_key;      // [nstatic]: the outside endpoint words, ascending
    const uint32_t* sin_idx;      // [nstatic]: the static each belongs to
    uint32_t naddr, nports, port_lo, nstatic;
    uint32_t E, W, nblk;          // entries per protocol; words (nblk * 32) and blocks of its free map
};

// ---- steps 2 to 5: the status so far (PKT_NAT_OK: a translatable packet), the protocol index, the offsets of the IP
// and the L4 header in the packet and the endpoint word this direction looks up (OUT: source, IN: destination)
struct NatPkt {
    uint32_t st, p, ipo, l4o;
    uint64_t key;
};

PKT_HD uint32_t nat_rd16(const uint8_t* q) { return (uint32_t)q[0] << 8 | q[1]; }
PKT_HD uint32_t nat_rd32(const uint8_t* q) {
    return (uint32_t)q[0] << 24 | (uint32_t)q[1] << 16 | (uint32_t)q[2] << 8 | q[3];
}

// pkt: the packet's first byte, len: its length under the batch clamp; the chain columns are slot-major [.][n]
PKT_HD NatPkt nat_classify(const uint8_t* pkt, uint32_t len, const uint8_t* n_hdrs, const uint8_t* hdr_type,
                           const uint16_t* hdr_off, uint64_t n, uint64_t i, uint32_t which, uint32_t dir) {
    NatPkt r{PKT_NAT_NO_IP, 0, 0, 0, 0};
    uint32_t nh = n_hdrs[i];
    nh = nh > PKT_MAX_HDRS ? PKT_MAX_HDRS : nh;
    uint32_t ipt = 0, ipo = 0, nxt = 0, nxo = 0, seen = 0;
    bool pend = false;  // the entry before this one was taken
    for (uint32_t j = 0; j < nh; j++) {
        const uint32_t t = hdr_type[(uint64_t)j * n + i];
        if (pend) {
            nxt = t;
            nxo = hdr_off[(uint64_t)j * n + i];
            pend = false;
        }
        if (t == PKT_HDR_IPV4 || t == PKT_HDR_IPV6) {
            if (which == PKT_FLOW_LAST || seen == which) {
                ipt = t;
                ipo = hdr_off[(uint64_t)j * n + i];
                nxt = nxo = 0;
                pend = true;
            }
            seen++;
        }
    }
    if (!ipt) return r;
    r.st = PKT_NAT_IPV6;
    if (ipt == PKT_HDR_IPV6) return r;
    r.st = PKT_NAT_SPAN;
    if (ipo + 20u > len) return r;
    const uint8_t* ip = pkt + ipo;
    r.st = PKT_NAT_BAD_HDR;
    if (ip[0] != 0x45) return r;
    r.st = PKT_NAT_FRAGMENT;
    if (nat_rd16(ip + 6) & 0x3FFFu) return r;
    r.st = PKT_NAT_NO_L4;
    const uint32_t p = nat_proto_index(ip[9]);
    if (p > 2) return r;
    if (nxt != (p == 0 ? (uint32_t)PKT_HDR_TCP : p == 1 ? (uint32_t)PKT_HDR_UDP : (uint32_t)PKT_HDR_ICMP)) return r;
    if (nxo + (p == 0 ? 20u : 8u) > len) {
        r.st = PKT_NAT_SPAN;
        return r;
    }
    const uint8_t* l4 = pkt + nxo;
    if (p == 2 && l4[0] != 8 && l4[0] != 0) return r;
    const uint32_t port = nat_rd16(l4 + (p == 2 ? 4u : dir ? 2u : 0u));
    const uint32_t addr = nat_rd32(ip + (dir ? 16u : 12u));
    r.st = PKT_NAT_OK;
    r.p = p;
    r.ipo = ipo;
    r.l4o = nxo;
    r.key = nat_key(p, addr, port);
    return r;
}

// ---- entry / port arithmetic
PKT_HD uint64_t nat_entry_out(const NatView& V, uint32_t p, uint32_t e) {  // a dynamic entry's outside endpoint word
    return nat_key(p, V.pool[e / V.nports], V.port_lo + e % V.nports);
}

// step 7: the entry an inbound endpoint word names (PKT_NAT_STATIC | index, p * E + e, or PKT_NAT_NONE) and its status
PKT_HD uint32_t nat_in_find(const NatView& V, uint64_t key, uint32_t& st) {
    uint32_t lo = 0, hi = V.nstatic;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (V.sin_key[mid] < key) lo = mid + 1; else hi = mid;
    }
    if (lo < V.nstatic && V.sin_key[lo] == key) {
        st = PKT_NAT_OK;
        return PKT_NAT_STATIC | V.sin_idx[lo];
    }
    const uint32_t p = nat_key_p(key), addr = nat_key_addr(key), port = nat_key_port(key);
    lo = 0, hi = V.naddr;
    const uint64_t want = (uint64_t)addr << 32;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (V.pool_sorted[mid] < want) lo = mid + 1; else hi = mid;
    }
    if (lo < V.naddr && (uint32_t)(V.pool_sorted[lo] >> 32) == addr && port >= V.port_lo && port - V.port_lo < V.nports) {
        const uint32_t ent = p * V.E + (uint32_t)V.pool_sorted[lo] * V.nports + (port - V.port_lo);
        const bool mapped = V.rev[ent] != 0;
        st = mapped ? PKT_NAT_OK : PKT_NAT_NO_SESSION;
        return mapped ? ent : PKT_NAT_NONE;
    }
    st = PKT_NAT_NOT_OURS;
    return PKT_NAT_NONE;
}

// the endpoint word an OK packet's address and port are rewritten to: dir OUT: the entry's outside endpoint; IN: its
// inside endpoint
PKT_HD uint64_t nat_target(const NatView& V, uint32_t entry, uint32_t p, uint32_t dir) {
    if (entry & PKT_NAT_STATIC) return dir ? V.st_in[entry & ~PKT_NAT_STATIC] : V.st_out[entry & ~PKT_NAT_STATIC];
    return dir ? V.rev[entry] : nat_entry_out(V, p, entry - p * V.E);
}

// ---- the free map in circular order from the cursor c: nblk + 1 segments.  Segment 0 is the cursor's block from c
// on, segments 1 .. nblk - 1 the blocks behind it (wrapping), segment nblk the cursor's block below c.
struct NatSeg {
    uint32_t lo, hi;  // entries [lo, hi)
};
PKT_HD NatSeg nat_segment(uint32_t k, uint32_t c, uint32_t E, uint32_t nblk) {
    const uint32_t bc = c / kNatBlk;
    const uint32_t b = (bc + k) % nblk;
    uint32_t lo = b * kNatBlk, hi = lo + kNatBlk;
    hi = hi > E ? E : hi;
    if (k == 0) lo = c;
    if (k == nblk) hi = c;
    return NatSeg{lo, hi};
}
// the free entries of word w (entries [32 w, 32 w + 32)) that lie in [lo, hi), as bits
PKT_HD uint32_t nat_free_bits(uint32_t used, uint32_t w, uint32_t lo, uint32_t hi) {
    const uint32_t base = w * 32u;
    if (hi <= base || lo >= base + 32u) return 0u;
    uint32_t m = ~0u;
    if (lo > base) m &= ~0u << (lo - base);
    if (hi < base + 32u) m &= ~(~0u << (hi - base));
    return ~used & m;
}
PKT_HD uint32_t nat_popc(uint32_t x) {
#ifdef __HIP_DEVICE_COMPILE__
    return (uint32_t)__popc(x);
#else
    return (uint32_t)__builtin_popcount(x);
#endif
}
PKT_HD uint32_t nat_segment_free(const uint32_t* used, uint32_t k, uint32_t c, uint32_t E, uint32_t nblk) {
    const NatSeg s = nat_segment(k, c, E, nblk);
    uint32_t cnt = 0;
    for (uint32_t w = s.lo / 32u; w * 32u < s.hi; w++) cnt += nat_popc(nat_free_bits(used[w], w, s.lo, s.hi));
    return cnt;
}
// The j-th free entry (from 0) in circular order from c.  pre[0 .. nblk + 1]: the exclusive prefix of the segments'
// free counts, pre[nblk + 1] the total; j < the total.  `used` is one protocol's map.
PKT_HD uint32_t nat_select(const uint32_t* used, const uint32_t* pre, uint32_t j, uint32_t c, uint32_t E, uint32_t nblk) {
    uint32_t lo = 0, hi = nblk + 1u;  // the last segment k with pre[k] <= j
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (pre[mid] <= j) lo = mid; else hi = mid;
    }
    const NatSeg s = nat_segment(lo, c, E, nblk);
    uint32_t r = j - pre[lo];
    for (uint32_t w = s.lo / 32u; w * 32u < s.hi; w++) {
        uint32_t f = nat_free_bits(used[w], w, s.lo, s.hi);
        const uint32_t cnt = nat_popc(f);
        if (r >= cnt) {
            r -= cnt;
            continue;
        }
        for (; r; r--) f &= f - 1u;
        uint32_t bit = 0;
        while (!(f >> bit & 1u)) bit++;
        return w * 32u + bit;
    }
    return E;  // not reached for j below the total
}

// ---- RFC 1624 eq. 3: hc the stored checksum, oldsum = sum(~m_k & 0xFFFF), newsum = sum(m'_k), at most three words each
PKT_HD uint32_t nat_csum(uint32_t hc, uint32_t oldsum, uint32_t newsum) {
    uint32_t s = (~hc & 0xFFFFu) + oldsum + newsum;
    s = (s & 0xFFFFu) + (s >> 16);
    s = (s & 0xFFFFu) + (s >> 16);
    return ~s & 0xFFFFu;
}

// the writes of an OK packet: ip / l4 = the headers' first bytes, to = the endpoint word written (nat_target).  Byte
// stores, so any alignment; ten bytes in all.
PKT_HD void nat_rewrite(uint8_t* ip, uint8_t* l4, uint32_t p, uint32_t dir, uint64_t to) {
    const uint32_t na = nat_key_addr(to), np = nat_key_port(to);
    uint8_t* a = ip + (dir ? 16 : 12);
    uint8_t* pt = l4 + (p == 2 ? 4 : dir ? 2 : 0);
    uint8_t* ck = l4 + (p == 0 ? 16 : p == 1 ? 6 : 2);
    const uint32_t oa = nat_rd32(a), op = nat_rd16(pt);
    const uint32_t osum = (~(oa >> 16) & 0xFFFFu) + (~oa & 0xFFFFu), nsum = (na >> 16) + (na & 0xFFFFu);
    const uint32_t hc = nat_csum(nat_rd16(ip + 10), osum, nsum);
    const uint32_t lc0 = nat_rd16(ck);
    uint32_t lc;
    if (p == 2) {
        lc = nat_csum(lc0, ~op & 0xFFFFu, np);
    } else {
        lc = nat_csum(lc0, osum + (~op & 0xFFFFu), nsum + np);
        if (p == 1) lc = lc0 == 0 ? 0u : lc == 0 ? 0xFFFFu : lc;
    }
    a[0] = (uint8_t)(na >> 24), a[1] = (uint8_t)(na >> 16), a[2] = (uint8_t)(na >> 8), a[3] = (uint8_t)na;
    ip[10] = (uint8_t)(hc >> 8), ip[11] = (uint8_t)hc;
    pt[0] = (uint8_t)(np >> 8), pt[1] = (uint8_t)np;
    ck[0] = (uint8_t)(lc >> 8), ck[1] = (uint8_t)lc;
}

// ---- create: the validated configuration and the small tables both handles read
struct NatImage {
    uint32_t naddr = 0, nports = 0, port_lo = 0, nstatic = 0, E = 0, W = 0, nblk = 0;
    uint64_t slots = 0;
    std::vector<uint32_t> pool;
    std::vector<uint64_t> pool_sorted, st_in, st_out, sin_key;
    std::vector<uint32_t> sin_idx;
};

// nullptr and `img` filled, or the refusal's text (after "pkt_nat_create: " / "pkt_nat_create_host: ")
inline const char* nat_create_error(const uint8_t* pool, uint32_t naddr, uint32_t port_lo, uint32_t port_hi, uint64_t slots,
                                    const pkt_nat_static_t* statics, uint32_t nstatic, NatImage& img) {
    if (naddr < 1 || naddr > PKT_NAT_MAX_ADDR) return "naddr not in 1..64";
    if (!pool) return "null pool";
    if (port_lo < 1 || port_lo > port_hi || port_hi > 65535) return "ports not 1 <= port_lo <= port_hi <= 65535";
    if (slots < kNatMinSlots || slots > kNatMaxSlots || (slots & (slots - 1))) return "slots not a power of two in 64..2^26";
    if (nstatic > PKT_NAT_MAX_STATIC) return "nstatic above PKT_NAT_MAX_STATIC";
    if (nstatic && !statics) return "null statics";
    if (nstatic > slots / 2) return "nstatic above slots / 2";
    img.naddr = naddr;
    img.port_lo = port_lo;
    img.nports = port_hi - port_lo + 1;
    img.nstatic = nstatic;
    img.slots = slots;
    img.E = naddr * img.nports;
    img.nblk = (img.E + kNatBlk - 1) / kNatBlk;
    img.W = img.nblk * kNatBlkWords;
    img.pool.resize(naddr);
    img.pool_sorted.resize(naddr);
    for (uint32_t a = 0; a < naddr; a++) {
        img.pool[a] = nat_rd32(pool + 4 * a);
        img.pool_sorted[a] = (uint64_t)img.pool[a] << 32 | a;
    }
    std::sort(img.pool_sorted.begin(), img.pool_sorted.end());
    for (uint32_t a = 1; a < naddr; a++)
        if (img.pool_sorted[a] >> 32 == img.pool_sorted[a - 1] >> 32) return "duplicate pool address";
    img.st_in.resize(nstatic);
    img.st_out.resize(nstatic);
    std::vector<std::pair<uint64_t, uint32_t>> ord(nstatic);
    for (uint32_t k = 0; k < nstatic; k++) {
        const pkt_nat_static_t& s = statics[k];
        const uint32_t p = nat_proto_index(s.proto);
        if (p > 2) return "a static's proto is not 6, 17 or 1";
        if (s.zero[0] | s.zero[1] | s.zero[2]) return "non-zero `zero`";
        img.st_in[k] = nat_key(p, nat_rd32(s.in_addr), s.in_port);
        img.st_out[k] = nat_key(p, nat_rd32(s.out_addr), s.out_port);
        ord[k] = {img.st_out[k], k};
        if (s.out_port >= port_lo && s.out_port <= port_hi)
            for (uint32_t a = 0; a < naddr; a++)
                if (img.pool[a] == nat_rd32(s.out_addr)) return "a static's outside endpoint is a dynamic pool entry";
    }
    std::vector<uint64_t> ins(img.st_in);
    std::sort(ins.begin(), ins.end());
    for (uint32_t k = 1; k < nstatic; k++)
        if (ins[k] == ins[k - 1]) return "duplicate inside endpoint";
    std::sort(ord.begin(), ord.end());
    img.sin_key.resize(nstatic);
    img.sin_idx.resize(nstatic);
    for (uint32_t k = 0; k < nstatic; k++) {
        if (k && ord[k].first == ord[k - 1].first) return "duplicate outside endpoint";
        img.sin_key[k] = ord[k].first;
        img.sin_idx[k] = ord[k].second;
    }
    return nullptr;
}

// the refusals of pkt_nat_batch on both handles (pkt_fwd_batch's rules): the text after "pkt_nat_batch: ", or nullptr.
// n == 0 is the caller's to take between the two.
inline const char* nat_call_error(const pkt_batch_t* b, const pkt_chain_t* chain, uint32_t which_ip, uint32_t flags,
                                  uint32_t dir_all, const uint8_t* dir, const uint64_t* hits, const uint64_t* bytes) {
    if (!b || !chain) return "null argument";
    if (b->n >= (1ull << 32)) return "n >= 2^32";
    if (flags & ~kNatFlags) return "unknown flag bits";
    if (which_ip >= PKT_MAX_HDRS && which_ip != PKT_FLOW_LAST) return "which_ip is neither below 16 nor PKT_FLOW_LAST";
    if (!dir && dir_all >= 2) return "dir_all is neither PKT_NAT_OUT nor PKT_NAT_IN";
    if (((uintptr_t)hits | (uintptr_t)bytes) & 7) return "hits / bytes not 8-byte aligned";
    return nullptr;
}
inline const char* nat_batch_error(const pkt_batch_t* b, const pkt_chain_t* chain, bool device) {
    if (!chain->n_hdrs || !chain->hdr_type || !chain->hdr_off) return "null chain column";
    const char* msg = device ? batch_slab16_error(b) : batch_null_slab(b) ? "null slab" : nullptr;
    return msg ? msg : batch_index_error(b);
}

// one call of pkt_nat_batch, as the handle's halves take it
struct NatCall {
    BatchSrc src;
    uint64_t n;
    const uint8_t* n_hdrs;
    const uint8_t* hdr_type;
    const uint16_t* hdr_off;
    uint32_t which, flags, dir_all, now;
    const uint8_t* dir;
    const uint8_t* select;
    uint8_t* status;
    uint32_t* entry;
    uint8_t* created;
    uint64_t* hits;
    uint64_t* bytes;
};

// a packet's direction: PKT_NAT_OUT, PKT_NAT_IN, or 2 = skipped (step 1)
PKT_HD uint32_t nat_dir(const NatCall& c, uint64_t i) {
    if (c.select && !c.select[i]) return 2u;
    const uint32_t d = c.dir ? c.dir[i] : c.dir_all;
    return d > 1u ? 2u : d;
}

struct pkt_nat;
// the device handle's calls (pktgpu_nat.hip); every refusal that needs no device is made before them
struct NatDevOps {
    int (*batch)(pkt_nat* t, const NatCall& c, void* stream);
    int (*expire)(pkt_nat* t, uint32_t now, const uint32_t idle[3], uint64_t* n_expired);
    int (*fetch)(pkt_nat* t, std::vector<uint64_t>* rev, std::vector<uint32_t>* seen, std::vector<uint32_t>* used);
    int (*put)(pkt_nat* t, pkt_nat_record_t* dst, const pkt_nat_record_t* src, uint64_t count);
    int (*clear)(pkt_nat* t, void* stream);
    int (*destroy)(pkt_nat* t);
    void (*refused)(pkt_nat* t);  // t->err also goes to the ctx
};

struct pkt_nat {
    const NatDevOps* ops = nullptr;  // NULL: a host handle
    NatImage img;
    NatView v{};
    std::string err;
    // host handle: the storage behind `v`
    std::vector<uint64_t> h_fkey, h_rev;
    std::vector<uint32_t> h_fval, h_ffirst, h_seen, h_used, h_cursor;
    // device handle
    void* ctx = nullptr;  // pkt_ctx
    int device = 0;
    void* dev_buf = nullptr;        // one allocation behind `v`, the second forward buffer and the scratch
    uint64_t* fkey2 = nullptr;      // the second forward buffer (pkt_nat_expire rebuilds into it and swaps)
    uint32_t* fval2 = nullptr;
    uint32_t* ffirst2 = nullptr;
    uint32_t* slot_scr = nullptr;   // [kNatChunk]: a chunk's candidate slots, then its creators' slots
    uint32_t* tile_cnt = nullptr;   // [3][kNatChunk / 256]: creators per tile, then their exclusive prefix
    uint32_t* seg = nullptr;        // [3][nblk + 2]: free entries per segment, then their exclusive prefix and total
    uint32_t* ctl = nullptr;        // [16]: ncreate[3], ncr[3], cur0[3], expired, ...
};

inline int nat_fail(pkt_nat* t, const char* where, const char* msg) {
    if (t) {
        t->err = std::string(where) + ": " + msg;
        if (t->ops) t->ops->refused(t);
    }
    return PKT_ERR_INVALID_ARG;
}

inline void nat_view_config(NatView& v, const NatImage& img) {
    v.slots = img.slots;
    v.naddr = img.naddr;
    v.nports = img.nports;
    v.port_lo = img.port_lo;
    v.nstatic = img.nstatic;
    v.E = img.E;
    v.W = img.W;
    v.nblk = img.nblk;
}

// a session's record
inline pkt_nat_record_t nat_record(uint64_t in, uint64_t out, uint32_t flags, uint32_t last_seen) {
    pkt_nat_record_t r{};
    const uint32_t ia = nat_key_addr(in), oa = nat_key_addr(out);
    for (int k = 0; k < 4; k++) {
        r.in_addr[k] = (uint8_t)(ia >> (24 - 8 * k));
        r.out_addr[k] = (uint8_t)(oa >> (24 - 8 * k));
    }
    r.in_port = (uint16_t)nat_key_port(in);
    r.out_port = (uint16_t)nat_key_port(out);
    r.proto = (uint8_t)nat_proto_of(nat_key_p(in));
    r.flags = (uint8_t)flags;
    r.last_seen = last_seen;
    return r;
}
