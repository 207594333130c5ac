// pktgpu_lpm.hpp — what the two halves of pkt_lpm_* share: the handle behind pkt_lpm_t, the compiled table (a
// leaf-pushed multibit trie, 16-bit root stride, then 8-bit strides), its compiler and THE walk.  pktgpu_host.cpp
// holds the public pkt_lpm_* calls and the host handle's sequential loops (it compiles under g++ alone);
// pktgpu_lpm.hip holds pkt_lpm_create and the device handle's lookups, which the handle reaches through `ops`.
// The kernel and the host loops call the same lpm_walk, so the CPU tests cover the whole compile-and-walk logic.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "pktgpu_batch.hpp"

static_assert(sizeof(pkt_lpm_route_t) == 24 && sizeof(pkt_lpm_info_t) == 56, "lpm ABI structs");

constexpr uint32_t kLpmChild = 0x80000000u;  // an entry's bit 31: the low bits are a child node's index
constexpr uint32_t kLpmRoot = 1u << 16;      // entries of a root
constexpr uint32_t kLpmNode = 256;           // entries of a node
constexpr uint32_t kLpmMaxLevels = 15;       // the root and 14 node levels: 16 + 14 * 8 = 128 bits
constexpr uint64_t kLpmDefaultBytes = 1ull << 30;

// a route's record, read once at the end of a lookup
struct alignas(8) LpmRec {
    uint32_t nexthop, plen;
};

// The compiled table as a lookup sees it: host or device addresses.  Node k is nodes[256 * k ..]; the two
// versions share the node pool.
struct LpmView {
    const uint32_t* root4;
    const uint32_t* root6;
    const uint32_t* nodes;
    const LpmRec* rec;
    uint32_t depth4, depth6;  // the deepest level a route reached (the root is 1; 0: no route of the version)
    uint32_t default_nexthop;
};

// byte k (0..15) of an address held as four big-endian words
PKT_HD uint32_t lpm_byte(const uint32_t w[4], uint32_t k) { return w[k >> 2] >> (24u - 8u * (k & 3u)) & 0xFFu; }

// THE walk: the entry at which the lookup of address w (four big-endian words; IPv4 in w[0]) ends: a route's index
// + 1, or 0 for no route.  A chain of dependent loads, bounded by the table's depth: below the deepest level no
// entry has bit 31.  (Unrolled, so that w is indexed by constants and stays in registers.)
PKT_HD uint32_t lpm_walk(const uint32_t w[4], bool v4, const LpmView& t) {
    const uint32_t depth = v4 ? t.depth4 : t.depth6;
    if (depth == 0) return 0;
    uint32_t e = (v4 ? t.root4 : t.root6)[w[0] >> 16];
#ifdef __HIPCC__
#pragma unroll
#endif
    for (uint32_t lvl = 1; lvl < kLpmMaxLevels; lvl++) {  // node level lvl takes address byte lvl + 1
        if (lvl >= depth || !(e & kLpmChild)) break;
        e = t.nodes[(uint64_t)(e & ~kLpmChild) * kLpmNode + lpm_byte(w, lvl + 1)];
    }
    return e & kLpmChild ? 0u : e;  // (a child entry at the deepest level: never compiled)
}

// the four outputs of one packet
struct LpmResult {
    uint32_t route, nexthop, plen, status;
};

PKT_HD LpmResult lpm_miss(const LpmView& t, uint32_t status) { return LpmResult{PKT_LPM_NONE, t.default_nexthop, 0xFFu, status}; }

// the lookup of one address (need_rec: nexthop or plen is asked for)
PKT_HD LpmResult lpm_lookup(const uint32_t w[4], bool v4, const LpmView& t, bool need_rec) {
    const uint32_t e = lpm_walk(w, v4, t);
    if (!e) return lpm_miss(t, PKT_LPM_NO_ROUTE);
    LpmResult r{e - 1u, 0u, 0u, PKT_LPM_OK};
    if (need_rec) {
        const LpmRec rec = t.rec[e - 1u];
        r.nexthop = rec.nexthop;
        r.plen = rec.plen;
    }
    return r;
}

// ------------------------------------------------------------------ the compiler (host code)

// The compiled table in one block of words: [root4 2^16][root6 2^16][nodes 256 each][records 2 each].
struct LpmImage {
    std::vector<uint32_t> words;
    pkt_lpm_info_t info{};
    uint64_t nodes_at() const { return 2ull * kLpmRoot; }
    uint64_t rec_at() const { return nodes_at() + (info.nodes_v4 + info.nodes_v6) * kLpmNode; }
    LpmView view(const uint32_t* base, uint32_t default_nexthop) const {
        return LpmView{base, base + kLpmRoot, base + nodes_at(), reinterpret_cast<const LpmRec*>(base + rec_at()),
                       (uint32_t)info.depth_v4, (uint32_t)info.depth_v6, default_nexthop};
    }
};

inline int lpm_refuse(std::string& err, int code, const std::string& msg) {
    err = "pkt_lpm_create: " + msg;
    return code;
}

// Validate `routes` and compile them.  PKT_SUCCESS, or the refusal with its text in `err`.
inline int lpm_compile(const pkt_lpm_route_t* routes, uint32_t n, uint64_t max_bytes, LpmImage& img, std::string& err) {
    if (n > PKT_LPM_MAX_ROUTES) return lpm_refuse(err, PKT_ERR_INVALID_ARG, "nroutes above PKT_LPM_MAX_ROUTES");
    if (n && !routes) return lpm_refuse(err, PKT_ERR_INVALID_ARG, "null routes");
    if (max_bytes == 0) max_bytes = kLpmDefaultBytes;
    pkt_lpm_info_t& info = img.info;
    info = pkt_lpm_info_t{};
    const auto bad = [&](uint32_t i, const char* what) {
        return lpm_refuse(err, PKT_ERR_INVALID_ARG, "route " + std::to_string(i) + ": " + what);
    };
    for (uint32_t i = 0; i < n; i++) {
        const pkt_lpm_route_t& r = routes[i];
        if (r.ipver != 4 && r.ipver != 6) return bad(i, "ipver is neither 4 nor 6");
        if (r.plen > (r.ipver == 4 ? 32 : 128)) return bad(i, "plen above 32 / 128");
        if (r.zero) return bad(i, "non-zero `zero`");
        for (uint32_t k = r.plen / 8; k < 16; k++) {
            const uint32_t keep = k == r.plen / 8u ? (0xFF00u >> (r.plen & 7u)) & 0xFFu : 0u;  // the byte's bits below plen
            if (r.addr[k] & ~keep) return bad(i, "an address bit at or past plen is set");
        }
        (r.ipver == 4 ? info.routes_v4 : info.routes_v6)++;
    }
    // by (version, address, plen): equal routes become neighbours, and so do the routes below one node
    std::vector<uint32_t> ord(n);
    for (uint32_t i = 0; i < n; i++) ord[i] = i;
    std::sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) {
        const pkt_lpm_route_t &x = routes[a], &y = routes[b];
        if (x.ipver != y.ipver) return x.ipver < y.ipver;
        const int c = memcmp(x.addr, y.addr, 16);
        if (c) return c < 0;
        if (x.plen != y.plen) return x.plen < y.plen;
        return a < b;
    });
    for (uint32_t k = 1; k < n; k++) {
        const pkt_lpm_route_t &x = routes[ord[k - 1]], &y = routes[ord[k]];
        if (x.ipver == y.ipver && x.plen == y.plen && !memcmp(x.addr, y.addr, 16))
            return lpm_refuse(err, PKT_ERR_INVALID_ARG, "routes " + std::to_string(std::min(ord[k - 1], ord[k])) + " and " +
                                                            std::to_string(std::max(ord[k - 1], ord[k])) +
                                                            " have the same (ipver, plen, prefix)");
    }
    // The nodes: one per distinct prefix of 16 + 8j bits (j = 0..13) among the routes longer than it.  In the sorted
    // order those routes are neighbours, so a node is new iff its prefix differs from the last such route's.
    {
        const pkt_lpm_route_t* last[kLpmMaxLevels] = {};
        for (uint32_t k = 0; k < n; k++) {
            const pkt_lpm_route_t& r = routes[ord[k]];
            for (uint32_t j = 0; 16u + 8u * j < r.plen; j++) {
                const pkt_lpm_route_t* p = last[j];
                if (!p || p->ipver != r.ipver || memcmp(p->addr, r.addr, 2 + j)) (r.ipver == 4 ? info.nodes_v4 : info.nodes_v6)++;
                last[j] = &r;
            }
        }
    }
    const uint64_t nnodes = info.nodes_v4 + info.nodes_v6;
    info.bytes = 4ull * (2ull * kLpmRoot + nnodes * kLpmNode) + 8ull * n;
    if (info.bytes > max_bytes)
        return lpm_refuse(err, PKT_ERR_UNSUPPORTED, "the compiled table needs " + std::to_string(info.bytes) + " bytes, max_bytes is " +
                                                        std::to_string(max_bytes));
    if (nnodes >= kLpmChild) return lpm_refuse(err, PKT_ERR_UNSUPPORTED, "more than 2^31 nodes");
    img.words.assign(info.bytes / 4, 0u);
    uint32_t* const root[2] = {img.words.data(), img.words.data() + kLpmRoot};
    uint32_t* const nodes = img.words.data() + img.nodes_at();
    uint32_t* const rec = img.words.data() + img.rec_at();  // {nexthop, plen} per route: LpmRec
    // by ascending plen: a fill never meets a child entry (children hang under entries only routes past this
    // level's last bit create, and those come later), and a longer prefix overwrites a shorter one
    std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return routes[a].plen < routes[b].plen; });
    uint64_t next = 0;
    for (uint32_t k = 0; k < n; k++) {
        const uint32_t idx = ord[k];
        const pkt_lpm_route_t& r = routes[idx];
        rec[2ull * idx] = r.nexthop;
        rec[2ull * idx + 1] = r.plen;
        const uint32_t L = r.plen, leaf = idx + 1u;
        uint32_t* tab = root[r.ipver == 6];
        uint32_t at = (uint32_t)r.addr[0] << 8 | r.addr[1], bits = 16, level = 1;
        while (L > bits) {  // down through the entry at `at`, creating the child as a copy of what it held
            uint32_t& e = tab[at];
            if (!(e & kLpmChild)) {
                uint32_t* nd = nodes + next * kLpmNode;
                for (uint32_t q = 0; q < kLpmNode; q++) nd[q] = e;
                e = kLpmChild | (uint32_t)next++;
            }
            tab = nodes + (uint64_t)(e & ~kLpmChild) * kLpmNode;
            at = r.addr[level + 1];
            bits += 8;
            level++;
        }
        const uint32_t count = 1u << (bits - L);
        for (uint32_t q = 0; q < count; q++) tab[at + q] = leaf;
        uint64_t& depth = r.ipver == 4 ? info.depth_v4 : info.depth_v6;
        depth = depth > level ? depth : level;
    }
    if (next != nnodes) return lpm_refuse(err, PKT_ERR_UNSUPPORTED, "internal: node count mismatch");
    return PKT_SUCCESS;
}

// One lookup call's arguments, as the device half takes them.
struct LpmCall {
    bool from_keys;
    BatchSrc src;  // batch source
    uint64_t n;
    const uint8_t* n_hdrs;
    const uint8_t* hdr_type;
    const uint16_t* hdr_off;
    const uint8_t* keys;  // keys source: [n][40]
    const uint8_t* key_status;
    uint32_t which, flags;
    uint32_t* route;
    uint32_t* nexthop;
    uint8_t* plen;
    uint8_t* status;
};

struct pkt_lpm;
struct LpmDevOps {
    int (*lookup)(pkt_lpm* t, const LpmCall& c, void* stream);
    int (*destroy)(pkt_lpm* t);
};

struct pkt_lpm {
    const LpmDevOps* ops = nullptr;  // NULL: a host handle
    LpmView view{};
    pkt_lpm_info_t info{};
    std::vector<uint32_t> host_words;  // host handle: the image
    std::string err;
    // device handle
    int device = 0;
    uint32_t* dev_words = nullptr;
};

inline int lpm_fail(pkt_lpm* t, int code, const char* msg) {
    if (t) t->err = msg;
    return code;
}
