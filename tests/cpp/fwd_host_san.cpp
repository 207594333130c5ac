// fwd_host_san.cpp — pkt_fwd_host (packet-rs_amd/csrc/pktgpu_host.cpp with pktgpu_fwd.hpp: the decision, the checksum
// arithmetic and the refusals the kernel shares) under AddressSanitizer + UndefinedBehaviorSanitizer: a stand-alone
// program, no GPU.  Every array (adjacencies, slab, chain columns, next hops, select, outputs, counters) is a heap
// block of its exact size, so a read or write past one is a report.  Packets lie at every source alignment 0..15,
// the last one ending on the slab's last byte; some chain columns are forged (an IP or Ether offset past the packet,
// n_hdrs of 255); every NULL-output combination runs with and without PKT_FWD_KEEP_L2 / PKT_FWD_NO_WRITE; the next
// hops come from an array and from a host lpm handle; the refusals leave everything alone.  Statuses, ports, adjacency
// indices, counters and every byte of the slab are checked against values worked out here.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/pktgpu.h"

namespace {

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 16);
}

[[noreturn]] void die(const char* what, uint64_t i) {
    std::printf("FAIL %s at %llu\n", what, (unsigned long long)i);
    std::exit(1);
}

// a heap block of exactly n elements
template <typename T>
struct Block {
    T* p;
    uint64_t n;
    explicit Block(uint64_t n_) : p(static_cast<T*>(std::malloc(n_ ? n_ * sizeof(T) : 1))), n(n_) {
        if (n) std::memset(static_cast<void*>(p), 0x77, n * sizeof(T));
    }
    ~Block() { std::free(p); }
    Block(const Block&) = delete;
    Block& operator=(const Block&) = delete;
    T& operator[](uint64_t i) { return p[i]; }
};

constexpr uint32_t kAdj = 8;
constexpr uint64_t kFill64 = 0x7777777777777777ull;

struct Want {
    uint8_t status;
    uint32_t port, adj;
};

// RFC 1624 eq. 3 as include/pktgpu.h states it
uint16_t csum_1624(uint16_t hc, uint16_t m) {
    const uint32_t m2 = (uint32_t)m - 0x0100u;
    uint32_t s = (~(uint32_t)hc & 0xFFFFu) + (~(uint32_t)m & 0xFFFFu) + m2;
    s = (s & 0xFFFFu) + (s >> 16);
    s = (s & 0xFFFFu) + (s >> 16);
    return (uint16_t)(~s & 0xFFFFu);
}

struct Outs {
    Block<uint8_t> status;
    Block<uint32_t> port, adj;
    Block<uint64_t> hits, bytes;
    explicit Outs(uint64_t n) : status(n), port(n), adj(n), hits(PKT_FWD_STATUS_COUNT), bytes(PKT_FWD_STATUS_COUNT) {}
};

void drive(uint64_t n, bool with_lpm) {
    // ---- adjacencies: 5 drops, 6 punts, 7 has an mtu between the IPv4 and the IPv6 packets' L3 lengths
    Block<pkt_fwd_adj_t> adj(kAdj);
    for (uint32_t k = 0; k < kAdj; k++) {
        pkt_fwd_adj_t a{};
        for (auto& x : a.dmac) x = (uint8_t)rnd();
        for (auto& x : a.smac) x = (uint8_t)rnd();
        a.port = 1000 + k;
        a.mtu = k == 7 ? 30 : k == 1 ? 1500 : 0;
        a.action = k == 5 ? PKT_FWD_ACT_DROP : k == 6 ? PKT_FWD_ACT_PUNT : PKT_FWD_ACT_FORWARD;
        adj[k] = a;
    }
    // ---- a host lpm handle: 10.k.0.0/16 -> k for k < 10, 2001:db8:k::/48 -> k; the default next hop is 9 (no adjacency)
    pkt_lpm_t* lpm = nullptr;
    if (with_lpm) {
        Block<pkt_lpm_route_t> rt(20);
        for (uint32_t k = 0; k < 10; k++) {
            pkt_lpm_route_t r4{}, r6{};
            r4.addr[0] = 10, r4.addr[1] = (uint8_t)k, r4.ipver = 4, r4.plen = 16, r4.nexthop = k;
            r6.addr[0] = 0x20, r6.addr[1] = 0x01, r6.addr[2] = 0x0d, r6.addr[3] = 0xb8, r6.addr[5] = (uint8_t)k;
            r6.ipver = 6, r6.plen = 48, r6.nexthop = k;
            rt[2 * k] = r4, rt[2 * k + 1] = r6;
        }
        if (pkt_lpm_create_host(rt.p, 20, 9, 0, &lpm) != PKT_SUCCESS) die("lpm create", 0);
    }
    // ---- packets: Ether / IPv4 (34 bytes + a tail) | Ether / Vlan / IPv6 (58 + a tail), packet i at alignment i % 16
    Block<uint64_t> offs(n);
    Block<uint32_t> lens(n), nexthop(n);
    Block<uint8_t> nh(n), ty(PKT_MAX_HDRS * n), sel(n);
    Block<uint16_t> of(PKT_MAX_HDRS * n);
    std::memset(ty.p, 0, ty.n);
    std::memset(static_cast<void*>(of.p), 0, of.n * 2);
    std::vector<Want> want(n);
    std::vector<uint32_t> ipo(n), hop(n);
    std::vector<uint8_t> kind(n);  // 0 plain, 1 cut, 2 no ip, 3 ip offset forged, 4 ether offset forged, 5 no ether entry
    uint64_t pos = 0;
    for (uint64_t i = 0; i < n; i++) {
        const bool v4 = i % 3 != 0;
        const uint32_t ip = v4 ? 14 : 18, hs = v4 ? 20 : 40;
        kind[i] = i % 11 == 4 && i + 1 < n ? 1 : i % 7 == 2 ? 2 : i % 17 == 7 ? 3 : i % 23 == 9 ? 4 : i % 29 == 11 ? 5 : 0;
        pos = (pos + 15) / 16 * 16 + i % 16;
        offs[i] = pos;
        lens[i] = kind[i] == 1 ? ip + hs - 1 : ip + hs + (i + 1 < n ? rnd() % 9 : 0);  // the last packet ends with its IP header
        pos += lens[i];
        ipo[i] = ip;
        nh[i] = i % 13 == 3 ? 255 : v4 ? 2 : 3;
        ty[0 * n + i] = kind[i] == 5 ? PKT_HDR_VLAN : PKT_HDR_ETHER;
        of[0 * n + i] = kind[i] == 4 ? (uint16_t)(lens[i] - 13) : 0;
        if (!v4) ty[1 * n + i] = PKT_HDR_VLAN, of[1 * n + i] = 14;
        ty[(v4 ? 1 : 2) * n + i] = kind[i] == 2 ? PKT_HDR_ARP : v4 ? PKT_HDR_IPV4 : PKT_HDR_IPV6;
        of[(v4 ? 1 : 2) * n + i] = kind[i] == 3 ? (uint16_t)(i % 2 ? 65535 : lens[i] - hs + 1) : (uint16_t)ip;
        sel[i] = i % 19 != 5;
        hop[i] = (uint32_t)(i % 10);
        nexthop[i] = hop[i] == 9 && i % 4 == 1 ? 0xFFFFFFFFu : hop[i];
    }
    Block<uint8_t> slab(pos), before(pos);
    for (uint64_t k = 0; k < pos; k++) slab[k] = (uint8_t)rnd();
    uint64_t whits[PKT_FWD_STATUS_COUNT] = {}, wbytes[PKT_FWD_STATUS_COUNT] = {};
    for (uint64_t i = 0; i < n; i++) {
        const bool v4 = i % 3 != 0;
        uint8_t* p = slab.p + offs[i];
        const uint32_t ip = ipo[i];
        const bool whole = kind[i] != 1;
        uint32_t ttl = i % 5 == 0 ? (uint32_t)(i % 2) : 2 + rnd() % 254;
        if (whole) {
            if (v4) {
                p[ip + 2] = 0, p[ip + 3] = 28, p[ip + 8] = (uint8_t)ttl;
                p[ip + 16] = 10, p[ip + 17] = (uint8_t)hop[i];
            } else {
                p[ip + 4] = 0, p[ip + 5] = 8, p[ip + 7] = (uint8_t)ttl;
                const uint8_t d[6] = {0x20, 0x01, 0x0d, 0xb8, 0, (uint8_t)hop[i]};
                std::memcpy(p + ip + 24, d, 6);
            }
        }
        Want w{PKT_FWD_OK, PKT_FWD_NONE, PKT_FWD_NONE};
        const uint32_t a = with_lpm ? hop[i] : nexthop[i];
        if (!sel[i]) w.status = PKT_FWD_SKIPPED;
        else if (kind[i] == 2) w.status = PKT_FWD_NO_IP;
        else if (kind[i] == 1 || kind[i] == 3) w.status = PKT_FWD_SPAN;
        else if (kind[i] == 5) w.status = PKT_FWD_NO_ETHER;
        else if (kind[i] == 4) w.status = PKT_FWD_SPAN;
        else if (ttl <= 1) w.status = PKT_FWD_TTL;
        else {
            w.adj = a;
            if (a >= kAdj) w.status = PKT_FWD_NO_ADJ;
            else if (a == 5) w.status = PKT_FWD_DROP;
            else if (a == 6) w.status = PKT_FWD_PUNT;
            else if (a == 7 && !v4) w.status = PKT_FWD_MTU;
            else w.port = 1000 + a;
        }
        want[i] = w;
        whits[w.status]++;
        wbytes[w.status] += lens[i];
    }
    std::memcpy(before.p, slab.p, pos);
    pkt_batch_t b{};
    b.slab = slab.p;
    b.slab_len = pos;
    b.offsets = offs.p;
    b.lens = lens.p;
    b.n = n;
    const pkt_chain_t ch{nh.p, ty.p, of.p};
    // the slab a call with `flags` must leave, from `before`
    std::vector<uint8_t> after(pos);
    auto expect_slab = [&](uint32_t flags) {
        std::memcpy(after.data(), before.p, pos);
        if (flags & PKT_FWD_NO_WRITE) return;
        for (uint64_t i = 0; i < n; i++) {
            if (want[i].status != PKT_FWD_OK) continue;
            uint8_t* p = after.data() + offs[i];
            const uint32_t a = want[i].adj, ip = ipo[i];
            std::memcpy(p, adj[a].dmac, 6);
            std::memcpy(p + 6, adj[a].smac, 6);
            if (i % 3 != 0) {
                const uint16_t hc = csum_1624((uint16_t)(p[ip + 10] << 8 | p[ip + 11]), (uint16_t)(p[ip + 8] << 8 | p[ip + 9]));
                p[ip + 8]--;
                p[ip + 10] = (uint8_t)(hc >> 8), p[ip + 11] = (uint8_t)hc;
            } else {
                p[ip + 7]--;
            }
        }
    };
    for (uint32_t flags : {0u, (uint32_t)PKT_FWD_NO_WRITE}) {
        for (uint32_t mask = 0; mask < 32; mask++) {
            std::memcpy(slab.p, before.p, pos);
            Outs o(n);
            const int rc = pkt_fwd_host(adj.p, kAdj, &b, &ch, 0, flags, lpm, with_lpm ? nullptr : nexthop.p, sel.p,
                                        mask & 1 ? o.status.p : nullptr, mask & 2 ? o.port.p : nullptr, mask & 4 ? o.adj.p : nullptr,
                                        mask & 8 ? o.hits.p : nullptr, mask & 16 ? o.bytes.p : nullptr);
            if (rc != PKT_SUCCESS) die("pkt_fwd_host", mask);
            for (uint64_t i = 0; i < n; i++) {
                if ((mask & 1) && o.status[i] != want[i].status) die("status", i);
                if ((mask & 2) && o.port[i] != want[i].port) die("port", i);
                if ((mask & 4) && o.adj[i] != want[i].adj) die("adj_index", i);
                if (!(mask & 2) && o.port[i] != 0x77777777u) die("a NULL output's neighbour written", i);
            }
            for (uint32_t s = 0; s < PKT_FWD_STATUS_COUNT; s++) {
                if (o.hits[s] != kFill64 + (mask & 8 ? whits[s] : 0)) die("hits", s);
                if (o.bytes[s] != kFill64 + (mask & 16 ? wbytes[s] : 0)) die("bytes", s);
            }
            expect_slab(flags);
            if (std::memcmp(slab.p, after.data(), pos) != 0) die("slab bytes", mask);
        }
    }
    // KEEP_L2: no Ether entry is looked for; only the statuses are compared with a second NO_WRITE run of the same call
    {
        std::memcpy(slab.p, before.p, pos);
        Outs o(n), q(n);
        if (pkt_fwd_host(adj.p, kAdj, &b, &ch, PKT_FLOW_LAST, PKT_FWD_KEEP_L2, lpm, with_lpm ? nullptr : nexthop.p, nullptr, o.status.p,
                         o.port.p, o.adj.p, nullptr, nullptr) != PKT_SUCCESS)
            die("keep_l2", 0);
        for (uint64_t i = 0; i < n; i++) {
            if (o.status[i] == PKT_FWD_NO_ETHER) die("keep_l2 looked for an Ether entry", i);
            if (std::memcmp(slab.p + offs[i], before.p + offs[i], 12) != 0) die("keep_l2 wrote a MAC", i);
        }
        std::memcpy(slab.p, before.p, pos);
        if (pkt_fwd_host(adj.p, kAdj, &b, &ch, PKT_FLOW_LAST, PKT_FWD_KEEP_L2 | PKT_FWD_NO_WRITE, lpm, with_lpm ? nullptr : nexthop.p, nullptr,
                         q.status.p, q.port.p, q.adj.p, nullptr, nullptr) != PKT_SUCCESS)
            die("keep_l2 no_write", 0);
        if (std::memcmp(o.status.p, q.status.p, n) || std::memcmp(o.port.p, q.port.p, 4 * n) || std::memcmp(slab.p, before.p, pos))
            die("keep_l2 no_write differs", 0);
    }
    // ---- refusals leave the outputs and the slab alone
    {
        std::memcpy(slab.p, before.p, pos);
        Outs r(n);
        pkt_batch_t nolens = b;
        nolens.lens = nullptr;
        pkt_fwd_adj_t bad_action = adj[0], bad_zero = adj[0];
        bad_action.action = 3;
        bad_zero.zero = 1;
        const uint32_t* nhp = with_lpm ? nullptr : nexthop.p;
        auto call = [&](const pkt_fwd_adj_t* a, uint32_t na, const pkt_batch_t* bb, const pkt_chain_t* cc, uint32_t which, uint32_t flags,
                        pkt_lpm_t* l, const uint32_t* h, uint64_t* hits) {
            return pkt_fwd_host(a, na, bb, cc, which, flags, l, h, sel.p, r.status.p, r.port.p, r.adj.p, hits, r.bytes.p);
        };
        const pkt_chain_t nocol{nh.p, nullptr, of.p};
        if (call(adj.p, kAdj, &b, &ch, 16, 0, lpm, nhp, r.hits.p) != PKT_ERR_INVALID_ARG) die("which_ip 16", 0);
        if (call(adj.p, kAdj, &b, &ch, 0xFE, 0, lpm, nhp, r.hits.p) != PKT_ERR_INVALID_ARG) die("which_ip 0xFE", 0);
        if (call(adj.p, kAdj, &b, &ch, 0, 4, lpm, nhp, r.hits.p) != PKT_ERR_INVALID_ARG) die("flag bits", 0);
        if (call(adj.p, kAdj, &nolens, &ch, 0, 0, lpm, nhp, r.hits.p) != PKT_ERR_INVALID_ARG) die("offsets without lens", 0);
        if (call(adj.p, kAdj, nullptr, &ch, 0, 0, lpm, nhp, r.hits.p) != PKT_ERR_INVALID_ARG) die("null batch", 0);
        if (call(adj.p, kAdj, &b, nullptr, 0, 0, lpm, nhp, r.hits.p) != PKT_ERR_INVALID_ARG) die("null chain", 0);
        if (call(adj.p, kAdj, &b, &nocol, 0, 0, lpm, nhp, r.hits.p) != PKT_ERR_INVALID_ARG) die("null chain column", 0);
        if (call(adj.p, kAdj, &b, &ch, 0, 0, nullptr, nullptr, r.hits.p) != PKT_ERR_INVALID_ARG) die("neither", 0);
        if (with_lpm && call(adj.p, kAdj, &b, &ch, 0, 0, lpm, nexthop.p, r.hits.p) != PKT_ERR_INVALID_ARG) die("both", 0);
        if (call(adj.p, kAdj, &b, &ch, 0, 0, lpm, nhp, reinterpret_cast<uint64_t*>(reinterpret_cast<uint8_t*>(r.hits.p) + 4)) != PKT_ERR_INVALID_ARG)
            die("misaligned hits", 0);
        if (call(&bad_action, 1, &b, &ch, 0, 0, lpm, nhp, r.hits.p) != PKT_ERR_INVALID_ARG) die("action", 0);
        if (call(&bad_zero, 1, &b, &ch, 0, 0, lpm, nhp, r.hits.p) != PKT_ERR_INVALID_ARG) die("zero", 0);
        if (call(nullptr, 1, &b, &ch, 0, 0, lpm, nhp, r.hits.p) != PKT_ERR_INVALID_ARG) die("null adj", 0);
        if (call(adj.p, PKT_FWD_MAX_ADJ + 1, &b, &ch, 0, 0, lpm, nhp, r.hits.p) != PKT_ERR_INVALID_ARG) die("nadj", 0);
        for (uint64_t i = 0; i < n; i++)
            if (r.status[i] != 0x77 || r.port[i] != 0x77777777u || r.adj[i] != 0x77777777u) die("refusal wrote", i);
        for (uint32_t s = 0; s < PKT_FWD_STATUS_COUNT; s++)
            if (r.hits[s] != kFill64 || r.bytes[s] != kFill64) die("refusal counted", s);
        if (std::memcmp(slab.p, before.p, pos)) die("refusal wrote the slab", 0);
        // nadj == 0 with a NULL array is legal: nobody is forwarded
        if (call(nullptr, 0, &b, &ch, 0, 0, lpm, nhp, r.hits.p) != PKT_SUCCESS) die("nadj 0", 0);
        for (uint64_t i = 0; i < n; i++)
            if (r.status[i] == PKT_FWD_OK || r.port[i] != PKT_FWD_NONE) die("nadj 0 forwarded", i);
        if (std::memcmp(slab.p, before.p, pos)) die("nadj 0 wrote the slab", 0);
        // n == 0
        pkt_batch_t empty = b;
        empty.n = 0;
        Outs e(1);
        if (pkt_fwd_host(adj.p, kAdj, &empty, &ch, 0, 0, lpm, nhp, nullptr, e.status.p, e.port.p, e.adj.p, e.hits.p, e.bytes.p) != PKT_SUCCESS ||
            e.status[0] != 0x77 || e.hits[0] != kFill64)
            die("n == 0", 0);
    }
    if (lpm && pkt_lpm_destroy(lpm) != PKT_SUCCESS) die("lpm destroy", 0);
    std::printf("%s: %llu packets, statuses", with_lpm ? "lpm" : "nexthop", (unsigned long long)n);
    for (uint32_t s = 0; s < PKT_FWD_STATUS_COUNT; s++) std::printf(" %llu", (unsigned long long)whits[s]);
    std::printf("\n");
}

}  // namespace

int main() {
    if (pkt_sizeof_fwd_adj() != 20 || sizeof(pkt_fwd_adj_t) != 20) die("sizeof", 0);
    for (uint64_t n : {1ull, 2ull, 63ull, 700ull}) {
        drive(n, false);
        drive(n, true);
    }
    std::printf("fwd OK\n");
    return 0;
}
