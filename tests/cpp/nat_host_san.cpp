// nat_host_san.cpp — the host handle of pkt_nat_* (packet-rs_amd/csrc/pktgpu_host.cpp with pktgpu_nat.hpp: the
// decision, the entry arithmetic, the inbound lookup, the checksum update and the refusals the kernels share) under
// AddressSanitizer + UndefinedBehaviorSanitizer: a stand-alone program, no GPU.  Every array (pool, statics, slab,
// chain columns, dir, select, outputs, counters, records) is a heap block of its exact size, so a read or write past
// one is a report.  Packets lie at every alignment 0..15, the last one ending on the slab's last byte; some chain
// columns are forged (an IP or L4 offset past the packet, n_hdrs of 255); every NULL-output combination runs with and
// without PKT_NAT_NO_WRITE; the refusals leave everything alone.  Statuses, entries, created flags, counters, records
// and the checksums (summed again here by RFC 1071) are checked against values worked out here.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/pktgpu.h"

namespace {

[[noreturn]] void die(const char* what, uint64_t i) {
    std::printf("FAIL %s at %llu\n", what, (unsigned long long)i);
    std::exit(1);
}

template <typename T>
struct Block {  // a heap block of exactly n elements
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

constexpr uint64_t kFill64 = 0x7777777777777777ull;
constexpr uint32_t kLo = 5000, kHi = 5009, kPorts = 10, kAddr = 2, kE = kAddr * kPorts;
const uint8_t kPool[8] = {192, 0, 2, 1, 192, 0, 2, 2};

// the one's-complement sum of [p, p + n)
uint32_t ones_sum(const uint8_t* p, uint32_t n, uint32_t s = 0) {
    for (uint32_t k = 0; k < n; k += 2) s += (uint32_t)p[k] << 8 | (k + 1 < n ? p[k + 1] : 0);
    while (s >> 16) s = (s & 0xFFFFu) + (s >> 16);
    return s;
}

bool l4_valid(const uint8_t* ip, const uint8_t* l4, uint32_t seg) {
    uint32_t s = 0;
    if (ip[9] != 1) {
        s = ones_sum(ip + 12, 8);
        s += ip[9] + seg;
    }
    return ones_sum(l4, seg, s) == 0xFFFFu;
}

void put16(uint8_t* p, uint32_t v) { p[0] = (uint8_t)(v >> 8), p[1] = (uint8_t)v; }

// Ether / IPv4 / TCP | UDP | ICMP echo with `tail` payload bytes and valid checksums; returns the length
uint32_t build(uint8_t* p, uint32_t px, uint32_t src, uint32_t sport, uint32_t tail) {
    const uint32_t hs = px == 0 ? 20 : 8, seg = hs + tail, len = 34 + seg;
    std::memset(p, 0, len);
    p[12] = 0x08;
    uint8_t* ip = p + 14;
    ip[0] = 0x45, ip[8] = 64, ip[9] = px == 0 ? 6 : px == 1 ? 17 : 1;
    put16(ip + 2, 20 + seg);
    put16(ip + 12, src >> 16), put16(ip + 14, src & 0xFFFF);
    ip[16] = 198, ip[17] = 51, ip[18] = 100, ip[19] = 7;
    put16(ip + 10, 0xFFFFu - ones_sum(ip, 20));
    uint8_t* l4 = p + 34;
    if (px == 2) {
        l4[0] = 8;
        put16(l4 + 4, sport);
    } else {
        put16(l4, sport), put16(l4 + 2, 443);
        if (px == 1) put16(l4 + 4, seg);
        if (px == 0) l4[12] = 0x50;
    }
    for (uint32_t k = 0; k < tail; k++) l4[hs + k] = (uint8_t)(k * 7 + px);
    uint8_t* ck = l4 + (px == 0 ? 16 : px == 1 ? 6 : 2);
    uint32_t s = 0;
    if (px != 2) s = ones_sum(ip + 12, 8) + ip[9] + seg;
    put16(ck, 0xFFFFu - ones_sum(l4, seg, s));
    return len;
}

struct Outs {
    Block<uint8_t> status, created;
    Block<uint32_t> entry;
    Block<uint64_t> hits, bytes;
    explicit Outs(uint64_t n) : status(n), created(n), entry(n), hits(PKT_NAT_STATUS_COUNT), bytes(PKT_NAT_STATUS_COUNT) {}
};

void expect_refusal(int rc, const pkt_nat_t* t, const char* text, uint64_t where) {
    if (rc != PKT_ERR_INVALID_ARG) die("refusal code", where);
    if (std::strcmp(pkt_nat_last_error(t), text) != 0) {
        std::printf("got '%s'\n", pkt_nat_last_error(t));
        die("refusal text", where);
    }
}

void drive(uint64_t n) {
    Block<uint8_t> pool(8);
    std::memcpy(pool.p, kPool, 8);
    Block<pkt_nat_static_t> st(1);
    std::memset(static_cast<void*>(st.p), 0, sizeof(pkt_nat_static_t));
    st[0].proto = 17, st[0].in_port = 53, st[0].out_port = 53;
    st[0].in_addr[0] = 10, st[0].in_addr[3] = 53, st[0].out_addr[0] = 192, st[0].out_addr[2] = 2, st[0].out_addr[3] = 1;
    pkt_nat_t* t = nullptr;
    if (pkt_nat_create_host(pool.p, kAddr, kLo, kHi, 64, st.p, 1, &t) != PKT_SUCCESS) die("create", n);
    // ---- packets: flow f = i % nflows, protocol f % 3; kinds: 0 plain, 1 cut in the L4 bytes, 2 IP offset forged,
    // 3 L4 offset forged, 4 n_hdrs 255 (rows past the list hold zeros), 5 the static's inside endpoint, 6 skipped
    const uint32_t nflows = 40;  // 14 / 13 / 13 per protocol: UDP and ICMP fit in kE = 20, TCP too
    Block<uint64_t> offs(n);
    Block<uint32_t> lens(n);
    Block<uint8_t> nh(n), ty(PKT_MAX_HDRS * n), sel(n), dir(n);
    Block<uint16_t> of(PKT_MAX_HDRS * n);
    std::memset(ty.p, 0, ty.n);
    std::memset(static_cast<void*>(of.p), 0, of.n * 2);
    std::vector<uint8_t> kind(n);
    std::vector<uint32_t> flow(n), plen(n);
    std::vector<uint8_t> scratch(256);
    uint64_t pos = 0;
    for (uint64_t i = 0; i < n; i++) {
        kind[i] = i % 11 == 4 && i + 1 < n ? 1 : i % 13 == 6 ? 2 : i % 17 == 7 ? 3 : i % 19 == 9 ? 4 : i % 23 == 5 ? 5 : i % 29 == 3 ? 6 : 0;
        flow[i] = (uint32_t)(i * 7 % nflows);
        const uint32_t px = kind[i] == 5 ? 1 : flow[i] % 3;
        uint32_t len = build(scratch.data(), px, kind[i] == 5 ? 0x0A000035u : 0x0A000100u + flow[i], kind[i] == 5 ? 53 : 1000 + flow[i],
                             (uint32_t)(i % 9));
        if (kind[i] == 1) len = 34 + (px == 0 ? 19 : 7);
        plen[i] = len;
        pos = (pos + 15) / 16 * 16 + i % 16;
        offs[i] = pos, lens[i] = len;
        pos += len;
    }
    Block<uint8_t> slab(pos);  // the last packet ends on the slab's last byte
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t px = kind[i] == 5 ? 1 : flow[i] % 3;
        build(scratch.data(), px, kind[i] == 5 ? 0x0A000035u : 0x0A000100u + flow[i], kind[i] == 5 ? 53 : 1000 + flow[i], (uint32_t)(i % 9));
        std::memcpy(slab.p + offs[i], scratch.data(), plen[i]);
        nh[i] = kind[i] == 4 ? 255 : 3;
        ty[0 * n + i] = PKT_HDR_ETHER, of[0 * n + i] = 0;
        ty[1 * n + i] = PKT_HDR_IPV4, of[1 * n + i] = kind[i] == 2 ? (uint16_t)(plen[i] - 19) : 14;
        ty[2 * n + i] = px == 0 ? PKT_HDR_TCP : px == 1 ? PKT_HDR_UDP : PKT_HDR_ICMP;
        of[2 * n + i] = kind[i] == 3 ? 65535 : 34;
        sel[i] = kind[i] != 6;
        dir[i] = PKT_NAT_OUT;
    }
    Block<uint8_t> before(pos);
    std::memcpy(before.p, slab.p, pos);
    // ---- what must come out: the new flows take entries 0, 1, 2, ... of their protocol in index order
    std::vector<uint8_t> want_st(n), want_made(n, 0);
    std::vector<uint32_t> want_ent(n, PKT_NAT_NONE), ent_of(nflows, PKT_NAT_NONE), next(3, 0);
    uint64_t want_hits[PKT_NAT_STATUS_COUNT] = {}, want_bytes[PKT_NAT_STATUS_COUNT] = {};
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t px = flow[i] % 3;
        uint8_t s = PKT_NAT_OK;
        if (kind[i] == 6) s = PKT_NAT_SKIPPED;
        else if (kind[i] == 1 || kind[i] == 2 || kind[i] == 3) s = PKT_NAT_SPAN;
        else if (kind[i] == 5) want_ent[i] = PKT_NAT_STATIC | 0;
        else {
            if (ent_of[flow[i]] == PKT_NAT_NONE) {
                ent_of[flow[i]] = px * kE + next[px]++;
                want_made[i] = 1;
            }
            want_ent[i] = ent_of[flow[i]];
        }
        want_st[i] = s;
        want_hits[s]++, want_bytes[s] += plen[i];
    }
    pkt_batch_t b{};
    b.slab = slab.p, b.slab_len = pos, b.offsets = offs.p, b.lens = lens.p, b.n = n;
    pkt_chain_t ch{nh.p, ty.p, of.p};
    // ---- every NULL-output combination, with and without NO_WRITE, each from a cleared table
    for (uint32_t mask = 0; mask < 64; mask++) {
        Outs o(n);
        const uint32_t flags = mask & 32 ? PKT_NAT_NO_WRITE : 0;
        std::memcpy(slab.p, before.p, pos);
        if (pkt_nat_clear(t, nullptr) != PKT_SUCCESS) die("clear", mask);
        const int rc = pkt_nat_batch(t, &b, &ch, 0, flags, 7, dir.p, sel.p, 100, mask & 1 ? o.status.p : nullptr,
                                     mask & 2 ? o.entry.p : nullptr, mask & 4 ? o.created.p : nullptr, mask & 8 ? o.hits.p : nullptr,
                                     mask & 16 ? o.bytes.p : nullptr, nullptr);
        if (rc != PKT_SUCCESS) die("batch", mask);
        for (uint64_t i = 0; i < n; i++) {
            if ((mask & 1) && o.status[i] != want_st[i]) die("status", i);
            if ((mask & 2) && o.entry[i] != want_ent[i]) die("entry", i);
            if ((mask & 4) && o.created[i] != want_made[i]) die("created", i);
            uint8_t* p = slab.p + offs[i];
            const bool changed = std::memcmp(p, before.p + offs[i], plen[i]) != 0;
            if (changed != (want_st[i] == PKT_NAT_OK && !flags)) die("written or not", i);
            if (!changed) continue;
            // the source is the entry's outside endpoint, both checksums are valid again, nothing else moved
            const uint32_t px = p[14 + 9] == 6 ? 0 : p[14 + 9] == 17 ? 1 : 2;
            uint32_t addr_i = 0, port = 53;
            if (!(want_ent[i] & PKT_NAT_STATIC)) {
                const uint32_t e = want_ent[i] - px * kE;
                addr_i = e / kPorts, port = kLo + e % kPorts;
            }
            if (std::memcmp(p + 26, kPool + 4 * addr_i, 4) != 0) die("source address", i);
            const uint8_t* pt = p + 34 + (px == 2 ? 4 : 0);
            if (((uint32_t)pt[0] << 8 | pt[1]) != port) die("source port", i);
            if (ones_sum(p + 14, 20) != 0xFFFFu) die("ip checksum", i);
            if (!l4_valid(p + 14, p + 34, plen[i] - 34)) die("l4 checksum", i);
            const uint32_t ck = 34 + (px == 0 ? 16 : px == 1 ? 6 : 2), po = 34 + (px == 2 ? 4 : 0);
            for (uint32_t k = 0; k < plen[i]; k++) {
                const bool may = (k >= 24 && k < 30) || k == po || k == po + 1 || k == ck || k == ck + 1;
                if (!may && p[k] != before.p[offs[i] + k]) die("a byte outside the named fields", i);
            }
        }
        for (uint32_t s = 0; s < PKT_NAT_STATUS_COUNT; s++) {
            if ((mask & 8) && o.hits[s] != kFill64 + want_hits[s]) die("hits", s);
            if ((mask & 16) && o.bytes[s] != kFill64 + want_bytes[s]) die("bytes", s);
        }
        for (uint64_t k = 0; k < pos; k++)  // the gaps between the packets
            if (slab.p[k] != before.p[k] && flags) die("NO_WRITE wrote", k);
    }
    // ---- count, export into a block of the exact size, expire, export again
    uint64_t counts[3], total = 0, gone = 0;
    if (pkt_nat_count(t, counts) != PKT_SUCCESS) die("count", 0);
    for (uint32_t px = 0; px < 3; px++) {
        if (counts[px] != next[px]) die("counts", px);
        total += counts[px];
    }
    uint64_t nrec = 0;
    if (pkt_nat_export(t, nullptr, 0, &nrec) != PKT_SUCCESS || nrec != total + 1) die("export count", nrec);
    {
        Block<pkt_nat_record_t> rec(nrec);
        if (pkt_nat_export(t, rec.p, nrec, &nrec) != PKT_SUCCESS) die("export", 0);
        uint64_t k = 0;
        for (uint32_t px = 0; px < 3; px++)
            for (uint32_t e = 0; e < next[px]; e++, k++) {
                const pkt_nat_record_t& r = rec[k];
                if (r.proto != (px == 0 ? 6 : px == 1 ? 17 : 1) || r.out_port != kLo + e % kPorts || r.flags || r.last_seen != 100 ||
                    std::memcmp(r.out_addr, kPool + 4 * (e / kPorts), 4) != 0 || r.in_addr[0] != 10)
                    die("record", k);
            }
        if (rec[k].flags != PKT_NAT_REC_STATIC || rec[k].in_port != 53 || rec[k].proto != 17) die("static record", k);
        Block<pkt_nat_record_t> two(2);
        if (pkt_nat_export(t, two.p, 2, &nrec) != PKT_SUCCESS || nrec != total + 1) die("export cap", 0);
    }
    const uint32_t idle[3] = {0, 50, 0};
    if (pkt_nat_expire(t, 149, idle, &gone) != PKT_SUCCESS || gone != 0) die("expire early", gone);
    if (pkt_nat_expire(t, 150, idle, &gone) != PKT_SUCCESS || gone != next[1]) die("expire", gone);
    if (pkt_nat_expire(t, 150, idle, nullptr) != PKT_SUCCESS) die("expire null", 0);
    if (pkt_nat_count(t, counts) != PKT_SUCCESS || counts[0] != next[0] || counts[1] != 0 || counts[2] != next[2]) die("after expire", 0);
    // ---- inbound: the first TCP session's outside endpoint, a free one, somebody else's; dir_all with dir NULL
    {
        Block<uint8_t> in(3 * 64);
        Block<uint8_t> inh(3), ity(PKT_MAX_HDRS * 3);
        Block<uint16_t> iof(PKT_MAX_HDRS * 3);
        std::memset(ity.p, 0, ity.n);
        std::memset(static_cast<void*>(iof.p), 0, iof.n * 2);
        for (uint32_t k = 0; k < 3; k++) {
            uint8_t* p = in.p + 64 * k;
            build(p, 0, 0xC6336407u, 443, 10);
            std::memcpy(p + 30, kPool + (k == 1 ? 4 : 0), 4);  // (entry 19 is never taken)
            if (k == 2) p[33] = 99;
            put16(p + 36, k == 1 ? kHi : kLo);
            inh[k] = 3, ity[k] = PKT_HDR_ETHER, ity[3 + k] = PKT_HDR_IPV4, ity[6 + k] = PKT_HDR_TCP, iof[3 + k] = 14, iof[6 + k] = 34;
        }
        pkt_batch_t ib{};
        ib.slab = in.p, ib.slab_len = 3 * 64, ib.stride = 64, ib.n = 3;
        pkt_chain_t ich{inh.p, ity.p, iof.p};
        Outs o(3);
        if (pkt_nat_batch(t, &ib, &ich, PKT_FLOW_LAST, 0, PKT_NAT_IN, nullptr, nullptr, 200, o.status.p, o.entry.p, o.created.p, nullptr,
                          nullptr, nullptr) != PKT_SUCCESS)
            die("inbound", 0);
        if (o.status[0] != PKT_NAT_OK || o.status[1] != PKT_NAT_NO_SESSION || o.status[2] != PKT_NAT_NOT_OURS) die("inbound status", 0);
        if (o.entry[0] != 0 || in[30] != 10) die("inbound rewrite", 0);
    }
    // ---- the refusals leave everything alone
    Outs o(n);
    std::memcpy(slab.p, before.p, pos);
    expect_refusal(pkt_nat_batch(t, nullptr, &ch, 0, 0, 0, nullptr, nullptr, 0, o.status.p, nullptr, nullptr, nullptr, nullptr, nullptr), t,
                   "pkt_nat_batch: null argument", 0);
    expect_refusal(pkt_nat_batch(t, &b, &ch, 16, 0, 0, nullptr, nullptr, 0, o.status.p, nullptr, nullptr, nullptr, nullptr, nullptr), t,
                   "pkt_nat_batch: which_ip is neither below 16 nor PKT_FLOW_LAST", 1);
    expect_refusal(pkt_nat_batch(t, &b, &ch, 0, 2, 0, nullptr, nullptr, 0, o.status.p, nullptr, nullptr, nullptr, nullptr, nullptr), t,
                   "pkt_nat_batch: unknown flag bits", 2);
    expect_refusal(pkt_nat_batch(t, &b, &ch, 0, 0, 2, nullptr, nullptr, 0, o.status.p, nullptr, nullptr, nullptr, nullptr, nullptr), t,
                   "pkt_nat_batch: dir_all is neither PKT_NAT_OUT nor PKT_NAT_IN", 3);
    expect_refusal(pkt_nat_batch(t, &b, &ch, 0, 0, 0, nullptr, nullptr, 0, o.status.p, nullptr, nullptr,
                                 reinterpret_cast<uint64_t*>(reinterpret_cast<uint8_t*>(o.hits.p) + 4), nullptr, nullptr),
                   t, "pkt_nat_batch: hits / bytes not 8-byte aligned", 4);
    pkt_chain_t bad{nh.p, nullptr, of.p};
    expect_refusal(pkt_nat_batch(t, &b, &bad, 0, 0, 0, nullptr, nullptr, 0, o.status.p, nullptr, nullptr, nullptr, nullptr, nullptr), t,
                   "pkt_nat_batch: null chain column", 5);
    pkt_batch_t nolens = b;
    nolens.lens = nullptr;
    expect_refusal(pkt_nat_batch(t, &nolens, &ch, 0, 0, 0, nullptr, nullptr, 0, o.status.p, nullptr, nullptr, nullptr, nullptr, nullptr), t,
                   "pkt_nat_batch: offsets without lens", 6);
    for (uint64_t i = 0; i < n; i++)
        if (o.status[i] != 0x77) die("a refusal wrote", i);
    if (std::memcmp(slab.p, before.p, pos) != 0) die("a refusal wrote the slab", 0);
    pkt_batch_t none = b;
    none.n = 0;
    if (pkt_nat_batch(t, &none, &ch, 0, 0, 0, nullptr, nullptr, 0, o.status.p, nullptr, nullptr, o.hits.p, nullptr, nullptr) != PKT_SUCCESS ||
        o.hits[0] != kFill64)
        die("n == 0", 0);
    if (pkt_nat_destroy(t) != PKT_SUCCESS) die("destroy", 0);
}

void create_refusals() {
    pkt_nat_t* t = nullptr;
    Block<uint8_t> pool(8);
    std::memcpy(pool.p, kPool, 8);
    struct {
        uint32_t naddr, lo, hi;
        uint64_t slots;
        const char* text;
    } cases[] = {{0, 1, 2, 64, "pkt_nat_create_host: naddr not in 1..64"},
                 {65, 1, 2, 64, "pkt_nat_create_host: naddr not in 1..64"},
                 {2, 0, 2, 64, "pkt_nat_create_host: ports not 1 <= port_lo <= port_hi <= 65535"},
                 {2, 3, 2, 64, "pkt_nat_create_host: ports not 1 <= port_lo <= port_hi <= 65535"},
                 {2, 3, 65536, 64, "pkt_nat_create_host: ports not 1 <= port_lo <= port_hi <= 65535"},
                 {2, 1, 2, 63, "pkt_nat_create_host: slots not a power of two in 64..2^26"},
                 {2, 1, 2, 1ull << 27, "pkt_nat_create_host: slots not a power of two in 64..2^26"}};
    uint64_t k = 0;
    for (const auto& c : cases) {
        if (pkt_nat_create_host(pool.p, c.naddr, c.lo, c.hi, c.slots, nullptr, 0, &t) != PKT_ERR_INVALID_ARG || t) die("create refusal", k);
        if (std::strcmp(pkt_nat_last_error(nullptr), c.text) != 0) die("create refusal text", k);
        k++;
    }
    std::memcpy(pool.p + 4, kPool, 4);
    if (pkt_nat_create_host(pool.p, 2, 1, 2, 64, nullptr, 0, &t) != PKT_ERR_INVALID_ARG ||
        std::strcmp(pkt_nat_last_error(nullptr), "pkt_nat_create_host: duplicate pool address") != 0)
        die("duplicate pool", 0);
    if (pkt_nat_create_host(nullptr, 2, 1, 2, 64, nullptr, 0, &t) != PKT_ERR_INVALID_ARG) die("null pool", 0);
    if (pkt_nat_create_host(pool.p, 1, 1, 2, 64, nullptr, 1, &t) != PKT_ERR_INVALID_ARG) die("null statics", 0);
    // the widest legal handle's neighbours: one address, the whole port range, the smallest table
    if (pkt_nat_create_host(pool.p, 1, 1, 65535, 64, nullptr, 0, &t) != PKT_SUCCESS) die("wide create", 0);
    uint64_t counts[3];
    if (pkt_nat_count(t, counts) != PKT_SUCCESS || counts[0] | counts[1] | counts[2]) die("wide count", 0);
    if (pkt_nat_destroy(t) != PKT_SUCCESS) die("wide destroy", 0);
}

}  // namespace

int main() {
    if (pkt_sizeof_nat_static() != sizeof(pkt_nat_static_t) || pkt_sizeof_nat_record() != sizeof(pkt_nat_record_t)) die("sizeof", 0);
    create_refusals();
    for (uint64_t n : {1ull, 2ull, 17ull, 64ull, 333ull}) drive(n);
    std::printf("nat OK\n");
    return 0;
}
