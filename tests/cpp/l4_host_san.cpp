// l4_host_san.cpp — pkt_l4_checksum_host (packet-rs_amd/csrc/pktgpu_host.cpp) under AddressSanitizer +
// UndefinedBehaviorSanitizer: a stand-alone program, no GPU.  Every slab is a heap block of exactly
// slab_len bytes, so a read past a packet's end (a segment summed to the padded word, an IP length taken
// on trust) is a report.  It drives TCP / UDP / ICMP over IPv4 and IPv6 at the edge payload lengths and
// every alignment, the last packet ending on the slab's last byte, IP lengths past the packet, packets
// clamped by the slab end, chains that point past the packet, UPDATE and NULL outputs; each result is
// checked against a word-by-word sum written here.
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
    std::printf("FAIL %s at packet %llu\n", what, (unsigned long long)i);
    std::exit(1);
}

struct Pkt {
    std::vector<uint8_t> bytes;
    uint32_t ip, l4;      // header offsets
    uint8_t ipt, l4t;     // header types
};

void put16(std::vector<uint8_t>& b, uint32_t at, uint32_t v) {
    b[at] = (uint8_t)(v >> 8);
    b[at + 1] = (uint8_t)v;
}

// Ether / IPv4 | IPv6 / TCP | UDP | ICMP / payload, random bytes, the IP lengths right
Pkt make(bool v6, uint8_t l4t, uint32_t pay) {
    Pkt p;
    const uint32_t iph = v6 ? 40 : 20, hs = l4t == PKT_HDR_TCP ? 20 : l4t == PKT_HDR_UDP ? 8 : 4;
    p.bytes.resize(14 + iph + hs + pay);
    for (auto& x : p.bytes) x = (uint8_t)rnd();
    p.ip = 14, p.l4 = 14 + iph, p.ipt = v6 ? PKT_HDR_IPV6 : PKT_HDR_IPV4, p.l4t = l4t;
    if (v6) {
        put16(p.bytes, 14 + 4, hs + pay);
    } else {
        put16(p.bytes, 14 + 2, 20 + hs + pay);
        put16(p.bytes, 14 + 6, 0x4000);
    }
    return p;
}

// the checksum of bytes [s, e) of p with the pseudo-header, the field at f taken as zero
uint32_t csum(const uint8_t* p, const Pkt& k, uint32_t s, uint32_t e, uint32_t f) {
    uint64_t sum = 0;
    const bool v4 = k.ipt == PKT_HDR_IPV4;
    const uint32_t proto = k.l4t == PKT_HDR_TCP ? 6 : k.l4t == PKT_HDR_UDP ? 17 : 58;
    if (!(v4 && k.l4t == PKT_HDR_ICMP)) {
        for (uint32_t j = v4 ? 12 : 8; j < (v4 ? 20u : 40u); j += 2) sum += (uint32_t)p[k.ip + j] << 8 | p[k.ip + j + 1];
        sum += proto + (e - s);
    }
    for (uint32_t j = s; j < e; j++) {
        if (j == f || j == f + 1) continue;
        sum += (j - s) % 2 ? p[j] : (uint32_t)p[j] << 8;
    }
    while (sum >> 16) sum = (sum & 0xFFFF) + (sum >> 16);
    uint32_t c = (uint32_t)~sum & 0xFFFF;
    return k.l4t == PKT_HDR_UDP && c == 0 ? 0xFFFF : c;
}

struct Batch {
    uint8_t* slab = nullptr;  // exactly slab_len bytes on the heap
    uint64_t slab_len = 0;
    std::vector<uint64_t> offs;
    std::vector<uint32_t> lens;
    std::vector<Pkt> pk;
    std::vector<uint8_t> nh, ty;
    std::vector<uint16_t> of;
    std::vector<uint8_t> want;  // the status each packet must get
    void add(const Pkt& p, uint32_t align, uint8_t st) {
        uint64_t at = (slab_len + 15) / 16 * 16 + align;
        slab = static_cast<uint8_t*>(std::realloc(slab, at + p.bytes.size()));
        for (uint64_t k = slab_len; k < at; k++) slab[k] = (uint8_t)rnd();
        std::memcpy(slab + at, p.bytes.data(), p.bytes.size());
        slab_len = at + p.bytes.size();
        offs.push_back(at), lens.push_back((uint32_t)p.bytes.size()), pk.push_back(p), want.push_back(st);
    }
    void chain() {
        const uint64_t n = offs.size();
        nh.assign(n, 3), ty.assign(PKT_MAX_HDRS * n, 0), of.assign(PKT_MAX_HDRS * n, 0);
        for (uint64_t i = 0; i < n; i++) {
            ty[0 * n + i] = PKT_HDR_ETHER;
            ty[1 * n + i] = pk[i].ipt, of[1 * n + i] = (uint16_t)pk[i].ip;
            ty[2 * n + i] = pk[i].l4t, of[2 * n + i] = (uint16_t)pk[i].l4;
        }
    }
    pkt_batch_t batch() const {
        pkt_batch_t b{};
        b.slab = slab, b.slab_len = slab_len, b.offsets = offs.data(), b.lens = lens.data(), b.n = offs.size();
        return b;
    }
};

void run(Batch& B, uint32_t which) {
    const uint64_t n = B.offs.size();
    const pkt_batch_t b = B.batch();
    const pkt_chain_t ch{B.nh.data(), B.ty.data(), B.of.data()};
    std::vector<uint16_t> calc(n), stored(n);
    std::vector<uint8_t> st(n), st2(n);
    if (pkt_l4_checksum_host(&b, &ch, which, 0, calc.data(), stored.data(), st.data()) != PKT_SUCCESS) die("rc", 0);
    for (uint64_t i = 0; i < n; i++) {
        const Pkt& k = B.pk[i];
        const uint8_t* p = B.slab + B.offs[i];
        uint8_t w = B.want[i];
        if (w <= PKT_L4_UNCHECKED) {
            const uint32_t e = k.ipt == PKT_HDR_IPV4 ? k.ip + ((uint32_t)p[k.ip + 2] << 8 | p[k.ip + 3])
                                                     : k.ip + 40 + ((uint32_t)p[k.ip + 4] << 8 | p[k.ip + 5]);
            const uint32_t f = k.l4 + (k.l4t == PKT_HDR_TCP ? 16 : k.l4t == PKT_HDR_UDP ? 6 : 2);
            const uint32_t c = csum(p, k, k.l4, e, f), s = (uint32_t)p[f] << 8 | p[f + 1];
            if (calc[i] != c) die("calc", i);
            if (stored[i] != s) die("stored", i);
            w = k.l4t == PKT_HDR_UDP && s == 0 ? (k.ipt == PKT_HDR_IPV4 ? PKT_L4_UNCHECKED : PKT_L4_BAD)
                : s == c || (s == 0xFFFF && c == 0) ? PKT_L4_OK : PKT_L4_BAD;
        } else if (calc[i] || stored[i]) {
            die("calc / stored of a packet that is not summed", i);
        }
        if (st[i] != w) die("status", i);
    }
    // NULL outputs, then UPDATE on a copy of the slab (again exactly slab_len bytes): only the field changes,
    // and a second pass reads OK
    if (pkt_l4_checksum_host(&b, &ch, which, 0, nullptr, nullptr, nullptr) != PKT_SUCCESS) die("rc", 1);
    if (pkt_l4_checksum_host(&b, &ch, which, 0, nullptr, nullptr, st2.data()) != PKT_SUCCESS || st2 != st) die("status alone", 0);
    Batch U = B;
    U.slab = static_cast<uint8_t*>(std::malloc(B.slab_len ? B.slab_len : 1));
    std::memcpy(U.slab, B.slab, B.slab_len);
    const pkt_batch_t ub = U.batch();
    if (pkt_l4_checksum_host(&ub, &ch, which, PKT_L4_UPDATE, nullptr, nullptr, st2.data()) != PKT_SUCCESS || st2 != st) die("update", 0);
    uint64_t diff = 0, expect = 0;
    for (uint64_t k = 0; k < B.slab_len; k++) diff += U.slab[k] != B.slab[k];
    for (uint64_t i = 0; i < n; i++)
        if (st[i] <= PKT_L4_UNCHECKED) expect += (calc[i] >> 8 != stored[i] >> 8) + ((calc[i] & 0xFF) != (stored[i] & 0xFF));
    if (diff != expect) die("bytes changed by UPDATE", diff);
    if (pkt_l4_checksum_host(&ub, &ch, which, 0, nullptr, nullptr, st2.data()) != PKT_SUCCESS) die("rc", 2);
    for (uint64_t i = 0; i < n; i++)
        if (st2[i] != (st[i] <= PKT_L4_UNCHECKED ? PKT_L4_OK : st[i])) die("status after UPDATE", i);
    std::free(U.slab);
}

}  // namespace

int main() {
    static const uint32_t kPay[] = {0, 1, 2, 15, 16, 17, 31, 32, 33, 1461, 4096};
    static const uint8_t kL4[] = {PKT_HDR_TCP, PKT_HDR_UDP, PKT_HDR_ICMP};
    // (1) every protocol pair at the edge lengths and every alignment; the last packet ends the slab
    {
        Batch B;
        for (uint32_t pay : kPay)
            for (uint8_t t : kL4)
                for (int v6 = 0; v6 < 2; v6++)
                    for (uint32_t al = 0; al < 16; al += pay > 100 ? 5 : 1) B.add(make(v6, t, pay), al, PKT_L4_OK);
        B.add(make(false, PKT_HDR_UDP, 1), 15, PKT_L4_OK);  // an odd tail on the slab's last byte
        B.chain();
        run(B, 0);
        run(B, PKT_L4_LAST);
        std::free(B.slab);
    }
    // (2) lengths that lie: IP lengths past the packet and short of the L4 header, fragments, packets cut by
    // the slab end, chains pointing past the packet, a list without L4 or without IP, n_hdrs 0 and 20
    {
        Batch B;
        Pkt p = make(false, PKT_HDR_TCP, 30);
        put16(p.bytes, 14 + 2, 20 + 20 + 31);
        B.add(p, 3, PKT_L4_SPAN);
        p = make(false, PKT_HDR_TCP, 30);
        put16(p.bytes, 14 + 2, 0xFFFF);
        B.add(p, 3, PKT_L4_SPAN);
        p = make(false, PKT_HDR_UDP, 30);
        put16(p.bytes, 14 + 2, 27);
        B.add(p, 9, PKT_L4_SPAN);
        p = make(true, PKT_HDR_UDP, 30);
        put16(p.bytes, 14 + 4, 0);
        B.add(p, 1, PKT_L4_SPAN);
        p = make(true, PKT_HDR_ICMP, 30);
        put16(p.bytes, 14 + 4, 0xFFFF);
        B.add(p, 1, PKT_L4_SPAN);
        p = make(false, PKT_HDR_UDP, 30);
        put16(p.bytes, 14 + 6, 0x2000);
        B.add(p, 0, PKT_L4_FRAGMENT);
        p = make(false, PKT_HDR_UDP, 30);
        put16(p.bytes, 14 + 6, 0x0001);
        B.add(p, 0, PKT_L4_FRAGMENT);
        p = make(false, PKT_HDR_UDP, 12);  // padded past total_len
        p.bytes.resize(60, 0xEE);
        B.add(p, 7, PKT_L4_OK);
        p = make(false, PKT_HDR_TCP, 8);   // the chain's L4 and IP offsets far past the packet
        p.l4 = 65000, p.ip = 64000;
        B.add(p, 2, PKT_L4_SPAN);
        p = make(false, PKT_HDR_TCP, 8);   // the L4 offset past the segment's end
        p.l4 = 14 + 20 + 28;
        B.add(p, 2, PKT_L4_SPAN);
        p = make(true, PKT_HDR_TCP, 8);    // the IP header runs past the packet
        p.ip = 50, p.l4 = 90;
        B.add(p, 2, PKT_L4_SPAN);
        p = make(false, PKT_HDR_TCP, 8);
        p.ipt = PKT_HDR_VLAN;
        B.add(p, 4, PKT_L4_NO_IP);
        p = make(false, PKT_HDR_TCP, 8);
        p.l4t = PKT_HDR_ARP;
        B.add(p, 4, PKT_L4_ABSENT);
        B.add(make(false, PKT_HDR_TCP, 8), 5, PKT_L4_ABSENT);   // n_hdrs 0, below
        B.add(make(false, PKT_HDR_TCP, 8), 5, PKT_L4_OK);       // n_hdrs 20: taken as 16
        B.add(make(false, PKT_HDR_TCP, 40), 6, PKT_L4_SPAN);    // cut by the slab end, below
        B.add(make(true, PKT_HDR_UDP, 40), 6, PKT_L4_SPAN);     // starts past the slab end, below
        B.chain();
        const uint64_t n = B.offs.size();
        B.nh[n - 4] = 0, B.nh[n - 3] = 20;
        B.slab_len = B.offs[n - 2] + 60;  // (the heap block is not shrunk in place: copy it to an exact one)
        uint8_t* exact = static_cast<uint8_t*>(std::malloc(B.slab_len));
        std::memcpy(exact, B.slab, B.slab_len);
        std::free(B.slab);
        B.slab = exact;
        B.lens[n - 1] = 0xFFFFFFFFu;
        run(B, 0);
        // a fixed-stride view of the same bytes with n running past the slab
        pkt_batch_t f{};
        f.slab = B.slab, f.slab_len = B.slab_len, f.stride = 61, f.n = B.slab_len / 61 + 3;
        std::vector<uint8_t> nh(f.n, 3), ty(PKT_MAX_HDRS * f.n, PKT_HDR_ETHER), st(f.n);
        std::vector<uint16_t> of(PKT_MAX_HDRS * f.n, 0);
        for (uint64_t i = 0; i < f.n; i++) {
            ty[1 * f.n + i] = i % 2 ? PKT_HDR_IPV4 : PKT_HDR_IPV6, of[1 * f.n + i] = (uint16_t)(rnd() % 70);
            ty[2 * f.n + i] = kL4[i % 3], of[2 * f.n + i] = (uint16_t)(rnd() % 90);
        }
        const pkt_chain_t ch{nh.data(), ty.data(), of.data()};
        if (pkt_l4_checksum_host(&f, &ch, 0, 0, nullptr, nullptr, st.data()) != PKT_SUCCESS) die("rc", 3);
        if (st[f.n - 1] != PKT_L4_SPAN) die("a slot past the slab", f.n - 1);
        // refusals
        const pkt_batch_t b = B.batch();
        const pkt_chain_t c2{B.nh.data(), B.ty.data(), B.of.data()};
        pkt_batch_t huge = b;
        huge.n = 1ull << 32;
        const pkt_chain_t nocol{B.nh.data(), nullptr, B.of.data()};
        if (pkt_l4_checksum_host(nullptr, &c2, 0, 0, nullptr, nullptr, nullptr) != PKT_ERR_INVALID_ARG ||
            pkt_l4_checksum_host(&b, nullptr, 0, 0, nullptr, nullptr, nullptr) != PKT_ERR_INVALID_ARG ||
            pkt_l4_checksum_host(&b, &nocol, 0, 0, nullptr, nullptr, nullptr) != PKT_ERR_INVALID_ARG ||
            pkt_l4_checksum_host(&huge, &c2, 0, 0, nullptr, nullptr, nullptr) != PKT_ERR_INVALID_ARG ||
            pkt_l4_checksum_host(&b, &c2, 16, 0, nullptr, nullptr, nullptr) != PKT_ERR_INVALID_ARG ||
            pkt_l4_checksum_host(&b, &c2, 0, 4, nullptr, nullptr, nullptr) != PKT_ERR_INVALID_ARG ||
            pkt_l4_checksum_host(&b, &c2, 0, PKT_L4_KEEP_ZERO_UDP, nullptr, nullptr, nullptr) != PKT_ERR_INVALID_ARG)
            die("refusals", 0);
        std::free(B.slab);
    }
    // (3) n == 0
    {
        pkt_batch_t e{};
        const pkt_chain_t ch{reinterpret_cast<const uint8_t*>(&e), reinterpret_cast<const uint8_t*>(&e),
                             reinterpret_cast<const uint16_t*>(&e)};
        if (pkt_l4_checksum_host(&e, &ch, 0, PKT_L4_UPDATE, nullptr, nullptr, nullptr) != PKT_SUCCESS) die("empty batch", 0);
    }
    std::printf("l4 OK\n");
    return 0;
}
