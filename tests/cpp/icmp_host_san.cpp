// icmp_host_san.cpp — pkt_icmp_err_host (packet-rs_amd/csrc/pktgpu_host.cpp with pktgpu_icmp.hpp: the find step, the
// decision, the header builders and the refusals the kernels share) under AddressSanitizer +
// UndefinedBehaviorSanitizer: a stand-alone program, no GPU.  Every array (slab, chain columns, codes, mtus, select,
// the map, every output) is a heap block of its exact size, so a read or write past one is a report.  Packets lie at
// every source alignment 0..15, the last one ending on the slab's last byte; some chain columns are forged (an Ether
// entry after the IP entry, offsets past the packet, n_hdrs of 255); the sizing pass gives out_cap and dst_len and the
// writing call gets exactly those: dst_len is exactly *bytes_out_total.  Every NULL-output combination runs; the
// overflow and the refusals leave what they must alone.  The outputs are checked by their own sums and against the
// source bytes.
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

uint32_t be16(const uint8_t* p) { return (uint32_t)p[0] << 8 | p[1]; }

// RFC 1071 over k bytes, on top of s
uint32_t sum1071(const uint8_t* h, uint32_t k, uint32_t s = 0) {
    for (uint32_t j = 0; j < k; j += 2) s += (uint32_t)h[j] << 8 | (j + 1 < k ? h[j + 1] : 0);
    while (s >> 16) s = (s & 0xFFFFu) + (s >> 16);
    return s;
}

pkt_icmp_cfg_t make_cfg(bool v4, bool v6) {
    pkt_icmp_cfg_t c{};
    if (v4) c.src4[0] = 192, c.src4[2] = 2, c.src4[3] = 1;
    if (v6) c.src6[0] = 0x20, c.src6[1] = 0x01, c.src6[15] = 1;
    c.ident = 0xFFF8;
    return c;
}

// kinds: 0 plain, 1 Ether after IP (forged), 2 IP offset past the packet (forged), 3 n_hdrs 255, 4 no ip, 5 cut record,
// 6 Ether offset past the IP entry (forged)
void drive(uint64_t n, bool with_map) {
    Block<uint64_t> offs(n);
    Block<uint32_t> lens(n);
    Block<uint8_t> nh(n), ty(PKT_MAX_HDRS * n), sel(n), code(n), map(256);
    Block<uint16_t> of(PKT_MAX_HDRS * n), mtu(n);
    std::memset(ty.p, 0, ty.n);
    std::memset(static_cast<void*>(of.p), 0, of.n * 2);
    std::memset(map.p, 0, 256);
    map[5] = 1, map[9] = 2, map[6] = 3, map[77] = 200;
    std::vector<uint32_t> ipo(n), kind(n), v6(n);
    uint64_t pos = 0;
    for (uint64_t i = 0; i < n; i++) {
        kind[i] = i % 11 == 5 ? 1 : i % 13 == 7 ? 2 : i % 17 == 9 ? 3 : i % 19 == 11 ? 4 : i % 23 == 13 && i + 1 < n ? 5 : i % 29 == 3 ? 6 : 0;
        v6[i] = i % 3 == 1;
        ipo[i] = 14 + 4 * (i % 3);
        const uint32_t pay = 8 + rnd() % 1800;
        uint32_t len = ipo[i] + (v6[i] ? 40 : 20) + pay + (i % 5 == 0 ? rnd() % 9 : 0);
        if (kind[i] == 5) len = ipo[i] + (v6[i] ? 40 : 20) + pay / 2;
        pos = (pos + 15) / 16 * 16 + i % 16;
        offs[i] = pos;
        lens[i] = len;
        pos += len;
        mtu[i] = (uint16_t)(576 + rnd() % 9000);
        sel[i] = i % 9 != 4;
        code[i] = with_map ? (uint8_t)(i % 31 == 7 ? 77 : i % 4 == 0 ? 5 : i % 4 == 1 ? 9 : i % 4 == 2 ? 6 : 0) : (uint8_t)(i % 8);
    }
    Block<uint8_t> slab(pos);  // the last packet ends at the slab's last byte
    for (uint64_t k = 0; k < pos; k++) slab[k] = (uint8_t)rnd();
    for (uint64_t i = 0; i < n; i++) {
        uint8_t* e = slab.p + offs[i];
        uint8_t* ip = e + ipo[i];
        e[0] &= 0xFE;  // a unicast destination
        const uint32_t H = v6[i] ? 40 : 20, room = lens[i] - ipo[i];
        const uint32_t L = kind[i] == 5 ? room * 2 : room - (i % 5 == 0 ? room % 3 : 0);
        if (v6[i]) {
            ip[0] = 0x60;
            ip[4] = (uint8_t)((L - 40) >> 8), ip[5] = (uint8_t)(L - 40);
            ip[6] = 17;
            ip[8] = 0x20, ip[24] = 0x20;
        } else {
            ip[0] = 0x45;
            ip[2] = (uint8_t)(L >> 8), ip[3] = (uint8_t)L;
            ip[6] = (uint8_t)(i % 4 == 1 ? 0x20 : 0), ip[7] = 0;
            ip[9] = 17;
            ip[12] = 10, ip[16] = 198;
        }
        uint32_t r = 0;
        if (kind[i] != 1) ty[r * n + i] = PKT_HDR_ETHER, of[r * n + i] = (uint16_t)(kind[i] == 6 ? ipo[i] - 3 : 0), r++;
        for (uint32_t k = 0; k < i % 3; k++) ty[r * n + i] = PKT_HDR_VLAN, of[r * n + i] = (uint16_t)(14 + 4 * k), r++;
        if (kind[i] != 4) {
            ty[r * n + i] = v6[i] ? PKT_HDR_IPV6 : PKT_HDR_IPV4;
            of[r * n + i] = (uint16_t)(kind[i] == 2 ? 65530 : ipo[i]);
            r++;
        }
        if (kind[i] == 1) ty[r * n + i] = PKT_HDR_ETHER, of[r * n + i] = 0, r++;
        ty[r * n + i] = PKT_HDR_UDP, of[r * n + i] = (uint16_t)(ipo[i] + H), r++;
        nh[i] = (uint8_t)(kind[i] == 3 ? 255 : r);
    }
    pkt_batch_t b{};
    b.slab = slab.p, b.slab_len = pos, b.offsets = offs.p, b.lens = lens.p, b.n = n;
    const pkt_chain_t ch{nh.p, ty.p, of.p};
    const pkt_icmp_cfg_t cfg = make_cfg(true, n != 47);  // one drive without an IPv6 source
    const uint8_t* mp = with_map ? map.p : nullptr;

    // ---- the sizing pass, then the writing call with exactly what it said
    uint64_t tot = 0, cnt = 0;
    Block<uint8_t> st0(n);
    Block<uint32_t> oi0(n);
    if (pkt_icmp_err_host(&b, &ch, 0, PKT_ICMPE_NO_WRITE, &cfg, code.p, 0, mp, mtu.p, 0, sel.p, st0.p, oi0.p, nullptr, 0, 0, nullptr,
                          nullptr, nullptr, nullptr, nullptr, &tot, &cnt) != PKT_SUCCESS)
        die("sizing pass", n);
    const uint64_t cap = cnt ? cnt : 1;
    for (uint32_t mask = 0; mask < 128; mask += (n > 200 ? 37 : 1)) {
        Block<uint8_t> st(n), dst(tot), onh(cap), oty(PKT_MAX_HDRS * cap);
        Block<uint32_t> oi(n), ol(cap), si(cap);
        Block<uint64_t> oo(cap), hits(PKT_ICMPE_STATUS_COUNT);
        Block<uint16_t> oof(PKT_MAX_HDRS * cap);
        for (uint32_t s = 0; s < PKT_ICMPE_STATUS_COUNT; s++) hits[s] = 1000;
        const pkt_chain_t oc{mask & 8 ? nullptr : onh.p, mask & 16 ? nullptr : oty.p, mask & 32 ? nullptr : oof.p};
        if (((uintptr_t)dst.p & 15) != 0) die("malloc gave a dst that is not 16-byte aligned", 0);
        uint64_t t2 = 0, c2 = 0;
        const int rc = pkt_icmp_err_host(&b, &ch, 0, 0, &cfg, code.p, 0, mp, mtu.p, 0, sel.p, mask & 1 ? nullptr : st.p,
                                         mask & 2 ? nullptr : oi.p, dst.p, tot, cap, oo.p, ol.p, mask & 4 ? nullptr : si.p, &oc,
                                         mask & 64 ? nullptr : hits.p, &t2, &c2);
        if (rc != PKT_SUCCESS || t2 != tot || c2 != cnt) die("writing call", mask);
        if (mask) continue;
        // ---- mask 0: everything is there
        uint64_t q = 0, at = 0, nhits = 0;
        for (uint32_t s = 0; s < PKT_ICMPE_STATUS_COUNT; s++) nhits += hits[s] - 1000;
        if (nhits != n) die("hits", nhits);
        for (uint64_t i = 0; i < n; i++) {
            if (st[i] != st0[i] || oi[i] != oi0[i]) die("sizing pass and writing call differ", i);
            const uint32_t r = with_map ? map[code[i]] : code[i];
            if ((!sel[i] || r == 0) && st[i] != PKT_ICMPE_SKIPPED) die("select / reason 0", i);
            if (sel[i] && r > 6 && st[i] != PKT_ICMPE_BAD_REASON) die("bad reason", i);
            const bool live = sel[i] && r >= 1 && r <= 6;
            if (live && kind[i] == 4 && st[i] != PKT_ICMPE_NO_IP) die("no ip", i);
            if (live && (kind[i] == 2 || kind[i] == 6) && st[i] != PKT_ICMPE_SPAN) die("span", i);
            if (live && kind[i] == 1 && st[i] != PKT_ICMPE_NO_ETHER) die("ether after ip", i);
            if (live && v6[i] && n == 47 && kind[i] != 4 && kind[i] != 2 && kind[i] != 1 && kind[i] != 6 && st[i] != PKT_ICMPE_NO_SRC)
                die("no src", i);
            if (st[i] != PKT_ICMPE_SENT) {
                if (oi[i] != PKT_ICMPE_NONE) die("out_index of a packet without an output", i);
                continue;
            }
            if (oi[i] != q || si[q] != i || oo[q] != at) die("output row", i);
            const uint8_t* p = slab.p + offs[i];
            const uint8_t* d = dst.p + at;
            const uint32_t io = ipo[i], H = v6[i] ? 40 : 20, Q = ol[q] - io - H - 8;
            if (std::memcmp(d, p + 6, 6) || std::memcmp(d + 6, p, 6) || std::memcmp(d + 12, p + 12, io - 12)) die("prefix", i);
            if (std::memcmp(d + io + H + 8, p + io, Q)) die("quote", i);
            if (Q > (v6[i] ? 1232u : 548u) || io + Q > lens[i]) die("quote length", i);
            if (v6[i]) {
                if (be16(d + io + 4) != 8 + Q || d[io + 6] != 58 || std::memcmp(d + io + 24, p + io + 8, 16)) die("ipv6 header", i);
                uint8_t ps[8] = {0, 0, (uint8_t)((8 + Q) >> 8), (uint8_t)(8 + Q), 0, 0, 0, 58};
                if (sum1071(d + io + H, 8 + Q, sum1071(ps, 8, sum1071(d + io + 8, 32))) != 0xFFFF) die("icmpv6 checksum", i);
            } else {
                if (be16(d + io + 2) != 28 + Q || d[io + 9] != 1 || std::memcmp(d + io + 16, p + io + 12, 4)) die("ipv4 header", i);
                if (be16(d + io + 4) != ((0xFFF8u + q) & 0xFFFFu)) die("identification", i);
                if (sum1071(d + io, 20) != 0xFFFF || sum1071(d + io + H, 8 + Q) != 0xFFFF) die("checksums", i);
            }
            const uint32_t rows = 2 + i % 3;
            if (onh[q] != rows + 1 || oty[rows * cap + q] != PKT_HDR_ICMP || oof[rows * cap + q] != io + H ||
                oty[(rows - 1) * cap + q] != (v6[i] ? PKT_HDR_IPV6 : PKT_HDR_IPV4) || oof[(rows - 1) * cap + q] != io)
                die("out_chain", i);
            for (uint64_t z = ol[q]; z < (ol[q] + 15) / 16 * 16; z++)
                if (d[z]) die("padding", i);
            at += (ol[q] + 15) / 16 * 16;
            q++;
        }
        if (q != cnt || at != tot) die("totals", q);
    }
    // ---- one output too few, 16 bytes too few: PKT_ERR_INVALID_ARG with both totals, nothing written outside
    if (cnt > 1) {
        for (int cause = 0; cause < 2; cause++) {
            const uint64_t c1 = cause == 0 ? cnt - 1 : cnt, d1 = cause == 1 ? tot - 16 : tot;
            Block<uint8_t> dst(d1);
            Block<uint32_t> ol(c1);
            Block<uint64_t> oo(c1);
            uint64_t t2 = 0, c2 = 0;
            if (pkt_icmp_err_host(&b, &ch, 0, 0, &cfg, code.p, 0, mp, mtu.p, 0, sel.p, nullptr, nullptr, dst.p, d1, c1, oo.p, ol.p,
                                  nullptr, nullptr, nullptr, &t2, &c2) != PKT_ERR_INVALID_ARG || t2 != tot || c2 != cnt)
                die("overflow", cause);
        }
    }
    // ---- refusals
    {
        Block<uint8_t> dst(64);
        Block<uint32_t> ol(4);
        Block<uint64_t> oo(4);
        uint64_t t2 = 9, c2 = 9;
        auto call = [&](const pkt_batch_t* bb, const pkt_chain_t* cc, uint32_t which, uint32_t fl, const pkt_icmp_cfg_t* cf,
                        uint32_t call_, const uint16_t* mt, uint32_t mall, uint8_t* d, uint64_t c, uint64_t* o, uint32_t* l,
                        uint64_t* h) {
            return pkt_icmp_err_host(bb, cc, which, fl, cf, nullptr, call_, nullptr, mt, mall, nullptr, nullptr, nullptr, d, 64, c, o, l,
                                     nullptr, nullptr, h, &t2, &c2);
        };
        const pkt_chain_t nocol{nh.p, nullptr, of.p};
        pkt_batch_t big = b;
        big.n = 1ull << 32;
        pkt_batch_t nolens = b;
        nolens.lens = nullptr;
        const pkt_icmp_cfg_t none = make_cfg(false, false);
        pkt_icmp_cfg_t m4 = cfg, m6 = cfg;
        m4.max4 = 55, m6.max6 = 95;
        int bad = 0;
        bad += call(nullptr, &ch, 0, 0, &cfg, 1, nullptr, 576, dst.p, 4, oo.p, ol.p, nullptr) != PKT_ERR_INVALID_ARG;
        bad += call(&b, nullptr, 0, 0, &cfg, 1, nullptr, 576, dst.p, 4, oo.p, ol.p, nullptr) != PKT_ERR_INVALID_ARG;
        bad += call(&b, &nocol, 0, 0, &cfg, 1, nullptr, 576, dst.p, 4, oo.p, ol.p, nullptr) != PKT_ERR_INVALID_ARG;
        bad += call(&big, &ch, 0, 0, &cfg, 1, nullptr, 576, dst.p, 4, oo.p, ol.p, nullptr) != PKT_ERR_INVALID_ARG;
        bad += call(&nolens, &ch, 0, 0, &cfg, 1, nullptr, 576, dst.p, 4, oo.p, ol.p, nullptr) != PKT_ERR_INVALID_ARG;
        bad += call(&b, &ch, 16, 0, &cfg, 1, nullptr, 576, dst.p, 4, oo.p, ol.p, nullptr) != PKT_ERR_INVALID_ARG;
        bad += call(&b, &ch, 0, 2, &cfg, 1, nullptr, 576, dst.p, 4, oo.p, ol.p, nullptr) != PKT_ERR_INVALID_ARG;
        bad += call(&b, &ch, 0, 0, nullptr, 1, nullptr, 576, dst.p, 4, oo.p, ol.p, nullptr) != PKT_ERR_INVALID_ARG;
        bad += call(&b, &ch, 0, 0, &none, 1, nullptr, 576, dst.p, 4, oo.p, ol.p, nullptr) != PKT_ERR_INVALID_ARG;
        bad += call(&b, &ch, 0, 0, &m4, 1, nullptr, 576, dst.p, 4, oo.p, ol.p, nullptr) != PKT_ERR_INVALID_ARG;
        bad += call(&b, &ch, 0, 0, &m6, 1, nullptr, 576, dst.p, 4, oo.p, ol.p, nullptr) != PKT_ERR_INVALID_ARG;
        bad += call(&b, &ch, 0, 0, &cfg, 256, nullptr, 576, dst.p, 4, oo.p, ol.p, nullptr) != PKT_ERR_INVALID_ARG;
        bad += call(&b, &ch, 0, 0, &cfg, 1, nullptr, 65536, dst.p, 4, oo.p, ol.p, nullptr) != PKT_ERR_INVALID_ARG;
        bad += call(&b, &ch, 0, 0, &cfg, 1, reinterpret_cast<const uint16_t*>(sel.p + 1), 0, dst.p, 4, oo.p, ol.p, nullptr) != PKT_ERR_INVALID_ARG;
        bad += call(&b, &ch, 0, 0, &cfg, 1, nullptr, 576, dst.p + 8, 4, oo.p, ol.p, nullptr) != PKT_ERR_INVALID_ARG;
        bad += call(&b, &ch, 0, 0, &cfg, 1, nullptr, 576, dst.p, 4, reinterpret_cast<uint64_t*>(dst.p + 4), ol.p, nullptr) != PKT_ERR_INVALID_ARG;
        bad += call(&b, &ch, 0, 0, &cfg, 1, nullptr, 576, dst.p, 4, oo.p, ol.p, reinterpret_cast<uint64_t*>(dst.p + 4)) != PKT_ERR_INVALID_ARG;
        bad += call(&b, &ch, 0, 0, &cfg, 1, nullptr, 576, nullptr, 4, oo.p, ol.p, nullptr) != PKT_ERR_INVALID_ARG;
        bad += call(&b, &ch, 0, 0, &cfg, 1, nullptr, 576, dst.p, 4, nullptr, ol.p, nullptr) != PKT_ERR_INVALID_ARG;
        bad += call(&b, &ch, 0, 0, &cfg, 1, nullptr, 576, dst.p, 4, oo.p, nullptr, nullptr) != PKT_ERR_INVALID_ARG;
        bad += call(&b, &ch, 0, 0, &cfg, 1, nullptr, 576, dst.p, 0, oo.p, ol.p, nullptr) != PKT_ERR_INVALID_ARG;
        bad += call(&b, &ch, 0, 0, &cfg, 1, nullptr, 576, dst.p, 1ull << 32, oo.p, ol.p, nullptr) != PKT_ERR_INVALID_ARG;
        if (bad || t2 || c2) die("refusals", (uint64_t)bad);
        for (uint64_t k = 0; k < 64; k++)
            if (dst[k] != 0x77) die("a refused call wrote dst", k);
    }
}

}  // namespace

int main() {
    drive(1, false);
    drive(47, false);
    drive(48, true);
    drive(700, true);
    // n == 0: the empty tail alone
    {
        pkt_batch_t b{};
        const pkt_chain_t ch{nullptr, nullptr, nullptr};
        const pkt_icmp_cfg_t cfg = make_cfg(true, true);
        Block<uint8_t> dst(16), onh(3);
        Block<uint32_t> ol(3), si(3);
        Block<uint64_t> oo(3);
        const pkt_chain_t oc{onh.p, nullptr, nullptr};
        uint64_t t = 5, c = 5;
        if (pkt_icmp_err_host(&b, &ch, 0, 0, &cfg, nullptr, 1, nullptr, nullptr, 576, nullptr, nullptr, nullptr, dst.p, 16, 3, oo.p, ol.p,
                              si.p, &oc, nullptr, &t, &c) != PKT_SUCCESS || t || c)
            die("n == 0", 0);
        for (int k = 0; k < 3; k++)
            if (oo[k] || ol[k] || si[k] != PKT_ICMPE_NONE || onh[k]) die("empty tail", (uint64_t)k);
    }
    std::printf("icmp OK\n");
    return 0;
}
