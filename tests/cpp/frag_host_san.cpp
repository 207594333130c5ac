// frag_host_san.cpp — pkt_frag_host (packet-rs_amd/csrc/pktgpu_host.cpp with pktgpu_frag.hpp: the decision, the
// fragment header and the refusals the kernels share) under AddressSanitizer + UndefinedBehaviorSanitizer: a
// stand-alone program, no GPU.  Every array (slab, chain columns, mtus, select, every output) is a heap block of its
// exact size, so a read or write past one is a report.  Packets lie at every source alignment 0..15, the last one
// ending on the slab's last byte; some chain columns are forged (an IP offset past the packet, n_hdrs of 255); the
// sizing pass gives out_cap and dst_len and the writing call gets exactly those: dst_len is exactly
// *bytes_out_total.  Every NULL-output combination runs; the overflow and the refusals leave what they must alone.
// The outputs are checked by putting the fragments together again.
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

uint32_t sum1071(const uint8_t* h) {
    uint32_t s = 0;
    for (int k = 0; k < 20; k += 2) s += be16(h + k);
    while (s >> 16) s = (s & 0xFFFFu) + (s >> 16);
    return s;
}

constexpr uint16_t kMtus[4] = {28, 68, 576, 1500};

void drive(uint64_t n, uint32_t flags_extra) {
    // ---- packets: Ether / [Vlan] / IPv4 / payload, packet i at alignment i % 16
    Block<uint64_t> offs(n);
    Block<uint32_t> lens(n);
    Block<uint8_t> nh(n), ty(PKT_MAX_HDRS * n), sel(n);
    Block<uint16_t> of(PKT_MAX_HDRS * n), mtu(n);
    std::memset(ty.p, 0, ty.n);
    std::memset(static_cast<void*>(of.p), 0, of.n * 2);
    std::vector<uint32_t> ipo(n), kind(n);  // 0 plain, 1 v6, 2 DF, 3 ip offset forged, 4 n_hdrs 255, 5 no ip, 6 cut
    uint64_t pos = 0;
    for (uint64_t i = 0; i < n; i++) {
        kind[i] = i % 7 == 3 ? 1 : i % 11 == 5 ? 2 : i % 13 == 7 ? 3 : i % 17 == 9 ? 4 : i % 19 == 11 ? 5 : i % 23 == 13 && i + 1 < n ? 6 : 0;
        ipo[i] = i % 2 ? 18 : 14;
        const uint32_t pay = 8 + rnd() % 1800;
        uint32_t len = ipo[i] + (kind[i] == 1 ? 40 : 20) + pay + (i % 5 == 0 ? rnd() % 9 : 0);
        if (kind[i] == 6) len = ipo[i] + 20 + pay / 2;
        pos = (pos + 15) / 16 * 16 + i % 16;
        offs[i] = pos;
        lens[i] = len;
        pos += len;
        mtu[i] = kMtus[rnd() % 4];
        sel[i] = i % 9 != 4;
    }
    Block<uint8_t> slab(pos);  // the last packet ends at the slab's last byte
    for (uint64_t k = 0; k < pos; k++) slab[k] = (uint8_t)rnd();
    for (uint64_t i = 0; i < n; i++) {
        uint8_t* ip = slab.p + offs[i] + ipo[i];
        const uint32_t room = lens[i] - ipo[i];
        if (kind[i] == 1) {
            ip[0] = 0x60;
            ip[4] = (uint8_t)((room - 40) >> 8), ip[5] = (uint8_t)(room - 40);
        } else {
            const uint32_t L = kind[i] == 6 ? room * 2 - 20 : room - (i % 5 == 0 ? (lens[i] - ipo[i] - 20) % 3 : 0);
            ip[0] = 0x45;
            ip[2] = (uint8_t)(L >> 8), ip[3] = (uint8_t)L;
            ip[6] = (uint8_t)((kind[i] == 2 ? 0x40 : 0) | (i % 4 == 1 ? 0x20 : 0));
            ip[7] = (uint8_t)(i % 4 == 1 ? 37 : 0);
        }
        uint32_t r = 0;
        ty[r * n + i] = PKT_HDR_ETHER, of[r * n + i] = 0, r++;
        if (ipo[i] == 18) ty[r * n + i] = PKT_HDR_VLAN, of[r * n + i] = 14, r++;
        if (kind[i] != 5) {
            ty[r * n + i] = kind[i] == 1 ? PKT_HDR_IPV6 : PKT_HDR_IPV4;
            of[r * n + i] = (uint16_t)(kind[i] == 3 ? 65530 : ipo[i]);
            r++;
        }
        ty[r * n + i] = PKT_HDR_UDP, of[r * n + i] = (uint16_t)(ipo[i] + 20), r++;
        nh[i] = (uint8_t)(kind[i] == 4 ? 255 : r);
    }
    pkt_batch_t b{};
    b.slab = slab.p, b.slab_len = pos, b.offsets = offs.p, b.lens = lens.p, b.n = n;
    const pkt_chain_t ch{nh.p, ty.p, of.p};
    const uint32_t flags = flags_extra;

    // ---- the sizing pass, then the writing call with exactly what it said
    uint64_t tot = 0, cnt = 0;
    Block<uint8_t> st0(n);
    Block<uint32_t> nf0(n), fi0(n);
    if (pkt_frag_host(&b, &ch, 0, flags | PKT_FRAG_NO_WRITE, mtu.p, 0, sel.p, st0.p, nf0.p, fi0.p, nullptr, 0, 0, nullptr, nullptr,
                      nullptr, nullptr, nullptr, nullptr, &tot, &cnt) != PKT_SUCCESS)
        die("sizing pass", n);
    const uint64_t cap = cnt ? cnt : 1;
    for (uint32_t mask = 0; mask < 512; mask += (n > 200 ? 73 : 1)) {
        Block<uint8_t> st(n), dst(tot), onh(cap), oty(PKT_MAX_HDRS * cap);
        Block<uint32_t> nf(n), fi(n), ol(cap), si(cap);
        Block<uint64_t> oo(cap), hits(PKT_FRAG_STATUS_COUNT);
        Block<uint16_t> fx(cap), oof(PKT_MAX_HDRS * cap);
        for (uint32_t s = 0; s < PKT_FRAG_STATUS_COUNT; s++) hits[s] = 1000;
        const pkt_chain_t oc{mask & 32 ? nullptr : onh.p, mask & 64 ? nullptr : oty.p, mask & 128 ? nullptr : oof.p};
        if (((uintptr_t)dst.p & 15) != 0) die("malloc gave a dst that is not 16-byte aligned", 0);
        uint64_t t2 = 0, c2 = 0;
        const int rc = pkt_frag_host(&b, &ch, 0, flags, mtu.p, 0, sel.p, mask & 1 ? nullptr : st.p, mask & 2 ? nullptr : nf.p,
                                     mask & 4 ? nullptr : fi.p, dst.p, tot, cap, oo.p, ol.p, mask & 8 ? nullptr : si.p,
                                     mask & 16 ? nullptr : fx.p, &oc, mask & 256 ? nullptr : hits.p, &t2, &c2);
        if (rc != PKT_SUCCESS || t2 != tot || c2 != cnt) die("writing call", mask);
        if (mask) continue;
        // ---- mask 0: everything is there; put the fragments together again
        uint64_t q = 0, at = 0, nhits = 0;
        for (uint32_t s = 0; s < PKT_FRAG_STATUS_COUNT; s++) nhits += hits[s] - 1000;
        if (nhits != n) die("hits", nhits);
        for (uint64_t i = 0; i < n; i++) {
            if (st[i] != st0[i] || nf[i] != nf0[i] || fi[i] != fi0[i]) die("sizing pass and writing call differ", i);
            const uint8_t* p = slab.p + offs[i];
            if (!sel[i] && st[i] != PKT_FRAG_SKIPPED) die("select", i);
            if (sel[i] && kind[i] == 5 && st[i] != PKT_FRAG_NO_IP) die("no ip", i);
            if (sel[i] && kind[i] == 3 && st[i] != PKT_FRAG_SPAN) die("span", i);
            if (nf[i] == 0) {
                if (fi[i] != PKT_FRAG_NONE) die("first of a packet without outputs", i);
                continue;
            }
            if (fi[i] != q) die("first", i);
            if (st[i] == PKT_FRAG_FITS) {
                if (nf[i] != 1 || ol[q] != lens[i] || oo[q] != at || std::memcmp(dst.p + at, p, lens[i]) != 0) die("FITS output", i);
                if (si[q] != i || fx[q] != 0 || onh[q] != (nh[i] > PKT_MAX_HDRS ? PKT_MAX_HDRS : nh[i])) die("FITS row", i);
                for (uint64_t z = lens[i]; z < (lens[i] + 15) / 16 * 16; z++)
                    if (dst[at + z]) die("padding", i);
                at += (lens[i] + 15) / 16 * 16;
                q++;
                continue;
            }
            if (st[i] != PKT_FRAG_SPLIT || nf[i] < 2) die("status of a packet with outputs", i);
            const uint32_t io = ipo[i], L = be16(p + io + 2), m = mtu[i];
            uint32_t got = 0, off8 = be16(p + io + 6) & 0x1FFFu;
            for (uint32_t j = 0; j < nf[i]; j++, q++) {
                const uint8_t* d = dst.p + at;
                if (oo[q] != at || si[q] != i || fx[q] != j) die("fragment row", q);
                const uint32_t pay = ol[q] - io - 20;
                if (be16(d + io + 2) != 20 + pay || 20 + pay > m || (j + 1 < nf[i] && pay % 8)) die("fragment length", q);
                if (std::memcmp(d, p, io) != 0) die("prefix", q);
                if (std::memcmp(d + io + 20, p + io + 20 + got, pay) != 0) die("payload", q);
                if ((be16(d + io + 6) & 0x1FFFu) != off8) die("fragment offset", q);
                const bool mf = be16(d + io + 6) & 0x2000u;
                if (mf != (j + 1 < nf[i] || (p[io + 6] & 0x20))) die("more fragments", q);
                if (sum1071(d + io) != sum1071(p + io)) die("checksum moved", q);
                if (onh[q] != (io == 18 ? 3 : 2) || oty[(onh[q] - 1) * cap + q] != PKT_HDR_IPV4 || oof[(onh[q] - 1) * cap + q] != io)
                    die("out_chain", q);
                for (uint64_t z = ol[q]; z < (ol[q] + 15) / 16 * 16; z++)
                    if (d[z]) die("padding", q);
                got += pay;
                off8 += pay / 8;
                at += (ol[q] + 15) / 16 * 16;
            }
            if (got != L - 20) die("payload bytes", i);
        }
        if (q != cnt || at != tot) die("totals", q);
    }
    // ---- one output too few, 16 bytes too few: PKT_ERR_INVALID_ARG with both totals, nothing written outside
    if (cnt > 1 && !(flags & PKT_FRAG_NO_WRITE)) {
        for (int cause = 0; cause < 2; cause++) {
            const uint64_t c1 = cause == 0 ? cnt - 1 : cnt, d1 = cause == 1 ? tot - 16 : tot;
            Block<uint8_t> dst(d1);
            Block<uint32_t> ol(c1);
            Block<uint64_t> oo(c1);
            uint64_t t2 = 0, c2 = 0;
            if (pkt_frag_host(&b, &ch, 0, flags, mtu.p, 0, sel.p, nullptr, nullptr, nullptr, dst.p, d1, c1, oo.p, ol.p, nullptr, nullptr,
                              nullptr, nullptr, &t2, &c2) != PKT_ERR_INVALID_ARG || t2 != tot || c2 != cnt)
                die("overflow", cause);
        }
    }
    // ---- refusals
    {
        Block<uint8_t> dst(64);
        Block<uint32_t> ol(4);
        Block<uint64_t> oo(4);
        uint64_t t2 = 9, c2 = 9;
        auto call = [&](const pkt_batch_t* bb, const pkt_chain_t* cc, uint32_t which, uint32_t fl, const uint16_t* mt, uint32_t mall,
                        uint8_t* d, uint64_t c, uint64_t* o, uint32_t* l, uint64_t* h) {
            return pkt_frag_host(bb, cc, which, fl, mt, mall, nullptr, nullptr, nullptr, nullptr, d, 64, c, o, l, nullptr, nullptr, nullptr,
                                 h, &t2, &c2);
        };
        const pkt_chain_t nocol{nh.p, nullptr, of.p};
        pkt_batch_t big = b;
        big.n = 1ull << 32;
        pkt_batch_t nolens = b;
        nolens.lens = nullptr;
        int bad = 0;
        bad += call(nullptr, &ch, 0, 0, nullptr, 576, dst.p, 4, oo.p, ol.p, nullptr) != PKT_ERR_INVALID_ARG;
        bad += call(&b, nullptr, 0, 0, nullptr, 576, dst.p, 4, oo.p, ol.p, nullptr) != PKT_ERR_INVALID_ARG;
        bad += call(&b, &nocol, 0, 0, nullptr, 576, dst.p, 4, oo.p, ol.p, nullptr) != PKT_ERR_INVALID_ARG;
        bad += call(&big, &ch, 0, 0, nullptr, 576, dst.p, 4, oo.p, ol.p, nullptr) != PKT_ERR_INVALID_ARG;
        bad += call(&nolens, &ch, 0, 0, nullptr, 576, dst.p, 4, oo.p, ol.p, nullptr) != PKT_ERR_INVALID_ARG;
        bad += call(&b, &ch, 16, 0, nullptr, 576, dst.p, 4, oo.p, ol.p, nullptr) != PKT_ERR_INVALID_ARG;
        bad += call(&b, &ch, 0, 4, nullptr, 576, dst.p, 4, oo.p, ol.p, nullptr) != PKT_ERR_INVALID_ARG;
        bad += call(&b, &ch, 0, 0, nullptr, 65536, dst.p, 4, oo.p, ol.p, nullptr) != PKT_ERR_INVALID_ARG;
        bad += call(&b, &ch, 0, 0, reinterpret_cast<const uint16_t*>(sel.p + 1), 0, dst.p, 4, oo.p, ol.p, nullptr) != PKT_ERR_INVALID_ARG;
        bad += call(&b, &ch, 0, 0, nullptr, 576, dst.p + 8, 4, oo.p, ol.p, nullptr) != PKT_ERR_INVALID_ARG;
        bad += call(&b, &ch, 0, 0, nullptr, 576, dst.p, 4, reinterpret_cast<uint64_t*>(dst.p + 4), ol.p, nullptr) != PKT_ERR_INVALID_ARG;
        bad += call(&b, &ch, 0, 0, nullptr, 576, dst.p, 4, oo.p, ol.p, reinterpret_cast<uint64_t*>(dst.p + 4)) != PKT_ERR_INVALID_ARG;
        bad += call(&b, &ch, 0, 0, nullptr, 576, nullptr, 4, oo.p, ol.p, nullptr) != PKT_ERR_INVALID_ARG;
        bad += call(&b, &ch, 0, 0, nullptr, 576, dst.p, 4, nullptr, ol.p, nullptr) != PKT_ERR_INVALID_ARG;
        bad += call(&b, &ch, 0, 0, nullptr, 576, dst.p, 4, oo.p, nullptr, nullptr) != PKT_ERR_INVALID_ARG;
        bad += call(&b, &ch, 0, 0, nullptr, 576, dst.p, 0, oo.p, ol.p, nullptr) != PKT_ERR_INVALID_ARG;
        bad += call(&b, &ch, 0, 0, nullptr, 576, dst.p, 1ull << 32, oo.p, ol.p, nullptr) != PKT_ERR_INVALID_ARG;
        if (bad || t2 || c2) die("refusals", (uint64_t)bad);
        for (uint64_t k = 0; k < 64; k++)
            if (dst[k] != 0x77) die("a refused call wrote dst", k);
    }
}

}  // namespace

int main() {
    drive(1, 0);
    drive(47, 0);
    drive(47, PKT_FRAG_ONLY_SPLIT);
    drive(700, 0);
    // n == 0: the empty tail alone
    {
        pkt_batch_t b{};
        const pkt_chain_t ch{nullptr, nullptr, nullptr};
        Block<uint8_t> dst(16), onh(3);
        Block<uint32_t> ol(3), si(3);
        Block<uint64_t> oo(3);
        Block<uint16_t> fx(3);
        const pkt_chain_t oc{onh.p, nullptr, nullptr};
        uint64_t t = 5, c = 5;
        if (pkt_frag_host(&b, &ch, 0, 0, nullptr, 576, nullptr, nullptr, nullptr, nullptr, dst.p, 16, 3, oo.p, ol.p, si.p, fx.p, &oc, nullptr,
                          &t, &c) != PKT_SUCCESS || t || c)
            die("n == 0", 0);
        for (int k = 0; k < 3; k++)
            if (oo[k] || ol[k] || si[k] != PKT_FRAG_NONE || fx[k] || onh[k]) die("empty tail", (uint64_t)k);
    }
    std::printf("frag OK\n");
    return 0;
}
