// reasm_host_san.cpp — pkt_reasm_host (packet-rs_amd/csrc/pktgpu_host.cpp with pktgpu_reasm.hpp: the classification,
// the joined header and the refusals the kernels share) under AddressSanitizer + UndefinedBehaviorSanitizer: a
// stand-alone program, no GPU.  Every array (slab, chain columns, select, every output) is a heap block of its exact
// size, so a read or write past one is a report.  Datagrams are cut into fragments of 8 to 480 bytes and all packets
// are shuffled; they lie at every source alignment 0..15, the last one ending on the slab's last byte; some chain
// columns are forged (an IP offset past the packet, n_hdrs of 255); the sizing pass gives out_cap and dst_len and the
// writing call gets exactly those: dst_len is exactly *bytes_out_total.  Every NULL-output combination runs; the
// overflow and the refusals leave what they must alone.  The outputs are checked against the datagrams that were cut.
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

// a source packet: a whole packet (dg < 0) or the fragment [s, s + len) of datagram dg
struct Pkt {
    int dg;
    uint32_t s, len, mf, ipo, pad;
    uint32_t kind;  // 0 plain, 1 ip offset forged (SPAN), 2 n_hdrs 255, 3 no ip entry, 4 deselected
};
struct Dgram {
    std::vector<uint8_t> pay;
    uint32_t nfrag = 0, broken = 0;
};

void drive(uint32_t ndg, uint32_t flags) {
    // ---- the datagrams and their fragments, then whole packets, shuffled
    std::vector<Dgram> dgs(ndg);
    std::vector<Pkt> pk;
    for (uint32_t d = 0; d < ndg; d++) {
        Dgram& D = dgs[d];
        D.pay.resize(9 + rnd() % 2000);
        for (auto& x : D.pay) x = (uint8_t)rnd();
        const uint32_t per = 8 * (1 + rnd() % 60);
        for (uint32_t s = 0; s < D.pay.size(); s += per) {
            const uint32_t len = s + per < D.pay.size() ? per : (uint32_t)D.pay.size() - s;
            Pkt p{(int)d, s, len, s + per < D.pay.size() ? 1u : 0u, rnd() % 3 ? 14u : 18u, rnd() % 4 ? 0u : rnd() % 9, 0};
            if (d % 5 == 3 && s == per) {  // the second fragment's chain is forged, or it is deselected
                p.kind = 1 + d % 4;
                D.broken = p.kind != 2;  // (n_hdrs of 255 is cut to 16: that fragment still takes part)
            }
            pk.push_back(p);
            D.nfrag++;
        }
        if (d % 3 == 0) pk.push_back(Pkt{-1, 0, 20 + rnd() % 300, 0, 14, 0, d % 6 == 0 ? 2u : 0u});
    }
    for (uint64_t k = pk.size(); k > 1; k--) std::swap(pk[k - 1], pk[rnd() % k]);
    const uint64_t n = pk.size();
    Block<uint64_t> offs(n);
    Block<uint32_t> lens(n);
    Block<uint8_t> nh(n), ty(PKT_MAX_HDRS * n), sel(n);
    Block<uint16_t> of(PKT_MAX_HDRS * n);
    std::memset(ty.p, 0, ty.n);
    std::memset(static_cast<void*>(of.p), 0, of.n * 2);
    uint64_t pos = 0;
    for (uint64_t i = 0; i < n; i++) {
        pos = (pos + 15) / 16 * 16 + i % 16;
        offs[i] = pos;
        lens[i] = pk[i].ipo + 20 + pk[i].len + pk[i].pad;
        pos += lens[i];
    }
    Block<uint8_t> slab(pos);  // the last packet ends at the slab's last byte
    for (uint64_t k = 0; k < pos; k++) slab[k] = (uint8_t)rnd();
    for (uint64_t i = 0; i < n; i++) {
        const Pkt& p = pk[i];
        uint8_t* ip = slab.p + offs[i] + p.ipo;
        const uint32_t L = 20 + p.len, w = p.dg < 0 ? 0u : (p.mf << 13 | p.s / 8);
        std::memset(ip, 0, 20);
        ip[0] = 0x45;
        ip[2] = (uint8_t)(L >> 8), ip[3] = (uint8_t)L;
        ip[4] = (uint8_t)(p.dg >> 8), ip[5] = (uint8_t)p.dg;
        ip[6] = (uint8_t)(w >> 8), ip[7] = (uint8_t)w;
        ip[8] = 64, ip[9] = 17;
        ip[12] = 10, ip[15] = (uint8_t)(p.dg < 0 ? 9 : 1), ip[16] = 11;
        const uint32_t c = ~sum1071(ip) & 0xFFFFu;
        ip[10] = (uint8_t)(c >> 8), ip[11] = (uint8_t)c;
        if (p.dg >= 0) std::memcpy(ip + 20, dgs[p.dg].pay.data() + p.s, p.len);
        uint32_t r = 0;
        ty[r * n + i] = PKT_HDR_ETHER, of[r * n + i] = 0, r++;
        if (p.ipo == 18) ty[r * n + i] = PKT_HDR_VLAN, of[r * n + i] = 14, r++;
        if (p.kind != 3) {
            ty[r * n + i] = PKT_HDR_IPV4;
            of[r * n + i] = (uint16_t)(p.kind == 1 ? 65530 : p.ipo);
            r++;
        }
        nh[i] = (uint8_t)(p.kind == 2 ? 255 : r);
        sel[i] = p.kind != 4;
    }
    pkt_batch_t b{};
    b.slab = slab.p, b.slab_len = pos, b.offsets = offs.p, b.lens = lens.p, b.n = n;
    const pkt_chain_t ch{nh.p, ty.p, of.p};

    // ---- the sizing pass, then the writing call with exactly what it said
    uint64_t tot = 0, cnt = 0;
    Block<uint8_t> st0(n);
    Block<uint32_t> ix0(n);
    if (pkt_reasm_host(&b, &ch, 0, flags | PKT_REASM_NO_WRITE, sel.p, st0.p, ix0.p, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr,
                       nullptr, nullptr, &tot, &cnt) != PKT_SUCCESS)
        die("sizing pass", n);
    const uint64_t cap = cnt ? cnt : 1;
    for (uint32_t mask = 0; mask < 256; mask += (n > 300 ? 37 : 1)) {
        Block<uint8_t> st(n), dst(tot), onh(cap), oty(PKT_MAX_HDRS * cap);
        Block<uint32_t> ix(n), ol(cap), si(cap), nf(cap);
        Block<uint64_t> oo(cap), hits(PKT_REASM_STATUS_COUNT);
        Block<uint16_t> oof(PKT_MAX_HDRS * cap);
        for (uint32_t s = 0; s < PKT_REASM_STATUS_COUNT; s++) hits[s] = 1000;
        const pkt_chain_t oc{mask & 16 ? nullptr : onh.p, mask & 32 ? nullptr : oty.p, mask & 64 ? nullptr : oof.p};
        if (((uintptr_t)dst.p & 15) != 0) die("malloc gave a dst that is not 16-byte aligned", 0);
        uint64_t t2 = 0, c2 = 0;
        const int rc = pkt_reasm_host(&b, &ch, 0, flags, sel.p, mask & 1 ? nullptr : st.p, mask & 2 ? nullptr : ix.p, dst.p, tot, cap,
                                      oo.p, ol.p, mask & 4 ? nullptr : si.p, mask & 8 ? nullptr : nf.p, &oc,
                                      mask & 128 ? nullptr : hits.p, &t2, &c2);
        if (rc != PKT_SUCCESS || t2 != tot || c2 != cnt) die("writing call", mask);
        if (mask) continue;
        // ---- mask 0: everything is there; compare with what was cut
        uint64_t nhits = 0, at = 0;
        for (uint32_t s = 0; s < PKT_REASM_STATUS_COUNT; s++) nhits += hits[s] - 1000;
        if (nhits != n) die("hits", nhits);
        std::vector<int64_t> last(ndg, -1);  // a datagram's last-arriving member
        for (uint64_t i = 0; i < n; i++)
            if (pk[i].dg >= 0 && (pk[i].kind == 0 || pk[i].kind == 2)) last[pk[i].dg] = (int64_t)i;
        for (uint64_t q = 0; q < cnt; q++) {
            if (oo[q] != at) die("layout", q);
            for (uint64_t z = ol[q]; z < (ol[q] + 15) / 16 * 16; z++)
                if (dst[at + z]) die("padding", q);
            at += (ol[q] + 15) / 16 * 16;
            if (q && si[q] <= si[q - 1]) die("order of the outputs", q);
        }
        if (at != tot) die("total", at);
        for (uint64_t i = 0; i < n; i++) {
            const Pkt& p = pk[i];
            if (st[i] != st0[i] || ix[i] != ix0[i]) die("sizing pass and writing call differ", i);
            const uint8_t want = p.kind == 4 ? PKT_REASM_SKIPPED : p.kind == 3 ? PKT_REASM_NO_IP : p.kind == 1 ? PKT_REASM_SPAN
                                 : p.dg < 0                                   ? PKT_REASM_WHOLE
                                 : dgs[p.dg].broken                           ? PKT_REASM_PENDING
                                 : dgs[p.dg].nfrag == 1                       ? PKT_REASM_WHOLE
                                                                              : PKT_REASM_JOINED;
            if (st[i] != want) die("status", i);
            const bool out = want == PKT_REASM_JOINED || (want == PKT_REASM_WHOLE && !(flags & PKT_REASM_ONLY_JOINED));
            if (!out) {
                if (ix[i] != PKT_REASM_NONE) die("out_index of a packet without output", i);
                continue;
            }
            const uint64_t q = ix[i];
            if (q >= cnt) die("out_index", i);
            const uint8_t* d = dst.p + oo[q];
            if (want == PKT_REASM_WHOLE) {
                if (si[q] != i || nf[q] != 1 || ol[q] != lens[i] || std::memcmp(d, slab.p + offs[i], lens[i]) != 0) die("WHOLE output", i);
                if (onh[q] != (nh[i] > PKT_MAX_HDRS ? PKT_MAX_HDRS : nh[i])) die("WHOLE rows", i);
                continue;
            }
            const Dgram& D = dgs[p.dg];
            if ((int64_t)si[q] != last[p.dg] || nf[q] != D.nfrag) die("owner / nfrag", i);
            if (p.s != 0) continue;  // the s = 0 member checks the output: its prefix, the header, every payload byte
            const uint32_t io = p.ipo;
            if (ol[q] != io + 20 + D.pay.size() || std::memcmp(d, slab.p + offs[i], io) != 0) die("prefix", i);
            if (be16(d + io + 2) != 20 + D.pay.size() || be16(d + io + 6) != 0 || sum1071(d + io) != 0xFFFF) die("joined header", i);
            if (std::memcmp(d + io + 12, slab.p + offs[i] + io + 12, 8) != 0 || d[io + 9] != 17) die("joined header", i);
            if (std::memcmp(d + io + 20, D.pay.data(), D.pay.size()) != 0) die("payload", i);
            if (onh[q] != (io == 18 ? 3 : 2) || oty[(onh[q] - 1) * cap + q] != PKT_HDR_IPV4 || oof[(onh[q] - 1) * cap + q] != io)
                die("out_chain", q);
        }
    }
    // ---- one output too few, 16 bytes too few: PKT_ERR_INVALID_ARG with both totals, nothing written outside
    if (cnt > 1) {
        for (int cause = 0; cause < 2; cause++) {
            const uint64_t c1 = cause == 0 ? cnt - 1 : cnt, d1 = cause == 1 ? tot - 16 : tot;
            Block<uint8_t> dst(d1);
            Block<uint32_t> ol(c1);
            Block<uint64_t> oo(c1);
            uint64_t t2 = 0, c2 = 0;
            if (pkt_reasm_host(&b, &ch, 0, flags, sel.p, nullptr, nullptr, dst.p, d1, c1, oo.p, ol.p, nullptr, nullptr, nullptr, nullptr,
                               &t2, &c2) != PKT_ERR_INVALID_ARG || t2 != tot || c2 != cnt)
                die("overflow", cause);
        }
    }
    // ---- refusals
    {
        Block<uint8_t> dst(64);
        Block<uint32_t> ol(4);
        Block<uint64_t> oo(4);
        uint64_t t2 = 9, c2 = 9;
        auto call = [&](const pkt_batch_t* bb, const pkt_chain_t* cc, uint32_t which, uint32_t fl, uint8_t* d, uint64_t c, uint64_t* o,
                        uint32_t* l, uint64_t* h) {
            return pkt_reasm_host(bb, cc, which, fl, nullptr, nullptr, nullptr, d, 64, c, o, l, nullptr, nullptr, nullptr, h, &t2, &c2);
        };
        const pkt_chain_t nocol{nh.p, nullptr, of.p};
        pkt_batch_t big = b;
        big.n = 1ull << 32;
        pkt_batch_t nolens = b;
        nolens.lens = nullptr;
        int bad = 0;
        bad += call(nullptr, &ch, 0, 0, dst.p, 4, oo.p, ol.p, nullptr) != PKT_ERR_INVALID_ARG;
        bad += call(&b, nullptr, 0, 0, dst.p, 4, oo.p, ol.p, nullptr) != PKT_ERR_INVALID_ARG;
        bad += call(&b, &nocol, 0, 0, dst.p, 4, oo.p, ol.p, nullptr) != PKT_ERR_INVALID_ARG;
        bad += call(&big, &ch, 0, 0, dst.p, 4, oo.p, ol.p, nullptr) != PKT_ERR_INVALID_ARG;
        bad += call(&nolens, &ch, 0, 0, dst.p, 4, oo.p, ol.p, nullptr) != PKT_ERR_INVALID_ARG;
        bad += call(&b, &ch, 16, 0, dst.p, 4, oo.p, ol.p, nullptr) != PKT_ERR_INVALID_ARG;
        bad += call(&b, &ch, 0, 4, dst.p, 4, oo.p, ol.p, nullptr) != PKT_ERR_INVALID_ARG;
        bad += call(&b, &ch, 0, 0, dst.p + 8, 4, oo.p, ol.p, nullptr) != PKT_ERR_INVALID_ARG;
        bad += call(&b, &ch, 0, 0, dst.p, 4, reinterpret_cast<uint64_t*>(dst.p + 4), ol.p, nullptr) != PKT_ERR_INVALID_ARG;
        bad += call(&b, &ch, 0, 0, dst.p, 4, oo.p, ol.p, reinterpret_cast<uint64_t*>(dst.p + 4)) != PKT_ERR_INVALID_ARG;
        bad += call(&b, &ch, 0, 0, nullptr, 4, oo.p, ol.p, nullptr) != PKT_ERR_INVALID_ARG;
        bad += call(&b, &ch, 0, 0, dst.p, 4, nullptr, ol.p, nullptr) != PKT_ERR_INVALID_ARG;
        bad += call(&b, &ch, 0, 0, dst.p, 4, oo.p, nullptr, nullptr) != PKT_ERR_INVALID_ARG;
        bad += call(&b, &ch, 0, 0, dst.p, 0, oo.p, ol.p, nullptr) != PKT_ERR_INVALID_ARG;
        bad += call(&b, &ch, 0, 0, dst.p, 1ull << 32, oo.p, ol.p, nullptr) != PKT_ERR_INVALID_ARG;
        if (bad || t2 || c2) die("refusals", (uint64_t)bad);
        for (uint64_t k = 0; k < 64; k++)
            if (dst[k] != 0x77) die("a refused call wrote dst", k);
    }
}

}  // namespace

int main() {
    drive(1, 0);
    drive(12, 0);
    drive(12, PKT_REASM_ONLY_JOINED);
    drive(150, 0);
    // n == 0: the empty tail alone
    {
        pkt_batch_t b{};
        const pkt_chain_t ch{nullptr, nullptr, nullptr};
        Block<uint8_t> dst(16), onh(3);
        Block<uint32_t> ol(3), si(3), nf(3);
        Block<uint64_t> oo(3);
        const pkt_chain_t oc{onh.p, nullptr, nullptr};
        uint64_t t = 5, c = 5;
        if (pkt_reasm_host(&b, &ch, 0, 0, nullptr, nullptr, nullptr, dst.p, 16, 3, oo.p, ol.p, si.p, nf.p, &oc, nullptr, &t, &c) !=
                PKT_SUCCESS || t || c)
            die("n == 0", 0);
        for (int k = 0; k < 3; k++)
            if (oo[k] || ol[k] || si[k] != PKT_REASM_NONE || nf[k] || onh[k]) die("empty tail", (uint64_t)k);
    }
    std::printf("reasm OK\n");
    return 0;
}
