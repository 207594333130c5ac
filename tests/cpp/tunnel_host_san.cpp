// tunnel_host_san.cpp — the host handle and twins of pkt_tunnel_* (packet-rs_amd/csrc/pktgpu_host.cpp with
// pktgpu_tunnel.hpp: the table's checks and lookup, the search, both decisions, the header words, the rows and the
// refusals the kernels share) under AddressSanitizer + UndefinedBehaviorSanitizer: a stand-alone program, no GPU.
// Every array (entries, slab, chain columns, tunnel, entropy, select, outputs, counters) is a heap block of its exact
// size, so a read or write past one is a report.  Packets lie at every alignment 0..15, the last one ending on the
// slab's last byte; some chain columns are forged (offsets past the packet, n_hdrs of 255); every NULL-output
// combination runs with and without PKT_TUN_NO_WRITE; the refusals leave everything alone.  Checked here: the outer
// IPv4 and UDP checksums (summed again by RFC 1071), the length fields, and that decap(encap(x)) gives x back.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
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

// a 16-byte aligned heap block of exactly n bytes (dst)
struct Aligned {
    uint8_t* p;
    explicit Aligned(uint64_t n) : p(static_cast<uint8_t*>(std::aligned_alloc(16, n ? (n + 15) / 16 * 16 : 16))) {
        std::memset(p, 0x77, n ? (n + 15) / 16 * 16 : 16);
    }
    ~Aligned() { std::free(p); }
};

uint32_t ones_sum(const uint8_t* p, uint32_t n, uint32_t s = 0) {
    for (uint32_t k = 0; k < n; k += 2) s += (uint32_t)p[k] << 8 | (k + 1 < n ? p[k + 1] : 0);
    while (s >> 16) s = (s & 0xFFFFu) + (s >> 16);
    return s;
}
uint32_t be16(const uint8_t* p) { return (uint32_t)p[0] << 8 | p[1]; }
void put16(uint8_t* p, uint32_t v) { p[0] = (uint8_t)(v >> 8), p[1] = (uint8_t)v; }

constexpr uint32_t kN = 48, kRows = PKT_MAX_HDRS;

// Ether / [Vlan] / IPv4 or IPv6 / UDP with `tail` payload bytes; returns the length
uint32_t build(uint8_t* p, uint32_t i, bool v6, bool vlan, uint32_t tail) {
    uint32_t o = 0;
    for (uint32_t k = 0; k < 12; k++) p[o++] = (uint8_t)(0x10 + k + i);
    if (vlan) p[o++] = 0x81, p[o++] = 0, p[o++] = 0, p[o++] = 7;
    p[o++] = v6 ? 0x86 : 0x08, p[o++] = v6 ? 0xDD : 0x00;
    const uint32_t ul = 8 + tail;
    if (v6) {
        p[o] = 0x6A, p[o + 1] = 0xB0, p[o + 2] = p[o + 3] = 0;
        put16(p + o + 4, ul);
        p[o + 6] = 17, p[o + 7] = 64;
        for (uint32_t k = 0; k < 32; k++) p[o + 8 + k] = (uint8_t)(0x20 + k);
        o += 40;
    } else {
        p[o] = 0x45, p[o + 1] = 0xB8;
        put16(p + o + 2, 20 + ul);
        put16(p + o + 4, i), put16(p + o + 6, 0);
        p[o + 8] = 64, p[o + 9] = 17, p[o + 10] = p[o + 11] = 0;
        for (uint32_t k = 0; k < 8; k++) p[o + 12 + k] = (uint8_t)(10 + k);
        put16(p + o + 10, ~ones_sum(p + o, 20) & 0xFFFFu);
        o += 20;
    }
    put16(p + o, 1000 + i), put16(p + o + 2, 53), put16(p + o + 4, ul), put16(p + o + 6, 0);
    o += 8;
    for (uint32_t k = 0; k < tail; k++) p[o++] = (uint8_t)(k * 7 + i);
    return o;
}

pkt_tunnel_entry_t entry(uint32_t kind, uint32_t ipver, bool swap, uint32_t id, uint32_t flags) {
    pkt_tunnel_entry_t e;
    std::memset(&e, 0, sizeof e);
    e.kind = (uint8_t)kind, e.ipver = (uint8_t)ipver, e.tos = 3, e.flags = flags, e.id = id;
    e.sport_lo = 2000, e.sport_hi = 2999;
    for (uint32_t k = 0; k < 16; k++) {
        (swap ? e.dst : e.src)[k] = k < (ipver == 4 ? 4u : 16u) ? (uint8_t)(0xC0 + k) : 0;
        (swap ? e.src : e.dst)[k] = k < (ipver == 4 ? 4u : 16u) ? (uint8_t)(0xD0 + k) : 0;
    }
    for (uint32_t k = 0; k < 6; k++) e.eth_dst[k] = (uint8_t)(2 + k), e.eth_src[k] = (uint8_t)(0x42 + k);
    return e;
}

struct Outputs {
    Block<uint8_t> status;
    Block<uint32_t> out_index, tunnel_out, out_len, src_index;
    Block<uint64_t> out_off, hits;
    Block<uint8_t> oc_nh, oc_ty;
    Block<uint16_t> oc_of;
    Outputs(uint64_t n, uint64_t cap, uint32_t nst)
        : status(n), out_index(n), tunnel_out(n), out_len(cap), src_index(cap), out_off(cap), hits(nst), oc_nh(cap),
          oc_ty(kRows * cap), oc_of(kRows * cap) {
        for (uint32_t k = 0; k < nst; k++) hits[k] = 0;
    }
};

void expect_refusal(int rc, const pkt_tunnel_t* t, const char* text, uint64_t at) {
    if (rc != PKT_ERR_INVALID_ARG) die("a refusal's code", at);
    if (std::string(pkt_tunnel_last_error(t)) != text) {
        std::printf("got \"%s\"\n", pkt_tunnel_last_error(t));
        die("a refusal's text", at);
    }
}

}  // namespace

int main() {
    // ---- the table: 6 tunnels and the same as their other ends hold them
    const uint32_t kinds[6][3] = {{PKT_TUN_VXLAN, 4, PKT_TUN_F_UDP_CSUM | PKT_TUN_F_DF}, {PKT_TUN_VXLAN, 6, PKT_TUN_F_UDP_CSUM},
                                  {PKT_TUN_GRE, 4, PKT_TUN_F_KEY}, {PKT_TUN_GRE, 6, PKT_TUN_F_INHERIT_TOS},
                                  {PKT_TUN_IPIP, 4, 0}, {PKT_TUN_IPIP, 6, PKT_TUN_F_ANY_REMOTE}};
    Block<pkt_tunnel_entry_t> ents(12);
    for (uint32_t k = 0; k < 6; k++) {
        ents[k] = entry(kinds[k][0], kinds[k][1], false, 100 + k, kinds[k][2]);
        ents[6 + k] = entry(kinds[k][0], kinds[k][1], true, 100 + k, kinds[k][2]);
    }
    pkt_tunnel_t* tun = nullptr;
    if (pkt_tunnel_create_host(ents.p, 12, &tun) != PKT_SUCCESS) die(pkt_tunnel_last_error(nullptr), 0);
    if (pkt_sizeof_tunnel_entry() != 64) die("sizeof", 0);

    // ---- create refusals
    {
        pkt_tunnel_t* bad = nullptr;
        Block<pkt_tunnel_entry_t> two(2);
        const auto again = [&] { two[0] = entry(PKT_TUN_VXLAN, 4, false, 1, 0), two[1] = entry(PKT_TUN_VXLAN, 4, false, 2, 0); };
        again();
        expect_refusal(pkt_tunnel_create_host(nullptr, 2, &bad), nullptr, "pkt_tunnel_create: null entries", 1);
        expect_refusal(pkt_tunnel_create_host(two.p, 0, &bad), nullptr, "pkt_tunnel_create: count is 0 or above PKT_TUN_MAX_ENTRIES", 2);
        two[1].kind = 9;
        expect_refusal(pkt_tunnel_create_host(two.p, 2, &bad), nullptr, "pkt_tunnel_create: entry 1: unknown kind", 3);
        again(), two[1].ipver = 0;
        expect_refusal(pkt_tunnel_create_host(two.p, 2, &bad), nullptr, "pkt_tunnel_create: entry 1: ipver is neither 4 nor 6", 4);
        again(), two[0].flags = 0x100;
        expect_refusal(pkt_tunnel_create_host(two.p, 2, &bad), nullptr, "pkt_tunnel_create: entry 0: unknown flag bits", 5);
        again(), two[1].id = 1u << 24;
        expect_refusal(pkt_tunnel_create_host(two.p, 2, &bad), nullptr, "pkt_tunnel_create: entry 1: VNI above 2^24 - 1", 6);
        again(), two[1].sport_lo = 3000;
        expect_refusal(pkt_tunnel_create_host(two.p, 2, &bad), nullptr, "pkt_tunnel_create: entry 1: sport_lo above sport_hi", 7);
        again(), two[1].flags = PKT_TUN_F_KEY;
        expect_refusal(pkt_tunnel_create_host(two.p, 2, &bad), nullptr,
                       "pkt_tunnel_create: entry 1: PKT_TUN_F_KEY on an entry that is not GRE", 8);
        again(), two[1].kind = PKT_TUN_IPIP, two[1].flags = PKT_TUN_F_UDP_CSUM;
        expect_refusal(pkt_tunnel_create_host(two.p, 2, &bad), nullptr,
                       "pkt_tunnel_create: entry 1: PKT_TUN_F_UDP_CSUM on an entry that is not VXLAN", 9);
        again(), two[1].id = 1;
        expect_refusal(pkt_tunnel_create_host(two.p, 2, &bad), nullptr, "pkt_tunnel_create: entries 0 and 1 have the same decap key", 10);
        if (bad) die("a refused create left a handle", 0);
    }

    // ---- the batch: kN packets at every alignment, the last one ending on the slab's last byte
    std::vector<std::vector<uint8_t>> pk(kN);
    Block<uint64_t> offs(kN);
    Block<uint32_t> lens(kN);
    uint64_t pos = 0;
    for (uint32_t i = 0; i < kN; i++) {
        pk[i].resize(2000);
        pk[i].resize(build(pk[i].data(), i, i % 3 == 1, i % 4 == 2, i % 5 == 4 ? 1400 : 3 * i));
        pos = (pos + 15) / 16 * 16 + i % 16;
        offs[i] = pos, lens[i] = (uint32_t)pk[i].size();
        pos += pk[i].size();
    }
    Block<uint8_t> slab(pos);
    for (uint32_t i = 0; i < kN; i++) std::memcpy(slab.p + offs[i], pk[i].data(), pk[i].size());
    Block<uint8_t> nh(kN), ty(kRows * kN);
    Block<uint16_t> of(kRows * kN);
    for (uint32_t i = 0; i < kN; i++) {
        const bool v6 = i % 3 == 1, vlan = i % 4 == 2;
        uint32_t j = 0, o = 0;
        ty[j * kN + i] = PKT_HDR_ETHER, of[j++ * kN + i] = 0, o = 14;
        if (vlan) ty[j * kN + i] = PKT_HDR_VLAN, of[j++ * kN + i] = 14, o = 18;
        ty[j * kN + i] = v6 ? PKT_HDR_IPV6 : PKT_HDR_IPV4, of[j++ * kN + i] = (uint16_t)o, o += v6 ? 40 : 20;
        ty[j * kN + i] = PKT_HDR_UDP, of[j++ * kN + i] = (uint16_t)o;
        nh[i] = (uint8_t)j;
    }
    Block<uint32_t> tnl(kN), entropy(kN);
    Block<uint8_t> select(kN);
    for (uint32_t i = 0; i < kN; i++) tnl[i] = i % 6, entropy[i] = i * 2654435761u, select[i] = i % 11 != 7;
    tnl[5] = 12;  // NO_TUNNEL
    const pkt_batch_t b{slab.p, slab.n, offs.p, lens.p, 0, 0, kN};
    const pkt_chain_t ch{nh.p, ty.p, of.p};

    // ---- encap: the sizing pass, then exact capacities
    uint64_t tot = 0, cnt = 0;
    if (pkt_tunnel_encap_host(&b, &ch, 0, PKT_TUN_NO_WRITE, tun, tnl.p, 0, entropy.p, 9, select.p, nullptr, nullptr, nullptr, 0, 0,
                              nullptr, nullptr, nullptr, nullptr, nullptr, &tot, &cnt) != PKT_SUCCESS)
        die("encap sizing", 0);
    if (cnt == 0 || cnt >= kN) die("encap count", cnt);
    Outputs E(kN, cnt, PKT_TUNE_STATUS_COUNT);
    Aligned edst(tot);
    const pkt_chain_t eoc{E.oc_nh.p, E.oc_ty.p, E.oc_of.p};
    uint64_t tot2 = 0, cnt2 = 0;
    if (pkt_tunnel_encap_host(&b, &ch, 0, 0, tun, tnl.p, 0, entropy.p, 9, select.p, E.status.p, E.out_index.p, edst.p, tot, cnt,
                              E.out_off.p, E.out_len.p, E.src_index.p, &eoc, E.hits.p, &tot2, &cnt2) != PKT_SUCCESS)
        die("encap", 0);
    if (tot2 != tot || cnt2 != cnt) die("encap totals", 0);
    uint64_t sum = 0;
    for (uint32_t k = 0; k < PKT_TUNE_STATUS_COUNT; k++) sum += E.hits[k];
    if (sum != kN) die("encap hits", sum);
    for (uint64_t q = 0; q < cnt; q++) {
        const uint32_t i = E.src_index[q], t = tnl[i];
        const uint8_t* o = edst.p + E.out_off[q];
        if (E.status[i] != PKT_TUNE_OK || E.out_index[i] != q) die("encap status", i);
        const bool vx = kinds[t][0] == PKT_TUN_VXLAN, o4 = kinds[t][1] == 4;
        const uint32_t ipo = vx ? 14 : of[(nh[i] - 2) * kN + i], H = o4 ? 20 : 40;
        if (o4) {
            if (ones_sum(o + ipo, 20) != 0xFFFFu) die("outer IPv4 checksum", q);
            if (ipo + be16(o + ipo + 2) != E.out_len[q]) die("outer IPv4 length", q);
            if (be16(o + ipo + 4) != ((9 + q) & 0xFFFFu)) die("outer identification", q);
        } else if (ipo + 40 + be16(o + ipo + 4) != E.out_len[q]) {
            die("outer IPv6 length", q);
        }
        if (vx) {
            const uint8_t* u = o + 14 + H;
            const uint32_t ul = be16(u + 4);
            if (14 + H + ul != E.out_len[q] || be16(u + 2) != 4789) die("UDP header", q);
            if (be16(u) != 2000 + entropy[i] % 1000) die("UDP source port", q);
            uint32_t s = ones_sum(o + ipo + (o4 ? 12 : 8), o4 ? 8 : 32);
            s += 17 + ul;
            if (ones_sum(u, ul, s) != 0xFFFFu) die("UDP checksum", q);
            if (std::memcmp(u + 16, pk[i].data(), pk[i].size())) die("VXLAN inner bytes", q);
        }
        for (uint32_t k = E.out_len[q]; k < (E.out_len[q] + 15) / 16 * 16; k++)
            if (o[k]) die("zero fill", q);
    }

    // ---- decap of the outputs gives the packets back
    {
        Block<uint64_t> doffs(cnt);
        Block<uint32_t> dlens(cnt);
        for (uint64_t q = 0; q < cnt; q++) doffs[q] = E.out_off[q], dlens[q] = E.out_len[q];
        // an exact-size copy of the encap slab (its rounded tail is not the batch's)
        uint64_t dl = 0;
        for (uint64_t q = 0; q < cnt; q++) dl = doffs[q] + dlens[q];
        Block<uint8_t> dslab(dl);
        std::memcpy(dslab.p, edst.p, dl);
        const pkt_batch_t db{dslab.p, dl, doffs.p, dlens.p, 0, 0, cnt};
        uint64_t t3 = 0, c3 = 0;
        if (pkt_tunnel_decap_host(&db, &eoc, 0, PKT_TUN_NO_WRITE, tun, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr,
                                  nullptr, nullptr, nullptr, nullptr, &t3, &c3) != PKT_SUCCESS || c3 != cnt)
            die("decap sizing", c3);
        Outputs D(cnt, c3, PKT_TUND_STATUS_COUNT);
        Aligned ddst(t3);
        const pkt_chain_t doc{D.oc_nh.p, D.oc_ty.p, D.oc_of.p};
        if (pkt_tunnel_decap_host(&db, &eoc, 0, 0, tun, nullptr, D.status.p, D.out_index.p, D.tunnel_out.p, ddst.p, t3, c3,
                                  D.out_off.p, D.out_len.p, D.src_index.p, &doc, D.hits.p, &t3, &c3) != PKT_SUCCESS)
            die("decap", 0);
        if (D.hits[PKT_TUND_OK] != cnt) die("decap hits", D.hits[PKT_TUND_OK]);
        for (uint64_t q = 0; q < cnt; q++) {
            const uint32_t i = E.src_index[q];
            if (D.tunnel_out[q] != tnl[i] + 6) die("decap tunnel_out", q);
            if (D.out_len[q] != pk[i].size() || std::memcmp(ddst.p + D.out_off[q], pk[i].data(), pk[i].size())) die("decap bytes", q);
            if (D.oc_nh[q] != nh[i]) die("decap rows", q);
            for (uint32_t j = 0; j < nh[i]; j++)
                if (D.oc_ty[j * c3 + q] != ty[j * kN + i] || D.oc_of[j * c3 + q] != of[j * kN + i]) die("decap row", q);
        }
        // every NULL-output combination, with and without NO_WRITE
        for (uint32_t m = 0; m < 64; m++)
            for (uint32_t fl = 0; fl < 2; fl++) {
                const pkt_chain_t part{m & 8 ? D.oc_nh.p : nullptr, m & 16 ? D.oc_ty.p : nullptr, m & 32 ? D.oc_of.p : nullptr};
                const int rc = pkt_tunnel_decap_host(&db, &eoc, 0, fl, tun, nullptr, m & 1 ? D.status.p : nullptr,
                                                     m & 2 ? D.out_index.p : nullptr, m & 4 ? D.tunnel_out.p : nullptr, ddst.p, t3,
                                                     c3, D.out_off.p, D.out_len.p, m & 1 ? D.src_index.p : nullptr,
                                                     m & 56 ? &part : nullptr, m & 2 ? D.hits.p : nullptr, nullptr, nullptr);
                if (rc != PKT_SUCCESS) die("decap NULL outputs", m);
            }
    }
    for (uint32_t m = 0; m < 64; m++)
        for (uint32_t fl = 0; fl < 2; fl++) {
            const pkt_chain_t part{m & 8 ? E.oc_nh.p : nullptr, m & 16 ? E.oc_ty.p : nullptr, m & 32 ? E.oc_of.p : nullptr};
            const int rc = pkt_tunnel_encap_host(&b, &ch, 0, fl, tun, m & 4 ? tnl.p : nullptr, 1, m & 2 ? entropy.p : nullptr, 0,
                                                 m & 1 ? select.p : nullptr, m & 1 ? E.status.p : nullptr,
                                                 m & 2 ? E.out_index.p : nullptr, fl ? nullptr : edst.p, fl ? 0 : tot,
                                                 fl ? 0 : cnt, fl ? nullptr : E.out_off.p, fl ? nullptr : E.out_len.p,
                                                 m & 4 ? E.src_index.p : nullptr, m & 56 ? &part : nullptr,
                                                 m & 2 ? E.hits.p : nullptr, m & 1 ? &tot2 : nullptr, m & 4 ? &cnt2 : nullptr);
            // without select / with tunnel_all the outputs may outgrow the capacities: the refusal then
            if (rc != PKT_SUCCESS && !(rc == PKT_ERR_INVALID_ARG && !fl && (!(m & 1) || !(m & 4)))) die("encap NULL outputs", m);
        }

    // ---- forged chains: offsets past the packet, n_hdrs 255, for every tunnel kind and for decap
    {
        Block<uint8_t> fnh(kN), fty(kRows * kN);
        Block<uint16_t> fof(kRows * kN);
        for (uint32_t i = 0; i < kN; i++) {
            fnh[i] = i % 2 ? 255 : (uint8_t)(1 + i % 16);
            for (uint32_t j = 0; j < kRows; j++) {
                const uint32_t pick[6] = {PKT_HDR_ETHER, PKT_HDR_IPV4, PKT_HDR_IPV6, PKT_HDR_UDP, PKT_HDR_VXLAN, PKT_HDR_GRE};
                fty[j * kN + i] = (uint8_t)pick[(i + j * 5) % 6];
                fof[j * kN + i] = (uint16_t)((i * 977 + j * 7919) % 7 == 0 ? 65535 - j : (i * 31 + j * 14) % 1500);
            }
        }
        const pkt_chain_t fch{fnh.p, fty.p, fof.p};
        for (uint32_t t = 0; t < 6; t++)
            for (uint32_t which : {0u, 1u, (uint32_t)PKT_FLOW_LAST}) {
                uint64_t ft = 0, fc = 0;
                if (pkt_tunnel_encap_host(&b, &fch, which, PKT_TUN_NO_WRITE, tun, nullptr, t, nullptr, 0, nullptr, nullptr, nullptr,
                                          nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, &ft, &fc) != PKT_SUCCESS)
                    die("forged sizing", t);
                Outputs F(kN, fc ? fc : 1, PKT_TUNE_STATUS_COUNT);
                Aligned fdst(ft);
                const pkt_chain_t foc{F.oc_nh.p, F.oc_ty.p, F.oc_of.p};
                if (pkt_tunnel_encap_host(&b, &fch, which, 0, tun, nullptr, t, nullptr, 0, nullptr, F.status.p, F.out_index.p, fdst.p,
                                          ft, fc ? fc : 1, F.out_off.p, F.out_len.p, F.src_index.p, &foc, F.hits.p, nullptr,
                                          nullptr) != PKT_SUCCESS)
                    die("forged encap", t);
            }
        for (uint32_t which : {0u, 1u, 2u, (uint32_t)PKT_FLOW_LAST}) {
            uint64_t ft = 0, fc = 0;
            if (pkt_tunnel_decap_host(&b, &fch, which, PKT_TUN_NO_WRITE, tun, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0,
                                      nullptr, nullptr, nullptr, nullptr, nullptr, &ft, &fc) != PKT_SUCCESS)
                die("forged decap sizing", which);
            Outputs F(kN, fc ? fc : 1, PKT_TUND_STATUS_COUNT);
            Aligned fdst(ft);
            const pkt_chain_t foc{F.oc_nh.p, F.oc_ty.p, F.oc_of.p};
            if (pkt_tunnel_decap_host(&b, &fch, which, 0, tun, nullptr, F.status.p, F.out_index.p, F.tunnel_out.p, fdst.p, ft,
                                      fc ? fc : 1, F.out_off.p, F.out_len.p, F.src_index.p, &foc, F.hits.p, nullptr,
                                      nullptr) != PKT_SUCCESS)
                die("forged decap", which);
        }
    }

    // ---- call refusals: nothing is written
    {
        Outputs R(kN, cnt, PKT_TUNE_STATUS_COUNT);
        Aligned rdst(tot);
        const pkt_chain_t roc{R.oc_nh.p, R.oc_ty.p, R.oc_of.p};
        const auto enc = [&](const pkt_batch_t* bb, const pkt_chain_t* cc, uint32_t which, uint32_t fl, const pkt_tunnel_t* tt,
                             const uint32_t* tn, uint8_t* dst, uint64_t dl, uint64_t cap) {
            return pkt_tunnel_encap_host(bb, cc, which, fl, tt, tn, 0, entropy.p, 9, select.p, R.status.p, R.out_index.p, dst, dl, cap,
                                         R.out_off.p, R.out_len.p, R.src_index.p, &roc, R.hits.p, nullptr, nullptr);
        };
        expect_refusal(enc(nullptr, &ch, 0, 0, tun, tnl.p, rdst.p, tot, cnt), tun, "pkt_tunnel_encap_host: null argument", 20);
        expect_refusal(enc(&b, &ch, 0, 0, nullptr, tnl.p, rdst.p, tot, cnt), nullptr, "pkt_tunnel_encap_host: null tunnel table", 21);
        expect_refusal(enc(&b, &ch, 0, 4, tun, tnl.p, rdst.p, tot, cnt), tun, "pkt_tunnel_encap_host: unknown flag bits", 22);
        expect_refusal(enc(&b, &ch, 99, 0, tun, tnl.p, rdst.p, tot, cnt), tun,
                       "pkt_tunnel_encap_host: which_ip is neither below 16 nor PKT_FLOW_LAST", 23);
        expect_refusal(enc(&b, &ch, 0, 0, tun, reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(tnl.p) + 1), rdst.p,
                           tot, cnt),
                       tun, "pkt_tunnel_encap_host: a uint32_t array is not 4-byte aligned", 24);
        expect_refusal(enc(&b, &ch, 0, 0, tun, tnl.p, rdst.p + 4, tot, cnt), tun, "pkt_tunnel_encap_host: dst not 16-byte aligned", 25);
        expect_refusal(enc(&b, &ch, 0, 0, tun, tnl.p, nullptr, tot, cnt), tun,
                       "pkt_tunnel_encap_host: null dst, out_off or out_len without PKT_TUN_NO_WRITE", 26);
        expect_refusal(enc(&b, &ch, 0, 0, tun, tnl.p, rdst.p, tot, 0), tun, "pkt_tunnel_encap_host: out_cap is 0 or >= 2^32", 27);
        // one too small: the overflow refusal, the totals set, nothing written
        if (enc(&b, &ch, 0, 0, tun, tnl.p, rdst.p, tot - 1, cnt) != PKT_ERR_INVALID_ARG) die("dst one too small", 0);
        if (enc(&b, &ch, 0, 0, tun, tnl.p, rdst.p, tot, cnt - 1) != PKT_ERR_INVALID_ARG) die("out_cap one too small", 0);
        for (uint64_t k = 0; k < tot; k++)
            if (rdst.p[k] != 0x77) die("a refused call wrote dst", k);
        for (uint64_t k = 0; k < cnt; k++)
            if (R.out_len[k] != 0x77777777u) die("a refused call wrote out_len", k);
    }

    if (pkt_tunnel_destroy(tun) != PKT_SUCCESS) die("destroy", 0);
    std::printf("tunnel OK: %llu of %u packets encapsulated into %llu bytes and taken out again\n", (unsigned long long)cnt, kN,
                (unsigned long long)tot);
    return 0;
}
