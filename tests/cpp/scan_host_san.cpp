// scan_host_san.cpp — pkt_scan_create_host / pkt_scan_batch on host memory (packet-rs_amd/csrc/pktgpu_host.cpp with
// pktgpu_scan.hpp: the compiler, the walk, the region rule and the refusals the kernel shares) under AddressSanitizer
// + UndefinedBehaviorSanitizer: a stand-alone program, no GPU.  Every array (the pattern blob and table, the slab, the
// chain columns, select, every output, the counters) is a heap block of its exact size, so a read or write past one
// is a report.  The packets lie end to end at every source alignment, the last one ending on the slab's last byte
// with a pattern ending there; some chain columns are forged (n_hdrs of 255, an offset past the packet, a type
// outside 1..21); every NULL-output combination runs; the refusals leave what they must alone.  The outputs are
// checked against a naive search written here.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
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

uint8_t fold(uint8_t c) { return c >= 0x41 && c <= 0x5A ? c + 0x20 : c; }

struct Pat {
    std::string s;
    bool nocase;
    uint8_t group;
    uint32_t action;
};

constexpr uint32_t kHdrSize[22] = {0, 14, 4, 20, 40, 4, 20, 8, 28, 8, 14, 3, 5, 4, 4, 4, 4, 8, 12, 8, 35, 4};

void drive(uint32_t n, uint32_t region, bool with_select) {
    // ---- the patterns: a family, duplicates, both cases, a 64-byte one, bytes 0x00 and 0xFF
    std::vector<Pat> pats = {{"a", false, 0, 1},    {"ab", false, 1, 2},        {"abc", false, 2, 0},     {"abcd", false, 3, 4},
                             {"abc", false, 4, 5},  {"BCD", true, 5, 6},        {"dcb", true, 6, 7},      {std::string(64, 'd'), false, 7, 8},
                             {std::string("\0\xff", 2), false, 8, 9},           {"cdab", true, 63, 10},   {"tail!", false, 9, 11}};
    uint64_t nbytes = 0;
    for (auto& p : pats) nbytes += p.s.size();
    Block<uint8_t> blob(nbytes);
    Block<pkt_scan_pattern_t> tab(pats.size());
    uint64_t at = 0;
    for (size_t k = 0; k < pats.size(); k++) {
        std::memcpy(blob.p + at, pats[k].s.data(), pats[k].s.size());
        tab[k] = pkt_scan_pattern_t{(uint32_t)at, (uint16_t)pats[k].s.size(), (uint8_t)(pats[k].nocase ? PKT_SCAN_NOCASE : 0),
                                    pats[k].group, pats[k].action, 0};
        at += pats[k].s.size();
    }
    pkt_scan_t* sc = nullptr;
    if (pkt_scan_create_host(blob.p, nbytes, tab.p, (uint32_t)pats.size(), 77, &sc) != PKT_SUCCESS || !sc) die("create", 0);
    pkt_scan_info_t info;
    if (pkt_scan_info(sc, &info) != PKT_SUCCESS || info.npatterns != pats.size() || info.max_len != 64) die("info", 0);

    // ---- the packets, end to end (every alignment); the last ends at the slab's last byte with "tail!"
    std::vector<std::vector<uint8_t>> pk(n);
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t len = i % 11 == 0 ? 0 : 14 + rnd() % (i % 7 == 0 ? 300 : 40);
        pk[i].resize(len);
        for (auto& x : pk[i]) {
            const uint32_t r = rnd() % 16;
            x = r < 12 ? "abcd"[r & 3] : r < 14 ? "ABCD"[rnd() & 3] : r == 14 ? 0x00 : 0xFF;
        }
        if (i % 7 == 0 && len >= 200) std::memset(pk[i].data() + 100, 'd', 70);
        if (i == n - 1) {
            pk[i].resize(14 + 9);
            std::memcpy(pk[i].data() + 14, "abcdtail!", 9);
        }
        total += pk[i].size();
    }
    Block<uint8_t> slab(total);
    Block<uint64_t> offs(n);
    Block<uint32_t> lens(n);
    Block<uint8_t> nh(n), ty((uint64_t)PKT_MAX_HDRS * n), sel(n);
    Block<uint16_t> of((uint64_t)PKT_MAX_HDRS * n);
    std::memset(ty.p, 0, ty.n);
    std::memset(of.p, 0, of.n * 2);
    at = 0;
    for (uint32_t i = 0; i < n; i++) {
        offs[i] = at;
        lens[i] = (uint32_t)pk[i].size();
        if (!pk[i].empty()) std::memcpy(slab.p + at, pk[i].data(), pk[i].size());
        at += pk[i].size();
        nh[i] = 1;
        ty[i] = PKT_HDR_ETHER;
        sel[i] = i % 9 != 4;
        switch (i % 10) {  // forged chains
            case 2: nh[i] = 255; break;                                            // cut to 16 entries: type 0 follows
            case 3: of[i] = (uint16_t)(pk[i].size() + 5); break;                    // an offset past the packet
            case 5: ty[i] = 22; break;                                             // a type outside 1..21
            case 6: nh[i] = 0; break;
            case 7: nh[i] = 2; ty[n + i] = PKT_HDR_VLAN; of[n + i] = 2; break;      // the maximum, not the last
            default: break;
        }
    }
    lens[n - 1] = 0xFFFFFFFFu;  // clamped to the slab's end
    const pkt_batch_t b{slab.p, total, offs.p, lens.p, 0, 0, n};
    const pkt_chain_t ch{nh.p, ty.p, of.p};

    // ---- the answers, by a naive search
    std::vector<uint32_t> w_st(n), w_pat(n), w_off(n), w_act(n), w_cnt(n);
    std::vector<uint64_t> w_m(n), w_hits(pats.size() + 1, 0);
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t len = (uint32_t)pk[i].size();
        uint32_t st = PKT_SCAN_MISS, r0 = 0;
        if (with_select && !sel[i]) {
            st = PKT_SCAN_SKIPPED;
        } else if (region == PKT_SCAN_PAYLOAD) {
            if (nh[i] == 0) st = PKT_SCAN_NO_CHAIN;
            for (uint32_t j = 0; j < (nh[i] > 16u ? 16u : nh[i]) && st == PKT_SCAN_MISS; j++) {
                const uint32_t t = ty[(uint64_t)j * n + i];
                if (t < 1 || t > 21) st = PKT_SCAN_SPAN;
                else if (of[(uint64_t)j * n + i] + kHdrSize[t] > r0) r0 = of[(uint64_t)j * n + i] + kHdrSize[t];
            }
            if (st == PKT_SCAN_MISS && r0 > len) st = PKT_SCAN_SPAN;
        }
        w_st[i] = st;
        w_pat[i] = PKT_SCAN_NONE;
        w_act[i] = st == PKT_SCAN_SKIPPED ? 0 : 77;
        if (st != PKT_SCAN_MISS) continue;
        for (uint32_t p = 0; p < pats.size(); p++) {
            const std::string& s = pats[p].s;
            for (uint32_t q = r0; q + s.size() <= len; q++) {
                bool eq = true;
                for (size_t k = 0; k < s.size() && eq; k++)
                    eq = pats[p].nocase ? fold(pk[i][q + k]) == fold((uint8_t)s[k]) : pk[i][q + k] == (uint8_t)s[k];
                if (!eq) continue;
                if (w_pat[i] == PKT_SCAN_NONE) {
                    w_pat[i] = p;
                    w_off[i] = q;
                    w_act[i] = pats[p].action;
                }
                w_cnt[i]++;
                w_m[i] |= 1ull << pats[p].group;
                w_hits[p]++;
            }
        }
        if (w_cnt[i]) w_st[i] = PKT_SCAN_HIT;
        else w_hits[pats.size()]++;
    }
    if (region == PKT_SCAN_PACKET && w_st[n - 1] != PKT_SCAN_SKIPPED && (w_pat[n - 1] != 0 || !(w_m[n - 1] >> 9 & 1)))
        die("the last packet's patterns", n - 1);  // "tail!" ends on the slab's last byte

    // ---- every NULL-output combination
    for (uint32_t mask = 0; mask < 256; mask++) {
        Block<uint8_t> status(n), osel(n);
        Block<uint32_t> pat(n), action(n), count(n);
        Block<uint16_t> off(n);
        Block<uint64_t> matched(n), hits(pats.size() + 1);
        std::memset(static_cast<void*>(hits.p), 0, hits.n * 8);
        const int rc = pkt_scan_batch(sc, &b, region == PKT_SCAN_PAYLOAD ? &ch : nullptr, region, with_select ? sel.p : nullptr,
                                      mask & 1 ? status.p : nullptr, mask & 2 ? pat.p : nullptr, mask & 4 ? off.p : nullptr,
                                      mask & 8 ? action.p : nullptr, mask & 16 ? osel.p : nullptr, mask & 32 ? count.p : nullptr,
                                      mask & 64 ? matched.p : nullptr, mask & 128 ? hits.p : nullptr, nullptr);
        if (rc != PKT_SUCCESS) die("pkt_scan_batch", mask);
        for (uint32_t i = 0; i < n; i++) {
            if ((mask & 1) && status[i] != w_st[i]) die("status", i);
            if ((mask & 2) && pat[i] != w_pat[i]) die("pat", i);
            if ((mask & 4) && off[i] != w_off[i]) die("off", i);
            if ((mask & 8) && action[i] != w_act[i]) die("action", i);
            if ((mask & 16) && osel[i] != (w_act[i] != 0)) die("sel", i);
            if ((mask & 32) && count[i] != w_cnt[i]) die("count", i);
            if ((mask & 64) && matched[i] != w_m[i]) die("matched", i);
            if (!(mask & 1) && status[i] != 0x77) die("status written", i);
        }
        for (size_t p = 0; p <= pats.size(); p++)
            if (hits[p] != (mask & 128 ? w_hits[p] : 0)) die("hits", p);
    }

    // ---- refusals write nothing
    {
        Block<uint8_t> status(n);
        Block<uint64_t> odd(n + 1);
        pkt_batch_t bad = b;
        bad.lens = nullptr;
        if (pkt_scan_batch(sc, &bad, &ch, region, nullptr, status.p, 0, 0, 0, 0, 0, 0, 0, 0) != PKT_ERR_INVALID_ARG) die("offsets without lens", 0);
        if (pkt_scan_batch(sc, &b, nullptr, PKT_SCAN_PAYLOAD, nullptr, status.p, 0, 0, 0, 0, 0, 0, 0, 0) != PKT_ERR_INVALID_ARG) die("null chain", 0);
        if (pkt_scan_batch(sc, &b, &ch, 2, nullptr, status.p, 0, 0, 0, 0, 0, 0, 0, 0) != PKT_ERR_INVALID_ARG) die("region", 0);
        uint64_t* mis = reinterpret_cast<uint64_t*>(reinterpret_cast<uint8_t*>(odd.p) + 4);
        if (pkt_scan_batch(sc, &b, &ch, region, nullptr, status.p, 0, 0, 0, 0, 0, mis, 0, 0) != PKT_ERR_INVALID_ARG) die("matched alignment", 0);
        if (!std::strstr(pkt_scan_last_error(sc), "8-byte aligned")) die("text", 0);
        for (uint32_t i = 0; i < n; i++)
            if (status[i] != 0x77) die("a refusal wrote", i);
    }
    if (pkt_scan_destroy(sc) != PKT_SUCCESS) die("destroy", 0);
}

void limits() {
    // 2048 patterns of 64 bytes: PKT_SCAN_MAX_BYTES exactly; one more byte is refused
    Block<uint8_t> blob(PKT_SCAN_MAX_BYTES);
    for (uint64_t k = 0; k < blob.n; k++) blob[k] = (uint8_t)rnd();
    Block<pkt_scan_pattern_t> tab(2049);
    for (uint32_t k = 0; k < 2049; k++) tab[k] = pkt_scan_pattern_t{(k % 2048) * 64u, 64, (uint8_t)(k & 1), (uint8_t)(k % 64), k, 0};
    pkt_scan_t* sc = nullptr;
    if (pkt_scan_create_host(blob.p, blob.n, tab.p, 2049, 0, &sc) != PKT_ERR_INVALID_ARG || sc) die("max bytes", 0);
    if (!std::strstr(pkt_scan_last_error(nullptr), "PKT_SCAN_MAX_BYTES")) die("max bytes text", 0);
    if (pkt_scan_create_host(blob.p, blob.n, tab.p, 2048, 0, &sc) != PKT_SUCCESS) die("at the limit", 0);
    // a slab that is the blob itself: every pattern occurs at its own place
    const pkt_batch_t b{blob.p, blob.n, nullptr, nullptr, 4096, 0, 32};
    Block<uint32_t> count(32);
    Block<uint64_t> hits(2049);
    std::memset(static_cast<void*>(hits.p), 0, hits.n * 8);
    if (pkt_scan_batch(sc, &b, nullptr, PKT_SCAN_PACKET, nullptr, 0, 0, 0, 0, 0, count.p, 0, hits.p, nullptr) != PKT_SUCCESS) die("limits batch", 0);
    for (uint32_t i = 0; i < 32; i++)
        if (count[i] < 64) die("limits count", i);
    for (uint32_t k = 0; k < 2048; k++)
        if (hits[k] < 1) die("limits hits", k);
    pkt_scan_destroy(sc);
    tab[7].len = 65;
    if (pkt_scan_create_host(blob.p, blob.n, tab.p, 8, 0, &sc) != PKT_ERR_INVALID_ARG) die("len 65", 0);
    // npats == 0, n == 0
    if (pkt_scan_create_host(nullptr, 0, nullptr, 0, 3, &sc) != PKT_SUCCESS) die("empty set", 0);
    Block<uint32_t> act(32);
    if (pkt_scan_batch(sc, &b, nullptr, PKT_SCAN_PACKET, nullptr, 0, 0, 0, act.p, 0, 0, 0, 0, nullptr) != PKT_SUCCESS || act[31] != 3) die("empty set batch", 0);
    const pkt_batch_t none{};
    if (pkt_scan_batch(sc, &none, nullptr, PKT_SCAN_PAYLOAD, nullptr, 0, 0, 0, act.p, 0, 0, 0, 0, nullptr) != PKT_ERR_INVALID_ARG) die("n 0 null chain", 0);
    if (pkt_scan_batch(sc, &none, nullptr, PKT_SCAN_PACKET, nullptr, 0, 0, 0, act.p, 0, 0, 0, 0, nullptr) != PKT_SUCCESS) die("n 0", 0);
    pkt_scan_destroy(sc);
}

}  // namespace

int main() {
    for (uint32_t n : {1u, 64u, 131u})
        for (uint32_t region : {(uint32_t)PKT_SCAN_PACKET, (uint32_t)PKT_SCAN_PAYLOAD})
            for (bool with_select : {false, true}) drive(n, region, with_select);
    limits();
    std::printf("scan OK\n");
    return 0;
}
