// meter_host_san.cpp — the host handle of pkt_meter_* (packet-rs_amd/csrc/pktgpu_host.cpp with pktgpu_meter.hpp: the
// refill, the decision, the DSCP stores and the refusals the kernels share) under AddressSanitizer +
// UndefinedBehaviorSanitizer: a stand-alone program, no GPU.  Every array (cfg, slab, chain columns, meter, time,
// in_color, select, outputs, counters, exported state) is a heap block of its exact size, so a read or write past one
// is a report.  Packets lie at every alignment 0..15, the last one ending on the slab's last byte; some chain columns
// are forged (an IP offset past the packet, n_hdrs of 255); every NULL-output combination runs with and without
// PKT_METER_MARK; the refusals leave everything alone.  Colours, pass, marked, counters, the state and the IPv4
// checksums (summed again here by RFC 1071) are checked against a walk in 128-bit integers worked out here.
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

typedef unsigned __int128 u128;
constexpr uint64_t kUnit = 1000000000ull;
constexpr uint32_t kMeters = 7;

uint32_t ones_sum(const uint8_t* p, uint32_t n) {
    uint32_t s = 0;
    for (uint32_t k = 0; k < n; k += 2) s += (uint32_t)p[k] << 8 | p[k + 1];
    while (s >> 16) s = (s & 0xFFFFu) + (s >> 16);
    return s;
}

// Ether / IPv4 or IPv6 / 8 bytes and `tail` more; returns the length
uint32_t build(uint8_t* p, bool v4, uint32_t tos, uint32_t tail) {
    const uint32_t len = 14 + (v4 ? 20 : 40) + 8 + tail;
    for (uint32_t k = 0; k < len; k++) p[k] = (uint8_t)(k * 11 + tail);
    uint8_t* ip = p + 14;
    if (v4) {
        ip[0] = 0x45, ip[1] = (uint8_t)tos, ip[10] = ip[11] = 0;
        const uint32_t c = 0xFFFFu - ones_sum(ip, 20);
        ip[10] = (uint8_t)(c >> 8), ip[11] = (uint8_t)c;
    } else {
        ip[0] = (uint8_t)(0x60 | tos >> 4), ip[1] = (uint8_t)((tos & 15u) << 4 | 0x0A);
    }
    return len;
}

struct Ref {  // the model, in integers that cannot overflow
    u128 c[kMeters], x[kMeters];
    uint64_t last[kMeters], pk[kMeters][3], by[kMeters][3];
};

pkt_meter_cfg_t cfg_of(uint32_t k) {
    pkt_meter_cfg_t g;
    std::memset(&g, 0, sizeof g);
    g.cir = k == 5 ? PKT_METER_MAX_RATE : k * 3000000ull;
    g.pir = k == 5 ? PKT_METER_MAX_RATE : k * 5000000ull;
    g.cbs = k == 5 ? PKT_METER_MAX_BURST : 100u * k;
    g.xbs = k == 5 ? PKT_METER_MAX_BURST : 90u * (kMeters - k);
    g.mode = (uint8_t)(k & 1u);
    g.flags = (uint8_t)(k & 2u ? PKT_METER_F_COLOR_AWARE : 0);
    for (uint32_t c = 0; c < 3; c++) {
        g.action[c] = (uint8_t)((k + c) % 3);
        g.dscp[c] = (uint8_t)((k * 9 + c * 21 + 1) % 64);
    }
    return g;
}

void expect_refusal(int rc, const pkt_meter_t* t, const char* text, uint64_t where) {
    if (rc != PKT_ERR_INVALID_ARG) die("refusal code", where);
    if (std::strcmp(pkt_meter_last_error(t), text) != 0) {
        std::printf("got '%s'\n", pkt_meter_last_error(t));
        die("refusal text", where);
    }
}

void drive(uint64_t n, int32_t adjust) {
    Block<pkt_meter_cfg_t> cfg(kMeters);
    for (uint32_t k = 0; k < kMeters; k++) cfg[k] = cfg_of(k);
    pkt_meter_t* t = nullptr;
    if (pkt_meter_create_host(cfg.p, kMeters, adjust, &t) != PKT_SUCCESS) die("create", n);
    Ref R;
    std::memset(&R, 0, sizeof R);
    for (uint32_t k = 0; k < kMeters; k++) R.c[k] = (u128)cfg[k].cbs * kUnit, R.x[k] = (u128)cfg[k].xbs * kUnit;
    // ---- packets: kinds 0 IPv4, 1 IPv6, 2 cut inside the IP header, 3 IP offset forged, 4 n_hdrs 255, 5 no IP entry
    Block<uint64_t> offs(n), time(n);
    Block<uint32_t> lens(n), meter(n);
    Block<uint8_t> nh(n), ty(PKT_MAX_HDRS * n), sel(n), ic(n);
    Block<uint16_t> of(PKT_MAX_HDRS * n);
    std::memset(ty.p, 0, ty.n);
    std::memset(static_cast<void*>(of.p), 0, of.n * 2);
    std::vector<uint8_t> kind(n), scratch(256);
    std::vector<uint32_t> plen(n);
    uint64_t pos = 0;
    for (uint64_t i = 0; i < n; i++) {
        kind[i] = (uint8_t)(i % 11 == 4 ? 2 : i % 13 == 6 ? 3 : i % 17 == 7 ? 4 : i % 19 == 9 ? 5 : i & 1);
        const bool v4 = kind[i] != 1;
        plen[i] = build(scratch.data(), v4, (uint32_t)(i * 37 % 256), (uint32_t)(i % 9));
        if (kind[i] == 2) plen[i] = 14 + (v4 ? 19 : 39);
        pos = (pos + 15) / 16 * 16 + i % 16;
        offs[i] = pos;
        pos += plen[i];
    }
    Block<uint8_t> slab(pos);  // the last packet ends on the last byte
    for (uint64_t i = 0; i < n; i++) {
        const bool v4 = kind[i] != 1;
        build(scratch.data(), v4, (uint32_t)(i * 37 % 256), (uint32_t)(i % 9));
        std::memcpy(slab.p + offs[i], scratch.data(), plen[i]);
        lens[i] = plen[i];
        nh[i] = kind[i] == 4 ? 255 : 2;
        ty[0 * n + i] = PKT_HDR_ETHER;
        ty[1 * n + i] = kind[i] == 5 ? (uint8_t)PKT_HDR_ARP : v4 ? (uint8_t)PKT_HDR_IPV4 : (uint8_t)PKT_HDR_IPV6;
        of[1 * n + i] = kind[i] == 3 ? (uint16_t)(plen[i] - 19) : 14;
        meter[i] = i % 23 == 0 ? kMeters : i % 29 == 0 ? 0xFFFFFFFFu : (uint32_t)(i * 5 % kMeters);
        sel[i] = i % 31 != 3;
        ic[i] = (uint8_t)(i * 3 % 5);
        time[i] = i % 7 == 6 ? 10 : 1000 + i * 40 + (i % 37 == 0 ? ~0ull >> 1 : 0);
    }
    Block<uint8_t> before(pos);
    std::memcpy(before.p, slab.p, pos);
    pkt_batch_t b;
    std::memset(&b, 0, sizeof b);
    b.slab = slab.p, b.slab_len = pos, b.offsets = offs.p, b.lens = lens.p, b.n = n;
    const pkt_chain_t chain = {nh.p, ty.p, of.p};
    // ---- refusals: nothing is read or written
    uint64_t words[2];
    expect_refusal(pkt_meter_batch(t, nullptr, nullptr, 0, 0, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), t,
                   "pkt_meter_batch: null argument", 0);
    expect_refusal(pkt_meter_batch(t, &b, &chain, 0, 2, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), t,
                   "pkt_meter_batch: unknown flag bits", 1);
    expect_refusal(pkt_meter_batch(t, &b, nullptr, 0, PKT_METER_MARK, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr),
                   t, "pkt_meter_batch: PKT_METER_MARK with a null chain", 2);
    expect_refusal(pkt_meter_batch(t, &b, &chain, 16, PKT_METER_MARK, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr),
                   t, "pkt_meter_batch: which_ip is neither below 16 nor PKT_FLOW_LAST", 3);
    expect_refusal(pkt_meter_batch(t, &b, &chain, 0, 0, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                   reinterpret_cast<uint64_t*>(reinterpret_cast<uint8_t*>(words) + 4), nullptr, nullptr),
                   t, "pkt_meter_batch: hits / bytes / time_ns not 8-byte aligned", 4);
    expect_refusal(pkt_meter_batch(t, &b, &chain, 0, 0, 0, nullptr, 0, reinterpret_cast<uint64_t*>(reinterpret_cast<uint8_t*>(words) + 1), nullptr, nullptr,
                                   nullptr, nullptr, nullptr, nullptr, nullptr, nullptr),
                   t, "pkt_meter_batch: hits / bytes / time_ns not 8-byte aligned", 5);
    if (n) {
        pkt_batch_t bad = b;
        bad.lens = nullptr;
        expect_refusal(pkt_meter_batch(t, &bad, &chain, 0, 0, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), t,
                       "pkt_meter_batch: offsets without lens", 6);
        bad = b;
        bad.n = 1ull << 32;
        expect_refusal(pkt_meter_batch(t, &bad, &chain, 0, 0, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), t,
                       "pkt_meter_batch: n >= 2^32", 7);
        const pkt_chain_t holed = {nh.p, nullptr, of.p};
        expect_refusal(pkt_meter_batch(t, &b, &holed, 0, PKT_METER_MARK, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr),
                       t, "pkt_meter_batch: null chain column", 8);
    }
    if (std::memcmp(before.p, slab.p, pos) != 0) die("a refusal wrote", n);
    // ---- the call, with every NULL-output combination; the state of the first is checked, the rest reset first
    for (uint32_t mask = 0; mask < 64; mask++) {
        const bool mark = mask & 32u;
        if (mask) {
            if (pkt_meter_reset(t, nullptr) != PKT_SUCCESS) die("reset", mask);
            std::memcpy(slab.p, before.p, pos);
            std::memset(&R, 0, sizeof R);
            for (uint32_t k = 0; k < kMeters; k++) R.c[k] = (u128)cfg[k].cbs * kUnit, R.x[k] = (u128)cfg[k].xbs * kUnit;
        }
        Block<uint8_t> color(n), pass(n), marked(n);
        Block<uint64_t> hits(PKT_METER_COLORS), bytes(PKT_METER_COLORS);
        for (uint32_t q = 0; q < PKT_METER_COLORS; q++) hits[q] = 100 + q, bytes[q] = 1000 + q;
        const int rc = pkt_meter_batch(t, &b, mark ? &chain : nullptr, 0, mark ? PKT_METER_MARK : 0, 3, mask & 1u ? nullptr : meter.p, 500,
                                       mask & 2u ? nullptr : time.p, ic.p, sel.p, mask & 1u ? color.p : nullptr,
                                       mask & 2u ? pass.p : nullptr, mask & 4u ? marked.p : nullptr, mask & 8u ? hits.p : nullptr,
                                       mask & 16u ? bytes.p : nullptr, nullptr);
        if (rc != PKT_SUCCESS) die("batch", mask);
        uint64_t eh[PKT_METER_COLORS] = {100, 101, 102, 103}, eb[PKT_METER_COLORS] = {1000, 1001, 1002, 1003};
        for (uint64_t i = 0; i < n; i++) {
            const uint32_t k = mask & 1u ? 3u : meter[i];
            uint32_t col = PKT_METER_UNMETERED, act = PKT_METER_PASS;
            if (sel[i] && k < kMeters) {
                const pkt_meter_cfg_t& g = cfg[k];
                const uint64_t tm = mask & 2u ? 500 : time[i];
                const int64_t cost = (int64_t)plen[i] + adjust;
                const u128 B = cost < 0 ? 0 : (u128)cost * kUnit, cap = (u128)g.cbs * kUnit, xcap = (u128)g.xbs * kUnit;
                if (tm > R.last[k]) {
                    const u128 dt = tm - R.last[k];
                    R.last[k] = tm;
                    if (g.mode) {
                        R.c[k] = R.c[k] + g.cir * dt < cap ? R.c[k] + g.cir * dt : cap;
                        R.x[k] = R.x[k] + g.pir * dt < xcap ? R.x[k] + g.pir * dt : xcap;
                    } else {
                        const u128 a = g.cir * dt, c2 = R.c[k] + a < cap ? R.c[k] + a : cap, sp = R.c[k] + a - c2;
                        R.x[k] = R.x[k] + sp < xcap ? R.x[k] + sp : xcap;
                        R.c[k] = c2;
                    }
                }
                uint32_t c0 = g.flags & PKT_METER_F_COLOR_AWARE ? ic[i] : 0;
                c0 = c0 > 2 ? 2 : c0;
                if (g.mode) {
                    if (c0 == 2 || R.x[k] < B) col = 2;
                    else if (c0 == 1 || R.c[k] < B) col = 1, R.x[k] -= B;
                    else col = 0, R.c[k] -= B, R.x[k] -= B;
                } else {
                    if (c0 == 0 && R.c[k] >= B) col = 0, R.c[k] -= B;
                    else if (c0 <= 1 && R.x[k] >= B) col = 1, R.x[k] -= B;
                    else col = 2;
                }
                act = g.action[col];
                R.pk[k][col]++, R.by[k][col] += plen[i];
            }
            eh[col]++, eb[col] += plen[i];
            const uint32_t hdr = kind[i] == 1 ? 40 : 20, ipo = kind[i] == 3 ? plen[i] - 19 : 14;
            const bool wr = mark && act == PKT_METER_REMARK && kind[i] != 5 && ipo + hdr <= plen[i];
            if ((mask & 1u) && color[i] != col) die("color", i);
            if ((mask & 2u) && pass[i] != (act != PKT_METER_DROP)) die("pass", i);
            if ((mask & 4u) && marked[i] != wr) die("marked", i);
            const uint8_t* p = before.p + offs[i];
            const uint8_t* q = slab.p + offs[i];
            if (!wr) {
                if (std::memcmp(p, q, plen[i]) != 0) die("an unmarked packet changed", i);
                continue;
            }
            const uint32_t d = cfg[k].dscp[col];
            for (uint32_t j = 0; j < plen[i]; j++) {
                const bool may = kind[i] == 1 ? j == 14 || j == 15 : j == 15 || j == 24 || j == 25;
                if (!may && p[j] != q[j]) die("a byte outside the DSCP and the checksum changed", i);
            }
            if (kind[i] == 1) {
                const uint32_t tc = (q[14] & 15u) << 4 | q[15] >> 4, tc0 = (p[14] & 15u) << 4 | p[15] >> 4;
                if (tc >> 2 != d || (tc & 3u) != (tc0 & 3u) || (q[14] & 0xF0) != (p[14] & 0xF0) || (q[15] & 15) != (p[15] & 15)) die("v6 dscp", i);
            } else {
                if (q[15] >> 2 != (int)d || (q[15] & 3) != (p[15] & 3)) die("v4 dscp", i);
                if (ones_sum(q + 14, 20) != 0xFFFFu) die("v4 checksum", i);
            }
        }
        for (uint32_t q = 0; q < PKT_METER_COLORS; q++) {
            if (hits[q] != (mask & 8u ? eh[q] : 100 + q)) die("hits", q);
            if (bytes[q] != (mask & 16u ? eb[q] : 1000 + q)) die("bytes", q);
        }
        Block<pkt_meter_state_t> st(kMeters);
        if (pkt_meter_export(t, 0, kMeters, st.p) != PKT_SUCCESS) die("export", mask);
        for (uint32_t k = 0; k < kMeters; k++) {
            if (st[k].c != (uint64_t)R.c[k] || st[k].x != (uint64_t)R.x[k] || st[k].last != R.last[k]) die("state", k);
            for (uint32_t q = 0; q < 3; q++)
                if (st[k].packets[q] != R.pk[k][q] || st[k].bytes[q] != R.by[k][q]) die("counters", k);
        }
        Block<pkt_meter_state_t> one(1);
        if (pkt_meter_export(t, kMeters - 1, 1, one.p) != PKT_SUCCESS || one[0].c != st[kMeters - 1].c) die("export one", mask);
    }
    expect_refusal(pkt_meter_export(t, 1, kMeters, nullptr), t, "pkt_meter_export: first + count above nmeters", 9);
    if (pkt_meter_destroy(t) != PKT_SUCCESS) die("destroy", n);
}

void create_refusals() {
    Block<pkt_meter_cfg_t> cfg(2);
    pkt_meter_t* t = nullptr;
    for (uint32_t bad = 0; bad < 9; bad++) {
        cfg[0] = cfg_of(5), cfg[1] = cfg_of(5);
        pkt_meter_cfg_t& g = cfg[1];
        uint32_t nm = 2;
        switch (bad) {
            case 0: g.cir = PKT_METER_MAX_RATE + 1; break;
            case 1: g.pir = PKT_METER_MAX_RATE + 1; break;
            case 2: g.cbs = PKT_METER_MAX_BURST + 1; break;
            case 3: g.xbs = PKT_METER_MAX_BURST + 1; break;
            case 4: g.mode = 2; break;
            case 5: g.flags = 4; break;
            case 6: g.action[2] = 3; break;
            case 7: g.dscp[0] = 64; break;
            default: nm = 0; break;
        }
        if (pkt_meter_create_host(cfg.p, nm, 0, &t) != PKT_ERR_INVALID_ARG || t) die("create refusal", bad);
        if (std::strncmp(pkt_meter_last_error(nullptr), "pkt_meter_create_host: ", 23) != 0) die("create refusal text", bad);
    }
    if (pkt_meter_create_host(nullptr, 2, 0, &t) != PKT_ERR_INVALID_ARG) die("null cfg", 0);
    if (pkt_meter_create_host(cfg.p, PKT_METER_MAX_METERS + 1, 0, &t) != PKT_ERR_INVALID_ARG) die("too many", 0);
    if (pkt_meter_create_host(cfg.p, 2, 0, nullptr) != PKT_ERR_INVALID_ARG) die("null out", 0);
    if (pkt_sizeof_meter_cfg() != 32 || pkt_sizeof_meter_state() != 72) die("sizes", 0);
}

}  // namespace

int main() {
    create_refusals();
    const uint64_t ns[] = {0, 1, 17, 64, 333};
    const int32_t adj[] = {0, 20, -14, INT32_MAX, INT32_MIN};
    for (int k = 0; k < 5; k++) drive(ns[k], adj[k]);
    std::printf("meter OK\n");
    return 0;
}
