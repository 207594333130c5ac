// flow_host_san.cpp — pkt_flow_key_host and the host flow table (packet-rs_amd/csrc/pktgpu_host.cpp) under
// AddressSanitizer + UndefinedBehaviorSanitizer: a stand-alone program, no GPU.  Every slab is a heap block of
// exactly slab_len bytes, so a read past a packet's end (an IP header or ports taken on the chain's word) is a
// report.  It drives Ether / IPv4 | IPv6 / TCP | UDP | ICMP packets at every alignment with the last packet
// ending on the slab's last byte, the SPAN edges by lens and by the slab end (header short by one byte, whole,
// ports cut after 3 bytes, whole), the 65535 clamp, chains that point past the packet, every NULL-output
// combination, and a 64-slot table filled to the last slot and past it, exported with cap 0, cap < count and
// whole; keys, hash and counters are checked against values worked out here.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
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
    std::printf("FAIL %s at packet %llu\n", what, (unsigned long long)i);
    std::exit(1);
}

uint64_t mix(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ z >> 27) * 0x94D049BB133111EBull;
    return z ^ z >> 31;
}

struct Pkt {
    std::vector<uint8_t> bytes;
    bool v6;
    uint8_t l4t;
};

Pkt make(bool v6, uint8_t l4t, uint32_t pay) {
    Pkt p;
    const uint32_t iph = v6 ? 40 : 20, hs = l4t == PKT_HDR_TCP ? 20 : l4t == PKT_HDR_UDP ? 8 : 4;
    p.bytes.resize(14 + iph + hs + pay);
    for (auto& x : p.bytes) x = (uint8_t)rnd();
    p.v6 = v6, p.l4t = l4t;
    if (!v6) p.bytes[14 + 6] = 0x40, p.bytes[14 + 7] = 0;
    return p;
}

struct Batch {
    std::vector<Pkt> pk;
    uint8_t* slab = nullptr;  // exactly slab_len bytes
    uint64_t slab_len = 0;
    std::vector<uint64_t> offs;
    std::vector<uint32_t> lens;
    std::vector<uint8_t> nh, ty;
    std::vector<uint16_t> of;
    pkt_batch_t b{};
    pkt_chain_t ch{};
    ~Batch() { std::free(slab); }
};

// the packets back to back at the given alignments, the slab ending with the last packet's last byte
void lay(Batch& B, const std::vector<uint32_t>& align) {
    const uint64_t n = B.pk.size();
    uint64_t pos = 0;
    for (uint64_t i = 0; i < n; i++) {
        pos = (pos + 15) / 16 * 16 + align[i % align.size()];
        B.offs.push_back(pos);
        B.lens.push_back((uint32_t)B.pk[i].bytes.size());
        pos += B.pk[i].bytes.size();
    }
    B.slab_len = pos;
    B.slab = static_cast<uint8_t*>(std::malloc(pos ? pos : 1));
    std::memset(B.slab, 0xA5, pos);
    B.nh.assign(n, 3);
    B.ty.assign(PKT_MAX_HDRS * n, 0);
    B.of.assign(PKT_MAX_HDRS * n, 0);
    for (uint64_t i = 0; i < n; i++) {
        std::memcpy(B.slab + B.offs[i], B.pk[i].bytes.data(), B.pk[i].bytes.size());
        B.ty[0 * n + i] = PKT_HDR_ETHER;
        B.ty[1 * n + i] = B.pk[i].v6 ? PKT_HDR_IPV6 : PKT_HDR_IPV4;
        B.of[1 * n + i] = 14;
        B.ty[2 * n + i] = B.pk[i].l4t;
        B.of[2 * n + i] = B.pk[i].v6 ? 54 : 34;
    }
    B.b.slab = B.slab;
    B.b.slab_len = B.slab_len;
    B.b.offsets = B.offs.data();
    B.b.lens = B.lens.data();
    B.b.n = n;
    B.ch.n_hdrs = B.nh.data();
    B.ch.hdr_type = B.ty.data();
    B.ch.hdr_off = B.of.data();
}

struct Out {
    std::vector<pkt_flow_key_t> keys;
    std::vector<uint64_t> hash;
    std::vector<uint32_t> rss, plen;
    std::vector<uint8_t> dir, status;
    explicit Out(uint64_t n) : keys(n), hash(n), rss(n), plen(n), dir(n), status(n) {}
};

const uint8_t kRssKey[40] = {0x6d, 0x5a, 0x56, 0xda, 0x25, 0x5b, 0x0e, 0xc2, 0x41, 0x67, 0x25, 0x3d, 0x43, 0xa3,
                             0x8f, 0xb0, 0xd0, 0xca, 0x2b, 0xcb, 0xae, 0x7b, 0x30, 0xb4, 0x77, 0xcb, 0x2d, 0xa3,
                             0x80, 0x30, 0xf2, 0x0c, 0x6a, 0x42, 0xb7, 0x3b, 0xbe, 0xac, 0x01, 0xfa};

int run(const Batch& B, uint32_t which, uint32_t flags, Out& o, unsigned null_mask = 0) {
    return pkt_flow_key_host(&B.b, &B.ch, which, flags, 7, null_mask & 4 ? nullptr : kRssKey, null_mask & 1 ? nullptr : o.keys.data(),
                             null_mask & 2 ? nullptr : o.hash.data(), null_mask & 4 ? nullptr : o.rss.data(),
                             null_mask & 8 ? nullptr : o.dir.data(), null_mask & 16 ? nullptr : o.plen.data(),
                             null_mask & 32 ? nullptr : o.status.data());
}

// the expected status, key and hash of packet i with `len` of its bytes
void expect(const Batch& B, uint64_t i, uint32_t len, const Out& o) {
    const Pkt& p = B.pk[i];
    const uint32_t ipe = p.v6 ? 54 : 34;
    const bool l4 = p.l4t == PKT_HDR_TCP || p.l4t == PKT_HDR_UDP;
    const uint32_t st = len < ipe || (l4 && len < ipe + 4) ? PKT_FLOW_SPAN : PKT_FLOW_OK;
    if (o.status[i] != st) die("status", i);
    if (o.plen[i] != len) die("plen", i);
    uint8_t k[40] = {};
    uint64_t h = 0;
    if (st == PKT_FLOW_OK) {
        const uint32_t a = p.v6 ? 16 : 4;
        const uint8_t* q = p.bytes.data();
        std::memcpy(k, q + 14 + (p.v6 ? 8 : 12), a);
        std::memcpy(k + 16, q + 14 + (p.v6 ? 8 : 12) + a, a);
        if (l4) {
            k[32] = q[ipe + 1], k[33] = q[ipe];
            k[34] = q[ipe + 3], k[35] = q[ipe + 2];
        }
        k[36] = q[14 + (p.v6 ? 6 : 9)];
        k[37] = p.v6 ? 6 : 4;
        h = 7;
        for (int w = 0; w < 5; w++) {
            uint64_t x;
            std::memcpy(&x, k + 8 * w, 8);
            h = mix(h ^ x);
        }
    }
    if (std::memcmp(&o.keys[i], k, 40) != 0) die("key", i);
    if (o.hash[i] != h) die("hash", i);
    if (st != PKT_FLOW_OK && (o.rss[i] || o.dir[i])) die("non-OK outputs", i);
}

void keys_every_alignment() {
    Batch B;
    const uint8_t l4s[3] = {PKT_HDR_TCP, PKT_HDR_UDP, PKT_HDR_ICMP};
    for (uint32_t k = 0; k < 97; k++)  // the last one TCP over IPv4
        B.pk.push_back(make(k & 1, l4s[k % 3], k % 3 == 2 ? 0 : rnd() % 3));
    std::vector<uint32_t> al;
    for (uint32_t a = 0; a < 16; a++) al.push_back(a), al.push_back(a), al.push_back(a);
    lay(B, al);
    const uint64_t n = B.b.n;
    Out o(n);
    if (run(B, PKT_FLOW_LAST, 0, o) != PKT_SUCCESS) die("call", 0);
    for (uint64_t i = 0; i < n; i++) expect(B, i, B.lens[i], o);
    // every NULL-output combination
    for (unsigned m = 0; m < 64; m++) {
        Out q(n);
        if (run(B, 0, PKT_FLOW_SYMMETRIC, q, m) != PKT_SUCCESS) die("null outputs", m);
    }
    // the SPAN edges by lens: the header short by one byte, whole, ports cut after 3 bytes, whole
    for (uint32_t cut = 0; cut < 4; cut++) {
        for (uint64_t i = 0; i < n; i++) B.lens[i] = (B.pk[i].v6 ? 54 : 34) + (cut == 0 ? -1 : cut == 1 ? 0 : cut == 2 ? 3 : 4);
        for (uint64_t i = 0; i < n; i++) B.lens[i] = B.lens[i] > B.pk[i].bytes.size() ? (uint32_t)B.pk[i].bytes.size() : B.lens[i];
        if (run(B, PKT_FLOW_LAST, 0, o) != PKT_SUCCESS) die("call", cut);
        for (uint64_t i = 0; i < n; i++) expect(B, i, B.lens[i], o);
    }
    // ... and by the slab end: lens say 2000, the slab ends inside the last packet
    for (uint32_t keep = 0; keep < 60; keep += 1) {
        for (uint64_t i = 0; i < n; i++) B.lens[i] = 2000;
        const uint64_t end = B.offs[n - 1] + (keep < B.pk[n - 1].bytes.size() ? keep : B.pk[n - 1].bytes.size());
        uint8_t* exact = static_cast<uint8_t*>(std::malloc(end));
        std::memcpy(exact, B.slab, end);
        pkt_batch_t b = B.b;
        b.slab = exact;
        b.slab_len = end;
        Out q(n);
        if (pkt_flow_key_host(&b, &B.ch, 0, 0, 7, kRssKey, q.keys.data(), q.hash.data(), q.rss.data(), q.dir.data(),
                              q.plen.data(), q.status.data()) != PKT_SUCCESS)
            die("call", keep);
        expect(B, n - 1, (uint32_t)(end - B.offs[n - 1]), q);
        std::free(exact);
    }
    // chains that point past the packet, and more headers than rows
    for (uint64_t i = 0; i < n; i++) {
        B.lens[i] = (uint32_t)B.pk[i].bytes.size();
        B.nh[i] = 255;
        B.of[1 * n + i] = (uint16_t)(i % 2 ? 65535 : B.lens[i] - 19);
        B.of[2 * n + i] = 65535;
    }
    if (run(B, PKT_FLOW_LAST, PKT_FLOW_SYMMETRIC | PKT_FLOW_NO_PORTS, o) != PKT_SUCCESS) die("call", 1);
    for (uint64_t i = 0; i < n; i++)
        if (o.status[i] != PKT_FLOW_SPAN) die("chain past the packet", i);
}

void clamp_65535() {
    Batch B;
    B.pk.push_back(make(false, PKT_HDR_TCP, 0));
    lay(B, {0});
    std::free(B.slab);
    B.slab_len = 65535;  // exactly the clamp: lens say more
    B.slab = static_cast<uint8_t*>(std::malloc(B.slab_len));
    std::memset(B.slab, 0x5A, B.slab_len);
    B.b.slab = B.slab;
    B.b.slab_len = B.slab_len;
    B.lens[0] = 70000;
    Out o(1);
    for (uint32_t at : {65515u, 65516u, 65535u}) {
        B.of[1] = (uint16_t)at;
        B.of[2] = (uint16_t)(at + 20 > 65535 ? 65535 : at + 20);
        if (at + 8 <= B.slab_len) B.slab[at + 6] = 0x40, B.slab[at + 7] = 0;  // not a fragment: ports are taken
        if (run(B, 0, PKT_FLOW_NO_PORTS, o) != PKT_SUCCESS) die("call", at);
        if (o.plen[0] != 65535 || o.status[0] != (at == 65515 ? PKT_FLOW_OK : PKT_FLOW_SPAN)) die("clamp", at);
        if (run(B, 0, 0, o) != PKT_SUCCESS || o.status[0] != PKT_FLOW_SPAN) die("clamp ports", at);
    }
}

void table() {
    pkt_flow_table_t *t = nullptr, *none = nullptr;
    if (pkt_flow_table_create_host(48, &none) == PKT_SUCCESS || none) die("create 48", 0);
    if (pkt_flow_table_create_host(64, &t) != PKT_SUCCESS) die("create", 1);
    const uint64_t n = 65 * 9;
    std::vector<pkt_flow_key_t> keys(n);
    std::vector<uint64_t> hash(n);
    std::vector<uint8_t> dir(n), status(n, 0), upd(n);
    std::vector<uint32_t> w(n), id(n);
    std::memset(keys.data(), 0, n * sizeof(pkt_flow_key_t));
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t f = (uint32_t)(i % 65);  // flow 64 arrives last: the one that finds the table full
        keys[i].src[0] = (uint8_t)f;
        keys[i].ipver = 4;
        hash[i] = mix(f);
        dir[i] = (uint8_t)(rnd() & 1);
        w[i] = 60 + rnd() % 1400;
    }
    status[70] = 1;  // a packet of a flow the table already holds
    if (pkt_flow_table_update(t, keys.data(), hash.data(), dir.data(), w.data(), status.data(), n, 10, id.data(), upd.data(), nullptr))
        die("update", 0);
    std::map<uint32_t, std::vector<uint64_t>> want;  // flow -> pkts[2], bytes[2], first
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t f = (uint32_t)(i % 65);
        const uint8_t st = i == 70 ? PKT_FLOW_UPD_SKIPPED : f == 64 ? PKT_FLOW_UPD_FULL : PKT_FLOW_UPD_OK;
        if (upd[i] != st || (st != PKT_FLOW_UPD_OK) != (id[i] == 0xFFFFFFFFu)) die("upd_status", i);
        if (st != PKT_FLOW_UPD_OK) continue;
        auto& r = want[f];
        if (r.empty()) r = {0, 0, 0, 0, 10 + i};
        r[dir[i]] += 1;
        r[2 + dir[i]] += w[i];
    }
    uint64_t cnt = 0;
    if (pkt_flow_table_count(t, &cnt, nullptr) || cnt != 64) die("count", cnt);
    if (pkt_flow_table_export(t, nullptr, 0, &cnt, nullptr) || cnt != 64) die("export cap 0", cnt);
    std::vector<pkt_flow_record_t> part(5), rec(64);
    if (pkt_flow_table_export(t, part.data(), 5, &cnt, nullptr) || cnt != 64) die("export cap 5", cnt);
    if (pkt_flow_table_export(t, rec.data(), 64, &cnt, nullptr) || cnt != 64) die("export", cnt);
    if (std::memcmp(part.data(), rec.data(), 5 * sizeof(pkt_flow_record_t)) != 0) die("export prefix", 0);
    for (const auto& r : rec) {
        const auto it = want.find(r.key.src[0]);
        if (it == want.end()) die("exported flow", r.key.src[0]);
        const auto& x = it->second;
        if (r.pkts[0] != x[0] || r.pkts[1] != x[1] || r.bytes[0] != x[2] || r.bytes[1] != x[3] || r.first != x[4])
            die("record", r.key.src[0]);
        want.erase(it);
    }
    if (!want.empty()) die("missing flows", want.size());
    // NULL dir / weight / status / outputs; a falling base; tag bits on a used table; clear
    if (pkt_flow_table_update(t, keys.data(), hash.data(), nullptr, nullptr, nullptr, n, 10 + n, nullptr, nullptr, nullptr)) die("update", 1);
    if (pkt_flow_table_update(t, keys.data(), hash.data(), nullptr, nullptr, nullptr, n, 10, nullptr, nullptr, nullptr) != PKT_ERR_INVALID_ARG)
        die("falling base", 0);
    if (pkt_flow_table_set_tag_bits(t, 2) != PKT_ERR_INVALID_ARG || !std::strlen(pkt_flow_table_last_error(t))) die("tag bits", 0);
    if (pkt_flow_table_clear(t, nullptr) || pkt_flow_table_set_tag_bits(t, 2)) die("clear", 0);
    if (pkt_flow_table_update(t, keys.data(), hash.data(), dir.data(), w.data(), nullptr, n, 0, id.data(), upd.data(), nullptr)) die("update", 2);
    uint64_t ok = 0, coll = 0;
    for (uint64_t i = 0; i < n; i++) ok += upd[i] == PKT_FLOW_UPD_OK, coll += upd[i] == PKT_FLOW_UPD_COLLISION;
    if (pkt_flow_table_count(t, &cnt, nullptr) || cnt != 3 || ok + coll != n || !coll) die("two tag bits", cnt);
    if (pkt_flow_table_destroy(t)) die("destroy", 0);
}

}  // namespace

int main() {
    if (pkt_sizeof_flow_key() != 40 || pkt_sizeof_flow_record() != 80) die("sizeof", 0);
    keys_every_alignment();
    clamp_65535();
    table();
    std::printf("flow OK\n");
    return 0;
}
