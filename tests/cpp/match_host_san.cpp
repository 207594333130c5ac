// match_host_san.cpp — pkt_match_host (packet-rs_amd/csrc/pktgpu_host.cpp) under AddressSanitizer +
// UndefinedBehaviorSanitizer: a stand-alone program, no GPU.  Every slab is a heap block of exactly slab_len
// bytes with the last packet ending on its last byte, so a field read past a packet's end is a report.  It drives
// Ether / IPv4 / UDP packets at every alignment (a 42-byte one: the UDP header and its checksum field end on the
// packet's last byte), chains that point past the packet or end one byte past it, n_hdrs = 200, a random
// program of 64 rules and 256 terms over every op with and without NOT, 64-bit fields off a byte boundary, and
// every NULL-output combination; the outputs are checked against an evaluator written out here.
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

struct Batch {
    uint64_t n = 0;
    uint8_t* slab = nullptr;  // exactly slab_len bytes
    uint64_t slab_len = 0;
    std::vector<uint64_t> offs;
    std::vector<uint32_t> lens;
    std::vector<uint8_t> nh, ty;  // chain: [16][n]
    std::vector<uint16_t> of;
    ~Batch() { std::free(slab); }
};

// n packets of 42 + (i % 40) bytes, packet i at alignment i % 16, the last one ending the slab
void build(Batch& b, uint64_t n) {
    b.n = n;
    uint64_t pos = 0;
    for (uint64_t i = 0; i < n; i++) {
        pos = (pos + 15) / 16 * 16 + i % 16;
        b.offs.push_back(pos);
        b.lens.push_back(42 + (uint32_t)(i % 40 == 39 ? 0 : i % 40));
        pos += b.lens.back();
    }
    b.slab_len = pos;
    b.slab = static_cast<uint8_t*>(std::malloc(pos));
    for (uint64_t k = 0; k < pos; k++) b.slab[k] = (uint8_t)rnd();
    b.nh.assign(n, 3);
    b.ty.assign(16 * n, 0);
    b.of.assign(16 * n, 0);
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t len = b.lens[i];
        uint8_t* p = b.slab + b.offs[i];
        p[23] = i % 3 ? 17 : 6;           // protocol
        p[36] = 0, p[37] = (uint8_t)(i % 7 ? 53 : 80);  // UDP dst
        uint16_t udp = 34;
        switch (i % 11) {
            case 3: udp = (uint16_t)(len - 8); break;     // ends on the packet's last byte: present
            case 4: udp = (uint16_t)(len - 7); break;     // one byte past it: absent
            case 5: udp = 65535; break;                   // far past the packet
            case 6: b.nh[i] = 200; break;                 // taken as 16: rows 3.. hold type 0
            default: break;
        }
        b.ty[0 * n + i] = PKT_HDR_ETHER, b.of[0 * n + i] = 0;
        b.ty[1 * n + i] = PKT_HDR_IPV4, b.of[1 * n + i] = i % 11 == 7 ? 60000 : 14;
        b.ty[2 * n + i] = PKT_HDR_UDP, b.of[2 * n + i] = udp;
    }
    // the last length may have been clamped by nothing: the slab ends exactly at the last packet's end
}

const uint8_t kSize[PKT_HDR_COUNT] = {0, 14, 4, 20, 40, 4, 20, 8, 28, 8, 14, 3, 5, 4, 4, 4, 4, 8, 12, 8, 35, 4};

// the contract, bit by bit, with an explicit bound on every byte it reads
bool term_true(const Batch& b, uint64_t i, const pkt_match_term_t& m) {
    const uint32_t len = b.lens[i];
    bool raw;
    if (m.op == PKT_MATCH_LEN) {
        raw = m.a <= len && len <= m.b;
    } else {
        uint32_t nh = b.nh[i] > 16 ? 16 : b.nh[i], cnt = 0;
        int64_t ho = -1;
        for (uint32_t j = 0; j < nh && ho < 0; j++)
            if (b.ty[j * b.n + i] == m.field.hdr_type && cnt++ == m.field.occurrence) ho = b.of[j * b.n + i];
        raw = ho >= 0 && (uint64_t)ho + kSize[m.field.hdr_type] <= len;
        if (raw && m.op != PKT_MATCH_HAS) {
            uint64_t v = 0;
            for (uint32_t q = m.field.start; q <= m.field.end; q++) {
                const uint64_t at = b.offs[i] + (uint64_t)ho + (q >> 3);
                if (at >= b.offs[i] + len || at >= b.slab_len) die("reference read outside the packet", i);
                v = v << 1 | ((b.slab[at] >> (7 - (q & 7))) & 1u);
            }
            const uint32_t w = m.field.end - m.field.start + 1u;
            const uint64_t wm = w >= 64 ? ~0ull : (1ull << w) - 1;
            raw = m.op == PKT_MATCH_EQ ? ((v ^ m.a) & m.b & wm) == 0 : (m.a <= v && v <= m.b);
        }
    }
    return raw != ((m.flags & PKT_MATCH_NOT) != 0);
}

struct Field {
    uint8_t t;
    uint16_t s, e;
};
const Field kFields[] = {{PKT_HDR_ETHER, 0, 47},  {PKT_HDR_ETHER, 4, 67},   {PKT_HDR_ETHER, 111, 111}, {PKT_HDR_IPV4, 72, 79},
                         {PKT_HDR_IPV4, 96, 127}, {PKT_HDR_IPV4, 159, 159}, {PKT_HDR_IPV4, 49, 49},    {PKT_HDR_UDP, 16, 31},
                         {PKT_HDR_UDP, 48, 63},   {PKT_HDR_UDP, 0, 63},     {PKT_HDR_UDP, 63, 63},     {PKT_HDR_TCP, 0, 15}};

pkt_match_term_t random_term(const Batch& b) {
    pkt_match_term_t m;
    std::memset(&m, 0, sizeof m);
    m.op = (uint8_t)(rnd() % 4);
    m.flags = rnd() % 4 == 0 ? PKT_MATCH_NOT : 0;
    if (m.op == PKT_MATCH_LEN) {
        m.a = 42 + rnd() % 30;
        m.b = m.a + rnd() % 20;
        return m;
    }
    const Field& f = kFields[rnd() % (sizeof kFields / sizeof kFields[0])];
    m.field.hdr_type = f.t;
    m.field.occurrence = rnd() % 8 == 0 ? 1 : 0;
    if (m.op == PKT_MATCH_HAS) return m;
    m.field.start = f.s, m.field.end = f.e;
    // a value some packet holds, where the header lies at its usual place
    const uint64_t i = rnd() % b.n;
    const uint32_t at = f.t == PKT_HDR_ETHER ? 0 : f.t == PKT_HDR_IPV4 ? 14 : 34;
    uint64_t v = 0;
    for (uint32_t q = f.s; q <= f.e; q++) v = v << 1 | ((b.slab[b.offs[i] + at + (q >> 3)] >> (7 - (q & 7))) & 1u);
    const uint32_t w = f.e - f.s + 1u;
    if (m.op == PKT_MATCH_EQ) {
        m.a = v;
        m.b = rnd() % 2 ? ~0ull : ~0ull << (rnd() % (w + 1 > 63 ? 63 : w + 1));
    } else {
        const uint64_t d = rnd() % 4096;
        m.a = v > d ? v - d : 0;
        m.b = v + d < v ? ~0ull : v + d;
        if (rnd() % 16 == 0) m.a = m.b + 1;  // lo > hi
    }
    return m;
}

void run(uint64_t n, uint32_t nrules, uint32_t per_rule) {
    Batch b;
    build(b, n);
    std::vector<pkt_match_term_t> terms;
    std::vector<pkt_match_rule_t> rules;
    for (uint32_t r = 0; r < nrules; r++) {
        // every fourth rule shares the previous rule's terms, every fifth has none
        pkt_match_rule_t R{(uint16_t)terms.size(), (uint16_t)per_rule, rnd() % 3};
        if (r % 4 == 3 && r) {
            R.first_term = rules.back().first_term;
        } else if (r % 5 == 4) {
            R.nterms = 0;
        } else {
            for (uint32_t k = 0; k < per_rule; k++) terms.push_back(random_term(b));
        }
        rules.push_back(R);
    }
    while (terms.size() < 256 && nrules == 64) terms.push_back(random_term(b));  // 256 terms, the tail unused
    const uint32_t nt = (uint32_t)terms.size(), dflt = 9;
    // expected
    std::vector<uint8_t> rule(n), sel(n);
    std::vector<uint32_t> act(n);
    std::vector<uint64_t> bits(n), hits(nrules + 1, 0), bytes(nrules + 1, 0);
    for (uint64_t i = 0; i < n; i++) {
        uint64_t m = 0;
        for (uint32_t r = 0; r < nrules; r++) {
            bool all = true;
            for (uint32_t k = 0; k < rules[r].nterms; k++) all = all && term_true(b, i, terms[rules[r].first_term + k]);
            if (all) m |= 1ull << r;
        }
        const uint32_t first = m ? (uint32_t)__builtin_ctzll(m) : PKT_MATCH_NONE;
        bits[i] = m, rule[i] = (uint8_t)first, act[i] = m ? rules[first].action : dflt, sel[i] = act[i] != 0;
        hits[m ? first : nrules]++;
        bytes[m ? first : nrules] += b.lens[i];
    }
    pkt_batch_t pb;
    std::memset(&pb, 0, sizeof pb);
    pb.slab = b.slab, pb.slab_len = b.slab_len, pb.offsets = b.offs.data(), pb.lens = b.lens.data(), pb.n = n;
    const pkt_chain_t ch{b.nh.data(), b.ty.data(), b.of.data()};
    for (uint32_t mask = 0; mask < 64; mask++) {  // every NULL-output combination, heap outputs of exact size
        uint8_t* g_rule = mask & 1 ? static_cast<uint8_t*>(std::malloc(n)) : nullptr;
        uint32_t* g_act = mask & 2 ? static_cast<uint32_t*>(std::malloc(4 * n)) : nullptr;
        uint8_t* g_sel = mask & 4 ? static_cast<uint8_t*>(std::malloc(n)) : nullptr;
        uint64_t* g_bits = mask & 8 ? static_cast<uint64_t*>(std::malloc(8 * n)) : nullptr;
        uint64_t* g_hits = mask & 16 ? static_cast<uint64_t*>(std::calloc(nrules + 1, 8)) : nullptr;
        uint64_t* g_bytes = mask & 32 ? static_cast<uint64_t*>(std::calloc(nrules + 1, 8)) : nullptr;
        for (int rep = 1; rep <= 2; rep++) {  // the counters accumulate
            const int rc = pkt_match_host(terms.data(), nt, rules.data(), nrules, dflt, &pb, &ch, g_rule, g_act, g_sel,
                                          g_bits, g_hits, g_bytes);
            if (rc != PKT_SUCCESS) die("pkt_match_host", mask);
            for (uint64_t i = 0; i < n; i++) {
                if (g_rule && g_rule[i] != rule[i]) die("rule", i);
                if (g_act && g_act[i] != act[i]) die("action", i);
                if (g_sel && g_sel[i] != sel[i]) die("select", i);
                if (g_bits && g_bits[i] != bits[i]) die("matched", i);
            }
            for (uint32_t r = 0; r <= nrules; r++) {
                if (g_hits && g_hits[r] != rep * hits[r]) die("hits", r);
                if (g_bytes && g_bytes[r] != rep * bytes[r]) die("bytes", r);
            }
        }
        std::free(g_rule), std::free(g_act), std::free(g_sel), std::free(g_bits), std::free(g_hits), std::free(g_bytes);
    }
}

}  // namespace

int main() {
    if (pkt_sizeof_match_term() != 32 || pkt_sizeof_match_rule() != 8) die("struct sizes", 0);
    run(1, 1, 1);
    run(97, 5, 3);
    run(200, 64, 5);   // 64 rules; 256 terms
    run(64, 0, 0);     // no rules
    std::printf("match OK\n");
    return 0;
}
