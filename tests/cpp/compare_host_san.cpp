// compare_host_san.cpp — pkt_compare_host (packet-rs_amd/csrc/pktgpu_host.cpp) under AddressSanitizer +
// UndefinedBehaviorSanitizer: a stand-alone program, no GPU.  Every slab is a heap block of exactly
// slab_len bytes, so a read past a clamped packet's end is a report.  It drives the edge lengths at
// every pair of alignments, packets running past the slab end on either side, slots wholly past it,
// NULL outputs, and ignore specs whose ranges start in, straddle and lie past the packet; each result is
// checked against a bit-by-bit walk of the definition.
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
    std::printf("FAIL %s at pair %llu\n", what, (unsigned long long)i);
    std::exit(1);
}

struct Side {
    uint8_t* slab;  // exactly slab_len bytes on the heap
    uint64_t slab_len;
    std::vector<uint64_t> offs;
    std::vector<uint32_t> lens;
    pkt_batch_t batch() const {
        pkt_batch_t b{};
        b.slab = slab;
        b.slab_len = slab_len;
        b.offsets = offs.data();
        b.lens = lens.data();
        b.n = offs.size();
        return b;
    }
    uint32_t len(uint64_t i) const {
        const uint64_t room = offs[i] < slab_len ? slab_len - offs[i] : 0;
        uint64_t l = lens[i] > room ? room : lens[i];
        return l > 65535 ? 65535u : (uint32_t)l;
    }
};

// the definition, bit by bit: ign_lo/ign_hi = packet i's resolved ranges (lo > hi: none)
void check(const Side& a, const Side& b, const std::vector<uint8_t>& res, const std::vector<uint32_t>& mt,
           const std::vector<uint32_t>& fd, const pkt_cmp_summary_t& sm, uint32_t nr, const uint32_t* lo,
           const uint32_t* hi) {
    const uint64_t n = a.offs.size();
    pkt_cmp_summary_t want{0, 0, 0, n};
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t la = a.len(i), lb = b.len(i), m = la < lb ? la : lb;
        uint32_t cnt = 0, first = m;
        for (uint32_t j = 0; j < m; j++) {
            bool same = true;
            for (uint32_t t = 8 * j; t < 8 * j + 8; t++) {
                bool ign = false;
                for (uint32_t r = 0; r < nr; r++) ign = ign || (lo[r * n + i] <= t && t <= hi[r * n + i]);
                const uint32_t sh = 7 - t % 8;
                if (!ign && ((a.slab[a.offs[i] + j] >> sh) & 1) != ((b.slab[b.offs[i] + j] >> sh) & 1)) same = false;
            }
            if (same)
                cnt++;
            else if (first == m)
                first = j;
        }
        const uint8_t r = la != lb ? PKT_CMP_LEN : cnt != la ? PKT_CMP_BYTES : PKT_CMP_EQUAL;
        if (res[i] != r) die("result", i);
        if (mt[i] != cnt) die("matching", i);
        if (fd[i] != first) die("first_diff", i);
        (r == PKT_CMP_EQUAL ? want.n_equal : r == PKT_CMP_LEN ? want.n_len : want.n_bytes)++;
        if (r != PKT_CMP_EQUAL && want.first_bad == n) want.first_bad = i;
    }
    if (std::memcmp(&want, &sm, sizeof sm) != 0) die("summary", n);
}

void run(const Side& a, const Side& b, const pkt_chain_t* ch, const pkt_field_spec_t* ign, uint32_t nign,
         const uint32_t* lo, const uint32_t* hi) {
    const uint64_t n = a.offs.size();
    std::vector<uint8_t> res(n);
    std::vector<uint32_t> mt(n), fd(n);
    pkt_cmp_summary_t sm, sm2;
    const pkt_batch_t ba = a.batch(), bb = b.batch();
    if (pkt_compare_host(&ba, &bb, ch, ign, nign, res.data(), mt.data(), fd.data(), &sm) != PKT_SUCCESS) die("rc", 0);
    check(a, b, res, mt, fd, sm, nign, lo, hi);
    if (pkt_compare_host(&ba, &bb, ch, ign, nign, nullptr, nullptr, nullptr, &sm2) != PKT_SUCCESS) die("rc", 1);
    if (std::memcmp(&sm, &sm2, sizeof sm) != 0) die("summary without outputs", 0);
    if (pkt_compare_host(&ba, &bb, ch, ign, nign, res.data(), nullptr, nullptr, nullptr) != PKT_SUCCESS) die("rc", 2);
}

Side make(uint64_t slab_len) {
    Side s;
    s.slab = static_cast<uint8_t*>(std::malloc(slab_len ? slab_len : 1));
    s.slab_len = slab_len;
    for (uint64_t k = 0; k < slab_len; k++) s.slab[k] = (uint8_t)rnd();
    return s;
}

}  // namespace

int main() {
    static const uint32_t kLens[] = {0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 4095, 4096, 4097, 65535};
    // (1) the edge lengths at every pair of alignments: equal, one byte flipped, b shorter
    {
        Side a = make(1 << 20), b = make((1 << 20) + 77);
        for (uint32_t ln : kLens)
            for (uint32_t al = 0; al < 256; al += ln > 100 ? 37 : 1) {
                const uint64_t oa = 4096 + (rnd() % 900000 & ~15u) + (al >> 4), ob = 4096 + (rnd() % 900000 & ~15u) + (al & 15);
                const uint32_t cut = ln && al % 5 == 0 ? rnd() % ln : ln;
                std::memcpy(b.slab + ob, a.slab + oa, ln);
                if (ln && al % 3 == 0) b.slab[ob + (al % 2 ? ln - 1 : rnd() % ln)] ^= 0x40;
                a.offs.push_back(oa), a.lens.push_back(ln);
                b.offs.push_back(ob), b.lens.push_back(cut);
            }
        run(a, b, nullptr, nullptr, 0, nullptr, nullptr);
        run(a, a, nullptr, nullptr, 0, nullptr, nullptr);  // the same buffer on both sides
        std::free(a.slab), std::free(b.slab);
    }
    // (2) the slab end: packets running past it on either side, slots at and past it, huge lens
    {
        Side a = make(1000), b = make(977);
        std::memcpy(b.slab, a.slab, 900);
        const uint64_t offs[] = {10, 900, 1000, 5000, 999, 0, 850, 976, 977, 1ull << 40, 990};
        const uint32_t lens[] = {50, 200, 50, 10, 70000, 70000, 150, 1, 1, 64, 0xFFFFFFFFu};
        for (int k = 0; k < 11; k++) {
            a.offs.push_back(offs[k]), a.lens.push_back(lens[k]);
            b.offs.push_back(offs[k]), b.lens.push_back(lens[k]);
        }
        run(a, b, nullptr, nullptr, 0, nullptr, nullptr);
        run(b, a, nullptr, nullptr, 0, nullptr, nullptr);
        // fixed stride with n past the slab
        pkt_batch_t fa{}, fb{};
        fa.slab = a.slab, fa.slab_len = 1000, fa.stride = 64, fa.n = 18;
        fb.slab = b.slab, fb.slab_len = 970, fb.stride = 64, fb.n = 18;
        std::vector<uint8_t> res(18);
        std::vector<uint32_t> mt(18), fd(18);
        pkt_cmp_summary_t sm;
        if (pkt_compare_host(&fa, &fb, nullptr, nullptr, 0, res.data(), mt.data(), fd.data(), &sm) != PKT_SUCCESS) die("rc", 3);
        if (res[15] != PKT_CMP_LEN || mt[15] > 10 || res[16] != PKT_CMP_EQUAL || mt[17] != 0 || sm.n_len != 1) die("fixed", 15);
        std::free(a.slab), std::free(b.slab);
    }
    // (3) ignores: a two-header chain per packet (type 1 at 0, type 3 at a random offset, sometimes past
    // the packet), 16 specs whose ranges start inside, straddle the end of, and lie past the packet
    {
        const uint64_t n = 600;
        Side a = make(200000), b = make(200000);
        std::vector<uint8_t> nh(n), ty(PKT_MAX_HDRS * n);
        std::vector<uint16_t> of(PKT_MAX_HDRS * n);
        for (uint64_t i = 0; i < n; i++) {
            const uint32_t ln = i % 50 == 0 ? 5000 : rnd() % 130;
            const uint64_t oa = 300 * i + rnd() % 16, ob = 300 * i + rnd() % 16;
            if (i % 50) {
                std::memcpy(b.slab + ob, a.slab + oa, ln);
                for (int k = 0; k < 3 && ln; k++) b.slab[ob + rnd() % ln] ^= (uint8_t)(1u << (rnd() % 8));
            }
            a.offs.push_back(oa), a.lens.push_back(ln);
            b.offs.push_back(ob), b.lens.push_back(i % 7 == 0 && ln ? ln - rnd() % ln : ln);
            nh[i] = (uint8_t)(i % 5 == 0 ? 0 : i % 5 == 1 ? 1 : i % 5 == 2 ? 20 : 3);  // 20: clamped to 16 slots
            ty[0 * n + i] = 1, of[0 * n + i] = 0;
            ty[1 * n + i] = 3, of[1 * n + i] = (uint16_t)(rnd() % 140);
            ty[2 * n + i] = 3, of[2 * n + i] = (uint16_t)(i % 11 == 0 ? 65535 : rnd() % 140);
        }
        pkt_field_spec_t sp[16];
        for (uint32_t s = 0; s < 16; s++) {
            sp[s].hdr_type = (uint8_t)(s % 3 == 0 ? 1 : s % 3 == 1 ? 3 : 7);  // 7: in no chain
            sp[s].occurrence = (uint8_t)(s % 3 == 1 ? (s / 3) % 3 : 0);
            sp[s].start = (uint16_t)(s == 15 ? 0 : rnd() % 600);
            sp[s].end = (uint16_t)(s == 15 ? 65535 : s == 14 ? sp[s].start : sp[s].start + rnd() % 300);
            sp[s].reserved = 0;
        }
        sp[15].hdr_type = 3, sp[15].occurrence = 1;
        for (uint32_t nign : {1u, 5u, 15u, 16u}) {
            std::vector<uint32_t> lo(nign * n, 1), hi(nign * n, 0);
            for (uint32_t s = 0; s < nign; s++)
                for (uint64_t i = 0; i < n; i++) {
                    uint32_t seen = 0;
                    for (uint32_t j = 0; j < (nh[i] > 16u ? 16u : nh[i]); j++)
                        if (j < 3 && ty[j * n + i] == sp[s].hdr_type && seen++ == sp[s].occurrence) {
                            lo[s * n + i] = 8u * of[j * n + i] + sp[s].start;
                            hi[s * n + i] = 8u * of[j * n + i] + sp[s].end;
                        }
                }
            const pkt_chain_t ch{nh.data(), ty.data(), of.data()};
            run(a, b, &ch, sp, nign, lo.data(), hi.data());
        }
        // argument errors
        const pkt_batch_t ba = a.batch(), bb = b.batch();
        pkt_batch_t shorter = bb;
        shorter.n = n - 1;
        const pkt_chain_t ch{nh.data(), ty.data(), of.data()};
        pkt_field_spec_t bad = sp[0];
        bad.start = 9, bad.end = 8;
        if (pkt_compare_host(&ba, &shorter, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr) != PKT_ERR_INVALID_ARG ||
            pkt_compare_host(&ba, &bb, nullptr, sp, 1, nullptr, nullptr, nullptr, nullptr) != PKT_ERR_INVALID_ARG ||
            pkt_compare_host(&ba, &bb, &ch, sp, 17, nullptr, nullptr, nullptr, nullptr) != PKT_ERR_INVALID_ARG ||
            pkt_compare_host(&ba, &bb, &ch, &bad, 1, nullptr, nullptr, nullptr, nullptr) != PKT_ERR_INVALID_ARG)
            die("argument errors", 0);
        std::free(a.slab), std::free(b.slab);
    }
    // (4) n == 0
    {
        pkt_batch_t e{};
        pkt_cmp_summary_t sm{9, 9, 9, 9};
        if (pkt_compare_host(&e, &e, nullptr, nullptr, 0, nullptr, nullptr, nullptr, &sm) != PKT_SUCCESS ||
            sm.n_equal || sm.n_len || sm.n_bytes || sm.first_bad)
            die("empty batch", 0);
    }
    std::printf("compare OK\n");
    return 0;
}
