// dispatch_host_san.cpp — pkt_dispatch_host and pkt_reorder_host (packet-rs_amd/csrc/pktgpu_host.cpp) under
// AddressSanitizer + UndefinedBehaviorSanitizer: a stand-alone program, no GPU.  Every array is a heap block of
// its exact size (start: nbuckets + 2 words; dst: m * slot bytes; a segmented slot column: 16 * m elements; the
// slab: slab_len bytes, the last packet ending on its last byte), so a store or load one element out is a report.
// It drives DIRECT and table mode at 1, 3 and 256 buckets with drops and a select, every NULL-output combination,
// n in {0, 1, 2, 1000}, and the reorder at every source alignment with cuts, empty positions, empty segments, a
// tail past seg_start[nseg], seg_start values past m, and column subsets; results are checked against a model
// written out here, and the refusals' texts (pktgpu_dispatch.hpp) are checked to carry their call's name.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/pktgpu.h"
#include "../../packet-rs_amd/csrc/pktgpu_dispatch.hpp"

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

template <typename T>
T* block(uint64_t count) {  // exactly count elements (a distinct non-null block for 0)
    return static_cast<T*>(std::malloc(count ? count * sizeof(T) : 1));
}

void dispatch_round(uint32_t nb, const std::vector<uint16_t>* table, uint64_t n, bool with_select) {
    uint32_t* key = block<uint32_t>(n);
    uint8_t* sel = block<uint8_t>(n);
    for (uint64_t i = 0; i < n; i++) {
        key[i] = table ? rnd() : rnd() % (nb + 2);
        sel[i] = rnd() % 5 != 0;
    }
    const uint16_t* tab = table ? table->data() : nullptr;
    const uint32_t tl = table ? (uint32_t)table->size() : 0;
    // the model: b', then a stable counting sort
    std::vector<uint32_t> bp(n);
    std::vector<uint64_t> want_start(nb + 2, 0);
    for (uint64_t i = 0; i < n; i++) {
        uint32_t b = tab ? tab[key[i] & (tl - 1)] : key[i];
        if (b >= nb || (with_select && !sel[i])) b = nb;
        bp[i] = b;
        want_start[b + 1]++;
    }
    for (uint32_t b = 1; b < nb + 2; b++) want_start[b] += want_start[b - 1];
    std::vector<uint32_t> want_perm(n), want_rank(n);
    std::vector<uint64_t> at(want_start.begin(), want_start.end());
    for (uint64_t i = 0; i < n; i++) {
        want_rank[i] = (uint32_t)at[bp[i]]++;
        want_perm[want_rank[i]] = (uint32_t)i;
    }
    for (uint32_t mask = 0; mask < 16; mask++) {
        uint16_t* bucket = mask & 1 ? block<uint16_t>(n) : nullptr;
        uint32_t* perm = mask & 2 ? block<uint32_t>(n) : nullptr;
        uint32_t* rank = mask & 4 ? block<uint32_t>(n) : nullptr;
        uint64_t* start = mask & 8 ? block<uint64_t>(nb + 2) : nullptr;
        if (pkt_dispatch_host(nb, tab, tl, key, with_select ? sel : nullptr, n, bucket, perm, rank, start) != 0)
            die("pkt_dispatch_host", mask);
        for (uint64_t i = 0; i < n; i++) {
            if (bucket && bucket[i] != (bp[i] == nb ? PKT_DISPATCH_DROP : bp[i])) die("bucket", i);
            if (perm && perm[i] != want_perm[i]) die("perm", i);
            if (rank && rank[i] != want_rank[i]) die("rank", i);
        }
        for (uint32_t b = 0; start && b < nb + 2; b++)
            if (start[b] != want_start[b]) die("start", b);
        std::free(bucket);
        std::free(perm);
        std::free(rank);
        std::free(start);
    }
    std::free(key);
    std::free(sel);
}

// n packets of 1 + (7 i) % 90 bytes, packet i at alignment (i + shift) % 16, the last one ending the slab
struct Batch {
    uint64_t n = 0, slab_len = 0;
    uint8_t* slab = nullptr;
    uint64_t* offs = nullptr;
    uint32_t* lens = nullptr;
    uint8_t *nh = nullptr, *ty = nullptr, *v6 = nullptr;
    uint16_t* of = nullptr;
    uint64_t* mac = nullptr;
    ~Batch() {
        std::free(slab), std::free(offs), std::free(lens), std::free(nh), std::free(ty), std::free(v6), std::free(of),
            std::free(mac);
    }
};

void build(Batch& b, uint64_t n, uint32_t shift) {
    b.n = n;
    b.offs = block<uint64_t>(n);
    b.lens = block<uint32_t>(n);
    uint64_t pos = 0;
    for (uint64_t i = 0; i < n; i++) {
        pos = (pos + 15) / 16 * 16 + (i + shift) % 16;
        b.offs[i] = pos;
        b.lens[i] = 1 + (uint32_t)(7 * i % 90);
        pos += b.lens[i];
    }
    b.slab_len = pos;
    b.slab = block<uint8_t>(pos);
    for (uint64_t k = 0; k < pos; k++) b.slab[k] = (uint8_t)(1 + rnd() % 255);
    b.nh = block<uint8_t>(n), b.ty = block<uint8_t>(16 * n), b.of = block<uint16_t>(16 * n);
    b.v6 = block<uint8_t>(16 * n), b.mac = block<uint64_t>(n);
    for (uint64_t i = 0; i < n; i++) {
        b.nh[i] = (uint8_t)(i % 19);  // some above PKT_MAX_HDRS
        b.mac[i] = ((uint64_t)rnd() << 32) | rnd() | 1;
    }
    for (uint64_t k = 0; k < 16 * n; k++) {
        b.ty[k] = (uint8_t)(1 + rnd() % 21);
        b.of[k] = (uint16_t)(1 + rnd() % 60000);
        b.v6[k] = (uint8_t)(1 + rnd() % 255);
    }
}

constexpr uint8_t kFill = 0x77;

void reorder_round(const Batch& b, uint32_t slot, uint32_t nseg, uint32_t colmask, bool with_bytes) {
    const uint64_t n = b.n, m = n + 5;
    uint32_t* perm = block<uint32_t>(m);
    for (uint64_t k = 0; k < m; k++) perm[k] = k % 6 == 5 ? (uint32_t)(n + rnd() % 3) : rnd() % (uint32_t)n;
    perm[m - 1] = 0xFFFFFFFFu;
    // segments: some empty, the last end below m, or (nseg == 3) values past m
    uint64_t* seg = block<uint64_t>(nseg + 1);
    for (uint32_t s = 0; s <= nseg; s++) seg[s] = nseg == 3 && s >= 2 ? m + 7 * s : (uint64_t)(s / 2) * 2 * (m - 3) / (nseg + 1);
    if (nseg) seg[0] = 0;
    uint8_t* dst = with_bytes ? static_cast<uint8_t*>(std::aligned_alloc(16, m * slot)) : nullptr;
    uint32_t* out_len = with_bytes ? block<uint32_t>(m) : nullptr;
    if (dst) std::memset(dst, kFill, m * slot);
    if (out_len) std::memset(out_len, kFill, m * 4);
    pkt_out_t ci{}, co{};
    uint8_t *o_nh = nullptr, *o_ty = nullptr, *o_v6 = nullptr;
    uint16_t* o_of = nullptr;
    uint64_t* o_mac = nullptr;
    if (colmask & 1) ci.n_hdrs = b.nh, co.n_hdrs = o_nh = block<uint8_t>(m), std::memset(o_nh, kFill, m);
    if (colmask & 2) ci.hdr_type = b.ty, co.hdr_type = o_ty = block<uint8_t>(16 * m), std::memset(o_ty, kFill, 16 * m);
    if (colmask & 4) ci.hdr_off = b.of, co.hdr_off = o_of = block<uint16_t>(16 * m), std::memset(o_of, kFill, 32 * m);
    if (colmask & 8) ci.ipv6_src = b.v6, co.ipv6_src = o_v6 = block<uint8_t>(16 * m), std::memset(o_v6, kFill, 16 * m);
    if (colmask & 16) ci.eth_dst = b.mac, co.eth_dst = o_mac = block<uint64_t>(m), std::memset(o_mac, kFill, 8 * m);
    if (colmask & 32) ci.tcp_src = b.of;  // a source column without an out column: not gathered
    pkt_batch_t pb{b.slab, b.slab_len, b.offs, b.lens, 0, 0, n};
    if (pkt_reorder_host(&pb, &ci, perm, m, nseg ? seg : nullptr, nseg, dst, dst ? m * slot : 0, dst ? slot : 0, out_len, &co) != 0)
        die("pkt_reorder_host", nseg);
    for (uint64_t k = 0; k < m; k++) {
        uint64_t s0 = 0, ns = m;
        bool live = true;
        if (nseg) {
            live = false;
            for (uint32_t s = 0; s < nseg; s++) {
                const uint64_t a = seg[s] < m ? seg[s] : m, e = seg[s + 1] < m ? seg[s + 1] : m;
                if (a <= k && k < e) live = true, s0 = a, ns = e - a;
            }
        }
        const uint64_t p = perm[k];
        const bool empty = p >= n;
        if (dst) {
            uint32_t len = empty ? 0 : (b.lens[p] < slot ? b.lens[p] : slot);
            if (!live) len = 0;
            const uint32_t up = live ? (len + 15) / 16 * 16 : 0;
            if (out_len[k] != (live ? len : 0x77777777u)) die("out_len", k);
            for (uint32_t j = 0; j < slot; j++) {
                const uint8_t w = j < len ? b.slab[b.offs[p] + j] : j < up ? 0 : kFill;
                if (dst[k * slot + j] != w) die("dst byte", k * slot + j);
            }
        }
        const uint32_t rows = (colmask & 1) && !empty ? (b.nh[p] < 16 ? b.nh[p] : 16) : 16;
        if (o_nh && o_nh[k] != (live ? (empty ? 0 : b.nh[p]) : kFill)) die("n_hdrs", k);
        if (o_mac && o_mac[k] != (live ? (empty ? 0 : b.mac[p]) : 0x7777777777777777ull)) die("eth_dst", k);
        for (uint32_t j = 0; j < 16; j++) {
            if (o_v6 && o_v6[16 * k + j] != (live ? (empty ? 0 : b.v6[16 * p + j]) : kFill)) die("ipv6_src", k);
            if (!live || j >= rows) continue;  // (rows at or past n_hdrs may be left unwritten)
            const uint64_t e = 16 * s0 + j * ns + (k - s0);
            if (o_ty && o_ty[e] != (empty ? 0 : b.ty[j * n + p])) die("hdr_type", k);
            if (o_of && o_of[e] != (empty ? 0 : b.of[j * n + p])) die("hdr_off", k);
        }
    }
    std::free(perm), std::free(seg), std::free(dst), std::free(out_len);
    std::free(o_nh), std::free(o_ty), std::free(o_of), std::free(o_v6), std::free(o_mac);
}

bool starts(const char* msg, const char* with) { return msg && std::strncmp(msg, with, std::strlen(with)) == 0; }

void refusals() {
    const uint16_t bad_tab[2] = {0, 3};
    uint32_t key[4] = {0, 1, 2, 3};
    uint64_t start[5];
    std::memset(start, kFill, sizeof start);
    if (!starts(dispatch_create_error(0, nullptr, 0, 1, true), "pkt_dispatch")) die("text nbuckets", 0);
    if (!starts(dispatch_create_error(257, nullptr, 0, 1, true), "pkt_dispatch")) die("text nbuckets", 257);
    if (!starts(dispatch_create_error(3, bad_tab, 3, 1, true), "pkt_dispatch")) die("text table_len", 3);
    if (!starts(dispatch_create_error(3, bad_tab, 2, 1, true), "pkt_dispatch")) die("text entry", 3);
    if (!starts(dispatch_create_error(3, nullptr, 0, 0, true), "pkt_dispatch")) die("text max_n", 0);
    if (!starts(dispatch_create_error(3, nullptr, 0, 1ull << 32, true), "pkt_dispatch")) die("text max_n", 1);
    if (dispatch_create_error(3, nullptr, 0, 0xFFFFFFFFull, true) || dispatch_create_error(256, nullptr, 0, 1, true))
        die("a legal definition refused", 0);
    if (!starts(dispatch_call_error(key, 5, 4, start), "pkt_dispatch_batch")) die("text max_n", 5);
    if (pkt_dispatch_host(0, nullptr, 0, key, nullptr, 4, nullptr, nullptr, nullptr, start) != PKT_ERR_INVALID_ARG) die("nbuckets 0", 0);
    if (pkt_dispatch_host(3, bad_tab, 2, key, nullptr, 4, nullptr, nullptr, nullptr, start) != PKT_ERR_INVALID_ARG) die("entry", 0);
    if (pkt_dispatch_host(3, nullptr, 0, nullptr, nullptr, 4, nullptr, nullptr, nullptr, start) != PKT_ERR_INVALID_ARG) die("key", 0);
    if (pkt_dispatch_host(3, nullptr, 0, key, nullptr, 4, nullptr, nullptr, nullptr,
                          reinterpret_cast<uint64_t*>(reinterpret_cast<uint8_t*>(start) + 4)) != PKT_ERR_INVALID_ARG)
        die("misaligned start", 0);
    for (uint64_t w : start)
        if (w != 0x7777777777777777ull) die("a refusal wrote start", 0);
    Batch b;
    build(b, 4, 0);
    pkt_batch_t pb{b.slab, b.slab_len, b.offs, b.lens, 0, 0, 4};
    uint8_t* dst = static_cast<uint8_t*>(std::aligned_alloc(16, 4 * 32));
    std::memset(dst, kFill, 128);
    if (pkt_reorder_host(&pb, nullptr, key, 4, nullptr, 0, dst, 128, 24, nullptr, nullptr) != PKT_ERR_INVALID_ARG) die("slot 24", 0);
    if (pkt_reorder_host(&pb, nullptr, key, 4, nullptr, 0, dst + 8, 120, 16, nullptr, nullptr) != PKT_ERR_INVALID_ARG) die("dst + 8", 0);
    if (pkt_reorder_host(&pb, nullptr, key, 4, nullptr, 0, dst, 127, 32, nullptr, nullptr) != PKT_ERR_INVALID_ARG) die("dst_len", 0);
    if (pkt_reorder_host(&pb, nullptr, key, 4, nullptr, 2, dst, 128, 32, nullptr, nullptr) != PKT_ERR_INVALID_ARG) die("seg_start", 0);
    if (pkt_reorder_host(&pb, nullptr, nullptr, 4, nullptr, 0, dst, 128, 32, nullptr, nullptr) != PKT_ERR_INVALID_ARG) die("perm", 0);
    if (!starts(reorder_error(&pb, nullptr, key, 4, nullptr, 0, dst, 128, 24, nullptr, nullptr, true), "pkt_reorder_batch")) die("text", 0);
    for (uint32_t k = 0; k < 128; k++)
        if (dst[k] != kFill) die("a refusal wrote dst", k);
    if (pkt_reorder_host(&pb, nullptr, key, 0, nullptr, 0, dst, 128, 32, nullptr, nullptr) != PKT_SUCCESS) die("m == 0", 0);
    std::free(dst);
}

}  // namespace

int main() {
    const std::vector<uint16_t> t1 = {PKT_DISPATCH_DROP};
    std::vector<uint16_t> t128(128), t4096(4096);
    for (uint32_t nb : {1u, 3u, 256u}) {
        for (size_t k = 0; k < t128.size(); k++) t128[k] = k % 9 == 4 ? PKT_DISPATCH_DROP : (uint16_t)(rnd() % nb);
        for (size_t k = 0; k < t4096.size(); k++) t4096[k] = (uint16_t)(k % nb);
        for (uint64_t n : {0ull, 1ull, 2ull, 1000ull})
            for (int sel = 0; sel < 2; sel++) {
                dispatch_round(nb, nullptr, n, sel);
                dispatch_round(nb, &t1, n, sel);
                dispatch_round(nb, &t128, n, sel);
                dispatch_round(nb, &t4096, n, sel);
            }
    }
    for (uint32_t shift = 0; shift < 16; shift++) {
        Batch b;
        build(b, 40 + shift, shift);
        for (uint32_t slot : {16u, 48u, 96u})
            for (uint32_t nseg : {0u, 1u, 3u, 6u, 257u}) {
                reorder_round(b, slot, nseg, 0x3F, true);
                reorder_round(b, slot, nseg, 6 + 8 * (shift & 1), shift % 3 != 0);
                reorder_round(b, slot, nseg, 0, true);
            }
    }
    refusals();
    std::printf("dispatch OK\n");
    return 0;
}
