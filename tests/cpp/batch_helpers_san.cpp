// batch_helpers_san.cpp — pkt_off / pkt_len (packet-rs_amd/csrc/pktgpu_batch.hpp) and the three host models that
// call them (pktgpu_host.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer: a stand-alone program, no GPU.
// Every slab and every dst is a heap block of exactly its length, so a length that is not clamped to the slab
// end is a report.  (1) the two rules on the stride form and the indexed form: an offset at the slab end, one
// past it, a length that crosses the slab end, a length above 65535, slab_len 0; (2) pkt_compare_host,
// pkt_pcap_write_host and pkt_edit_host on a 3-packet batch whose last packet the slab end cuts from 16 bytes
// to 8, against bytes written out here.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/pktgpu.h"
#include "../../packet-rs_amd/csrc/pktgpu_batch.hpp"

namespace {

[[noreturn]] void die(const char* what, uint64_t i) {
    std::printf("FAIL %s at %llu\n", what, (unsigned long long)i);
    std::exit(1);
}

uint8_t* block(size_t len, uint8_t fill) {  // exactly len bytes
    uint8_t* p = static_cast<uint8_t*>(std::malloc(len ? len : 1));
    std::memset(p, fill, len);
    return p;
}

void expect(const BatchSrc& s, uint64_t i, uint64_t off, uint32_t len, const char* what) {
    const uint64_t o = pkt_off(s, i);
    if (o != off) die(what, i);
    if (pkt_len(s, i, o) != len) die(what, i);
}

void rules() {
    uint8_t* slab = block(250, 0);
    // stride form: 125-byte slots in 250 bytes (packet 2 starts AT the slab end, packet 3 past it)
    const BatchSrc s125{slab, 250, nullptr, nullptr, 125};
    expect(s125, 0, 0, 125, "stride 125");
    expect(s125, 1, 125, 125, "stride 125");
    expect(s125, 2, 250, 0, "stride 125: offset at the slab end");
    expect(s125, 3, 375, 0, "stride 125: offset past the slab end");
    // 100-byte slots: packet 2 crosses the slab end
    const BatchSrc s100{slab, 250, nullptr, nullptr, 100};
    expect(s100, 2, 200, 50, "stride 100: crosses the slab end");
    expect(s100, 1ull << 40, 100ull << 40, 0, "stride 100: a far index");
    // per-packet lens on a fixed stride
    const uint32_t l3[3] = {7, 0, 0xFFFFFFFFu};
    const BatchSrc sl{slab, 250, nullptr, l3, 100};
    expect(sl, 0, 0, 7, "stride + lens");
    expect(sl, 1, 100, 0, "stride + lens");
    expect(sl, 2, 200, 50, "stride + lens: 2^32 - 1 crosses the slab end");
    // the indexed form
    const uint64_t offs[6] = {0, 240, 249, 250, 251, 1ull << 63};
    const uint32_t lens[6] = {250, 20, 1, 1, 1, 0xFFFFFFFFu};
    const BatchSrc ix{slab, 250, offs, lens, 0};
    expect(ix, 0, 0, 250, "indexed: the whole slab");
    expect(ix, 1, 240, 10, "indexed: crosses the slab end");
    expect(ix, 2, 249, 1, "indexed: the last byte");
    expect(ix, 3, 250, 0, "indexed: offset at the slab end");
    expect(ix, 4, 251, 0, "indexed: offset past the slab end");
    expect(ix, 5, 1ull << 63, 0, "indexed: offset far past the slab end");
    // slab_len 0 (no slab at all)
    const BatchSrc none{nullptr, 0, offs, lens, 0}, none_s{nullptr, 0, nullptr, nullptr, 64};
    for (uint64_t i = 0; i < 6; i++) expect(none, i, offs[i], 0, "slab_len 0, indexed");
    expect(none_s, 0, 0, 0, "slab_len 0, stride");
    expect(none_s, 9, 576, 0, "slab_len 0, stride");
    std::free(slab);
    // above 65535: 70000-byte slots in 200000 bytes, and lens above it
    uint8_t* big = block(200000, 0);
    const BatchSrc s70k{big, 200000, nullptr, nullptr, 70000};
    expect(s70k, 0, 0, 65535, "stride 70000: above 65535");
    expect(s70k, 1, 70000, 65535, "stride 70000: above 65535");
    expect(s70k, 2, 140000, 60000, "stride 70000: the slab end below 65535");
    const uint64_t boffs[3] = {0, 100000, 134465};
    const uint32_t blens[3] = {65536, 0xFFFFFFFFu, 70000};
    const BatchSrc bix{big, 200000, boffs, blens, 0};
    expect(bix, 0, 0, 65535, "indexed: 65536");
    expect(bix, 1, 100000, 65535, "indexed: 2^32 - 1");
    expect(bix, 2, 134465, 65535, "indexed: exactly 65535 left");
    // batch_src copies the five fields
    pkt_batch_t b{};
    b.slab = big, b.slab_len = 200000, b.offsets = boffs, b.lens = blens, b.stride = 3, b.n = 3;
    const BatchSrc c = batch_src(&b);
    if (c.slab != big || c.slab_len != 200000 || c.offsets != boffs || c.lens != blens || c.stride != 3) die("batch_src", 0);
    std::free(big);
}

// three 16-byte packets at 0, 16 and 32 of a 40-byte slab (byte k = k): the last is cut to 8 bytes
const uint64_t kOffs[3] = {0, 16, 32};
const uint32_t kLens[3] = {16, 16, 16};

void models() {
    uint8_t* slab = block(40, 0);
    for (int k = 0; k < 40; k++) slab[k] = (uint8_t)k;
    pkt_batch_t a{};
    a.slab = slab, a.slab_len = 40, a.offsets = kOffs, a.lens = kLens, a.n = 3;

    // pkt_pcap_write_host: 24 + (16 + 16) + (16 + 16) + (16 + 8) bytes
    {
        static const uint8_t want[112] = {
            0xD4, 0xC3, 0xB2, 0xA1, 2, 0, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0xFF, 0xFF, 0, 0, 1, 0, 0, 0,
            1, 0, 0, 0, 2, 0, 0, 0, 16, 0, 0, 0, 16, 0, 0, 0,
            0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15,
            1, 0, 0, 0, 2, 0, 0, 0, 16, 0, 0, 0, 16, 0, 0, 0,
            16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31,
            1, 0, 0, 0, 2, 0, 0, 0, 8, 0, 0, 0, 8, 0, 0, 0,
            32, 33, 34, 35, 36, 37, 38, 39};
        uint8_t* dst = block(112, 0x5A);
        uint64_t ro[3], bytes = 0, cnt = 0;
        uint32_t rl[3], si[3];
        if (pkt_pcap_write_host(&a, nullptr, 0, 1, 2, nullptr, nullptr, dst, 112, ro, rl, si, &bytes, &cnt) != PKT_SUCCESS) die("pcap rc", 0);
        if (bytes != 112 || cnt != 3) die("pcap totals", bytes);
        if (std::memcmp(dst, want, 112) != 0) die("pcap bytes", 0);
        if (ro[0] != 40 || ro[1] != 72 || ro[2] != 104 || rl[0] != 16 || rl[1] != 16 || rl[2] != 8) die("pcap record table", 0);
        if (si[0] != 0 || si[1] != 1 || si[2] != 2) die("pcap src_index", 0);
        // one byte short: refused with the size, nothing written past dst
        if (pkt_pcap_write_host(&a, nullptr, 0, 1, 2, nullptr, nullptr, dst, 111, nullptr, nullptr, nullptr, &bytes, &cnt) != PKT_ERR_INVALID_ARG ||
            bytes != 112)
            die("pcap short dst", bytes);
        std::free(dst);
    }

    // pkt_compare_host against 16-byte slots of a 39-byte slab that differs in packet 1's byte 1: the last pair
    // is 8 bytes against 7
    {
        uint8_t* other = block(39, 0);
        for (int k = 0; k < 39; k++) other[k] = (uint8_t)k;
        other[17] ^= 0x80;
        pkt_batch_t b{};
        b.slab = other, b.slab_len = 39, b.stride = 16, b.n = 3;
        uint8_t res[3];
        uint32_t mt[3], fd[3];
        pkt_cmp_summary_t sum{};
        if (pkt_compare_host(&a, &b, nullptr, nullptr, 0, res, mt, fd, &sum) != PKT_SUCCESS) die("compare rc", 0);
        if (res[0] != PKT_CMP_EQUAL || res[1] != PKT_CMP_BYTES || res[2] != PKT_CMP_LEN) die("compare result", 0);
        if (mt[0] != 16 || mt[1] != 15 || mt[2] != 7) die("compare matching", 0);
        if (fd[0] != 16 || fd[1] != 1 || fd[2] != 7) die("compare first_diff", 0);
        if (sum.n_equal != 1 || sum.n_bytes != 1 || sum.n_len != 1 || sum.first_bad != 1) die("compare summary", 0);
        // against itself: all equal, the last pair on its 8 bytes
        if (pkt_compare_host(&a, &a, nullptr, nullptr, 0, res, mt, fd, &sum) != PKT_SUCCESS) die("compare rc", 1);
        if (sum.n_equal != 3 || sum.first_bad != 3 || mt[2] != 8 || fd[2] != 8) die("compare with itself", 0);
        std::free(other);
    }

    // pkt_edit_host: Ether [0, 14) and 2 payload bytes per packet; the cut packet has 8 header bytes and no payload
    {
        const uint8_t status[3] = {PKT_OK, PKT_OK, PKT_OK}, n_hdrs[3] = {1, 1, 1};
        uint8_t hdr_type[PKT_MAX_HDRS * 3] = {PKT_HDR_ETHER, PKT_HDR_ETHER, PKT_HDR_ETHER};
        uint16_t hdr_off[PKT_MAX_HDRS * 3] = {0, 0, 0};
        const uint16_t pay_off[3] = {14, 14, 14}, pay_len[3] = {2, 2, 2};
        pkt_out_t parsed{};
        parsed.status = const_cast<uint8_t*>(status), parsed.n_hdrs = const_cast<uint8_t*>(n_hdrs);
        parsed.hdr_type = hdr_type, parsed.hdr_off = hdr_off;
        parsed.payload_off = const_cast<uint16_t*>(pay_off), parsed.payload_len = const_cast<uint16_t*>(pay_len);
        uint32_t out_len[3];
        uint8_t st[3];
        // no ops: to_vec of every packet in 16-byte slots
        static const uint8_t copy[48] = {0,  1,  2,  3,  4,  5,  6,  7,  8,    9,    10,   11,   12,   13,   14,   15,
                                         16, 17, 18, 19, 20, 21, 22, 23, 24,   25,   26,   27,   28,   29,   30,   31,
                                         32, 33, 34, 35, 36, 37, 38, 39, 0x5A, 0x5A, 0x5A, 0x5A, 0x5A, 0x5A, 0x5A, 0x5A};
        uint8_t* dst = block(48, 0x5A);
        if (pkt_edit_host(&a, &parsed, nullptr, 0, nullptr, 0, nullptr, dst, 48, nullptr, 16, out_len, st, nullptr) != PKT_SUCCESS) die("edit rc", 0);
        if (std::memcmp(dst, copy, 48) != 0) die("edit bytes (no ops)", 0);
        if (out_len[0] != 16 || out_len[1] != 16 || out_len[2] != 8) die("edit out_len (no ops)", 0);
        if (st[0] != PKT_EDIT_OK || st[1] != PKT_EDIT_OK || st[2] != PKT_EDIT_OK) die("edit status (no ops)", 0);
        // pop: the payloads alone
        static const uint8_t popped[48] = {14,   15,   0x5A, 0x5A, 0x5A, 0x5A, 0x5A, 0x5A, 0x5A, 0x5A, 0x5A, 0x5A, 0x5A, 0x5A, 0x5A, 0x5A,
                                           30,   31,   0x5A, 0x5A, 0x5A, 0x5A, 0x5A, 0x5A, 0x5A, 0x5A, 0x5A, 0x5A, 0x5A, 0x5A, 0x5A, 0x5A,
                                           0x5A, 0x5A, 0x5A, 0x5A, 0x5A, 0x5A, 0x5A, 0x5A, 0x5A, 0x5A, 0x5A, 0x5A, 0x5A, 0x5A, 0x5A, 0x5A};
        std::memset(dst, 0x5A, 48);
        const pkt_edit_op_t pop{PKT_EDIT_POP, 0, 0, 0, 0};
        if (pkt_edit_host(&a, &parsed, &pop, 1, nullptr, 0, nullptr, dst, 48, nullptr, 16, out_len, st, nullptr) != PKT_SUCCESS) die("edit rc", 1);
        if (std::memcmp(dst, popped, 48) != 0) die("edit bytes (pop)", 0);
        if (out_len[0] != 2 || out_len[1] != 2 || out_len[2] != 0) die("edit out_len (pop)", 0);
        std::free(dst);
    }
    std::free(slab);
}

}  // namespace

int main() {
    rules();
    models();
    std::printf("batch helpers OK\n");
    return 0;
}
