// edit_host_san.cpp — pkt_edit_host (packet-rs_amd/csrc/pktgpu_host.cpp) under AddressSanitizer +
// UndefinedBehaviorSanitizer: a stand-alone program, no GPU.  Every slab and every dst is a heap block of
// exactly its length, so a read past a clamped packet's end or a write past a slot's room is a report.
// It drives (1) the two-segment strip and the constant-plus-segment insert at every pair of source and
// destination alignments and the edge lengths, (2) rooms one byte short, exact and past dst_len, (3) the
// 16-header list with an insert before and after a remove, and (4) chain columns that are no parse of the
// batch (offsets and lengths past the packet, n_hdrs past 16, unknown types).  The outputs of (1)-(3)
// are checked byte by byte against the edit written out by hand.
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
    std::printf("FAIL %s at packet %llu\n", what, (unsigned long long)i);
    std::exit(1);
}

struct Batch {
    std::vector<uint8_t> bytes;  // copied to an exact heap block by run()
    std::vector<uint64_t> offs;
    std::vector<uint32_t> lens;
    std::vector<uint8_t> status, n_hdrs, hdr_type;
    std::vector<uint16_t> hdr_off, payload_off, payload_len;
    std::vector<std::vector<uint8_t>> want;  // expected output per packet
    std::vector<uint8_t> want_status;
    // Ether [0,14), ntags Vlan tags, payload: the chain a parse would give
    void add(uint32_t ntags, uint32_t payload, uint32_t align) {
        while (bytes.size() % 16 != align) bytes.push_back((uint8_t)rnd());
        offs.push_back(bytes.size());
        const uint32_t len = 14 + 4 * ntags + payload;
        lens.push_back(len);
        for (uint32_t k = 0; k < len; k++) bytes.push_back((uint8_t)rnd());
        status.push_back(PKT_OK);
        n_hdrs.push_back((uint8_t)(1 + ntags));
        payload_off.push_back((uint16_t)(14 + 4 * ntags));
        payload_len.push_back((uint16_t)payload);
    }
    void finish() {  // the slot-major columns
        const size_t n = offs.size();
        hdr_type.assign(PKT_MAX_HDRS * n, 0);
        hdr_off.assign(PKT_MAX_HDRS * n, 0);
        for (size_t i = 0; i < n; i++)
            for (uint32_t j = 0; j < n_hdrs[i] && j < PKT_MAX_HDRS; j++) {
                hdr_type[j * n + i] = j ? PKT_HDR_VLAN : PKT_HDR_ETHER;
                hdr_off[j * n + i] = (uint16_t)(j ? 14 + 4 * (j - 1) : 0);
            }
    }
    const uint8_t* pkt(size_t i) const { return bytes.data() + offs[i]; }
};

// runs the program; checks want / want_status when given, and that nothing outside the packets is written
void run(const Batch& B, const std::vector<pkt_edit_op_t>& ops, const std::vector<uint8_t>& data,
         const std::vector<uint64_t>& dst_offs, uint32_t slot, uint64_t dst_len, const uint8_t* select, bool check) {
    const size_t n = B.offs.size();
    uint8_t* slab = static_cast<uint8_t*>(std::malloc(B.bytes.size() ? B.bytes.size() : 1));
    std::memcpy(slab, B.bytes.data(), B.bytes.size());
    uint8_t* dst = static_cast<uint8_t*>(std::malloc(dst_len ? dst_len : 1));
    std::memset(dst, 0x5A, dst_len);
    uint8_t* hd = static_cast<uint8_t*>(std::malloc(data.size() ? data.size() : 1));  // exactly hdr_data_len
    if (!data.empty()) std::memcpy(hd, data.data(), data.size());
    pkt_batch_t b{};
    b.slab = slab, b.slab_len = B.bytes.size(), b.offsets = B.offs.data(), b.lens = B.lens.data(), b.n = n;
    pkt_out_t parsed{};
    parsed.status = const_cast<uint8_t*>(B.status.data());
    parsed.n_hdrs = const_cast<uint8_t*>(B.n_hdrs.data());
    parsed.hdr_type = const_cast<uint8_t*>(B.hdr_type.data());
    parsed.hdr_off = const_cast<uint16_t*>(B.hdr_off.data());
    parsed.payload_off = const_cast<uint16_t*>(B.payload_off.data());
    parsed.payload_len = const_cast<uint16_t*>(B.payload_len.data());
    std::vector<uint32_t> out_len(n);
    std::vector<uint8_t> st(n), c_status(n), c_nh(n), c_ty(PKT_MAX_HDRS * n);
    std::vector<uint16_t> c_of(PKT_MAX_HDRS * n), c_po(n), c_pl(n);
    std::vector<uint32_t> c_mask(n);
    pkt_out_t oc{};
    oc.status = c_status.data(), oc.n_hdrs = c_nh.data(), oc.hdr_type = c_ty.data(), oc.hdr_off = c_of.data();
    oc.payload_off = c_po.data(), oc.payload_len = c_pl.data(), oc.hdr_mask = c_mask.data();
    if (pkt_edit_host(&b, &parsed, ops.data(), (uint32_t)ops.size(), hd, (uint32_t)data.size(), select, dst, dst_len,
                      dst_offs.empty() ? nullptr : dst_offs.data(), slot, out_len.data(), st.data(), &oc) != PKT_SUCCESS)
        die("rc", 0);
    std::vector<uint8_t> touched(dst_len, 0);
    for (size_t i = 0; i < n; i++) {
        const uint64_t o = dst_offs.empty() ? i * slot : dst_offs[i];
        const uint64_t room = o >= dst_len ? 0 : (dst_len - o < slot ? dst_len - o : slot);
        if (out_len[i] > room) die("out_len past the room", i);
        if ((st[i] != PKT_EDIT_OK) != (c_status[i] != PKT_OK) && B.status[i] == PKT_OK) die("chain status", i);
        if (st[i] != PKT_EDIT_OK && (out_len[i] || c_nh[i] || c_po[i] || c_pl[i] || c_mask[i])) die("failed packet's columns", i);
        if (st[i] == PKT_EDIT_OK && (uint32_t)c_po[i] + c_pl[i] != out_len[i]) die("payload_off + payload_len", i);
        for (uint64_t k = 0; k < out_len[i]; k++) touched[o + k] = 1;
        if (!check) continue;
        if (st[i] != B.want_status[i]) die("status", i);
        if (st[i] != PKT_EDIT_OK) continue;
        if (out_len[i] != B.want[i].size()) die("out_len", i);
        if (out_len[i] && std::memcmp(dst + o, B.want[i].data(), out_len[i]) != 0) die("bytes", i);
    }
    for (uint64_t k = 0; k < dst_len; k++)
        if (!touched[k] && dst[k] != 0x5A) die("a byte outside the packets was written", k);
    // NULL outputs
    if (pkt_edit_host(&b, &parsed, ops.data(), (uint32_t)ops.size(), hd, (uint32_t)data.size(), select, dst, dst_len,
                      dst_offs.empty() ? nullptr : dst_offs.data(), slot, nullptr, nullptr, nullptr) != PKT_SUCCESS)
        die("rc without outputs", 0);
    std::free(slab), std::free(dst), std::free(hd);
}

pkt_edit_op_t op(uint8_t kind, uint8_t type, uint8_t index, uint32_t data_off = 0) { return pkt_edit_op_t{kind, type, index, 0, data_off}; }

const std::vector<uint8_t> kMpls = {0x12, 0x34, 0x51, 0x40};

}  // namespace

int main() {
    static const uint32_t kLens[] = {15, 16, 17, 31, 32, 33, 63, 64, 65, 4095, 4096, 4097, 65535};
    // (1) every pair of alignments: the strip [0,14) + [18, len), and the Ether header replaced by four constant bytes
    for (int insert = 0; insert < 2; insert++) {
        Batch B;
        std::vector<uint64_t> dst_offs;
        uint64_t pos = 0;
        for (uint32_t ln : kLens)
            for (uint32_t al = 0; al < 256; al += ln > 100 ? 37 : 1) {
                if (insert)
                    B.add(0, ln == 65535 ? ln - 14 : ln - 4, al >> 4);   // output ln (65535: 65525)
                else
                    B.add(1, ln == 65535 ? ln - 18 : ln - 14, al >> 4);  // output ln (65535: 65531)
                dst_offs.push_back(((pos + 15) & ~15ull) + (al & 15));
                pos = dst_offs.back() + ln + 8;
            }
        B.finish();
        for (size_t i = 0; i < B.offs.size(); i++) {
            const uint8_t* p = B.pkt(i);
            std::vector<uint8_t> w;
            if (insert) {
                w = kMpls;
                w.insert(w.end(), p + 14, p + B.lens[i]);
            } else {
                w.assign(p, p + 14);
                w.insert(w.end(), p + 18, p + B.lens[i]);
            }
            B.want.push_back(w);
            B.want_status.push_back(PKT_EDIT_OK);
        }
        if (insert)
            run(B, {op(PKT_EDIT_REMOVE_AT, 0, 0), op(PKT_EDIT_INSERT, PKT_HDR_MPLS, 0)}, kMpls, dst_offs, 65535, pos, nullptr, true);
        else
            run(B, {op(PKT_EDIT_REMOVE_HDR, PKT_HDR_VLAN, 0)}, {}, dst_offs, 65535, pos, nullptr, true);
    }
    // an insert that takes a 65535-byte packet, and only it, past 65535
    {
        Batch B;
        B.add(1, 65535 - 18, 5);
        B.add(1, 46, 11);
        B.finish();
        for (size_t i = 0; i < 2; i++) {
            const uint8_t* p = B.pkt(i);
            std::vector<uint8_t> w(p, p + 14);
            w.insert(w.end(), kMpls.begin(), kMpls.end());
            w.insert(w.end(), p + 14, p + B.lens[i]);
            B.want.push_back(w);
            B.want_status.push_back(i == 0 ? PKT_EDIT_NO_ROOM : PKT_EDIT_OK);
        }
        run(B, {op(PKT_EDIT_INSERT, PKT_HDR_MPLS, 1)}, kMpls, {}, 70000, 140000, nullptr, true);
    }
    // (2) rooms: a fixed slot of 100 with outputs of 99, 100, 101; dst_len cutting the last slot; offsets at and past dst_len
    {
        Batch B;
        const uint32_t lens[] = {103, 104, 105, 64, 104};
        for (int k = 0; k < 40; k++) B.add(1, lens[k % 5] - 18, rnd() % 16);
        B.finish();
        for (size_t i = 0; i < 40; i++) {
            const uint8_t* p = B.pkt(i);
            B.want.emplace_back(p, p + 14);
            B.want[i].insert(B.want[i].end(), p + 18, p + B.lens[i]);
            B.want_status.push_back(B.want[i].size() > 100 || i == 39 ? PKT_EDIT_NO_ROOM : PKT_EDIT_OK);
        }
        run(B, {op(PKT_EDIT_REMOVE_HDR, PKT_HDR_VLAN, 0)}, {}, {}, 100, 100 * 40 - 1, nullptr, true);  // 39: room 99 for 100 bytes
        std::vector<uint64_t> offs(40);
        for (size_t i = 0; i < 40; i++) offs[i] = 128 * i + i % 16;
        const uint64_t dst_len = offs[39] + 100;  // exactly 39's 100 bytes
        offs[5] = dst_len, offs[20] = dst_len + 1000, offs[33] = 1ull << 40;
        for (size_t i = 0; i < 40; i++)
            B.want_status[i] = B.want[i].size() > 100 || i == 5 || i == 20 || i == 33 ? PKT_EDIT_NO_ROOM : PKT_EDIT_OK;
        run(B, {op(PKT_EDIT_REMOVE_HDR, PKT_HDR_VLAN, 0)}, {}, offs, 100, dst_len, nullptr, true);
        // a selection: the unselected packets are copied whole (and 105 bytes do not fit)
        std::vector<uint8_t> sel(40);
        for (size_t i = 0; i < 40; i++) {
            sel[i] = (uint8_t)(rnd() & 1);
            if (!sel[i]) B.want[i].assign(B.pkt(i), B.pkt(i) + B.lens[i]);
            B.want_status[i] = B.want[i].size() > 100 ? PKT_EDIT_NO_ROOM : PKT_EDIT_OK;
        }
        run(B, {op(PKT_EDIT_REMOVE_HDR, PKT_HDR_VLAN, 0)}, {}, {}, 100, 4000, sel.data(), true);
    }
    // (3) depth: Ether and 15 tags; one insert is DEPTH, remove then insert OK, insert then remove DEPTH
    {
        Batch B;
        B.add(15, 30, 3);
        B.add(2, 30, 9);
        B.finish();
        for (int variant = 0; variant < 3; variant++) {
            B.want.clear(), B.want_status.clear();
            for (size_t i = 0; i < 2; i++) {
                const uint8_t* p = B.pkt(i);
                std::vector<uint8_t> w(p, p + 14);
                if (variant) {  // the first tag removed, the constant in its place (insert at 1 either way)
                    w.insert(w.end(), kMpls.begin(), kMpls.end());
                    w.insert(w.end(), p + 18, p + B.lens[i]);
                } else {
                    w.insert(w.end(), kMpls.begin(), kMpls.end());
                    w.insert(w.end(), p + 14, p + B.lens[i]);
                }
                B.want.push_back(w);
                B.want_status.push_back(i == 0 && variant != 1 ? PKT_EDIT_DEPTH : PKT_EDIT_OK);
            }
            std::vector<pkt_edit_op_t> ops;
            if (variant == 1) ops.push_back(op(PKT_EDIT_REMOVE_AT, 0, 1));
            ops.push_back(op(PKT_EDIT_INSERT, PKT_HDR_MPLS, 1));
            if (variant == 2) ops.push_back(op(PKT_EDIT_REMOVE_AT, 0, 2));
            run(B, ops, kMpls, {}, 256, 512, nullptr, true);
        }
        // eight ops, pushes and pops on lists that run empty
        std::vector<pkt_edit_op_t> ops = {op(PKT_EDIT_POP, 0, 0), op(PKT_EDIT_POP, 0, 0), op(PKT_EDIT_POP, 0, 0), op(PKT_EDIT_POP, 0, 0),
                                          op(PKT_EDIT_INSERT, PKT_HDR_MPLS, PKT_EDIT_END), op(PKT_EDIT_INSERT, PKT_HDR_MPLS, 200),
                                          op(PKT_EDIT_REMOVE_HDR, PKT_HDR_MPLS, 1), op(PKT_EDIT_REMOVE_AT, 0, 77)};
        run(B, ops, kMpls, {}, 256, 512, nullptr, false);
    }
    // (4) chain columns that are no parse of the batch
    {
        Batch B;
        for (int k = 0; k < 600; k++) B.add(rnd() % 3, rnd() % 40, rnd() % 16);
        B.lens[7] = 0xFFFFFFFFu, B.offs[9] = 1ull << 40, B.lens[11] = 0;
        B.finish();
        static const uint16_t kOffs[] = {0, 3, 14, 30, 39, 40, 41, 1000, 65535};
        for (size_t i = 0; i < 600; i++) {
            B.status[i] = (uint8_t)(rnd() % 10 == 0 ? rnd() % 4 : 0);
            B.n_hdrs[i] = (uint8_t)(rnd() % 40);
            B.payload_off[i] = kOffs[rnd() % 9], B.payload_len[i] = kOffs[rnd() % 9];
            for (uint32_t j = 0; j < PKT_MAX_HDRS; j++) {
                B.hdr_type[j * 600 + i] = (uint8_t)(rnd() % 3 ? rnd() % 22 : rnd());
                B.hdr_off[j * 600 + i] = kOffs[rnd() % 9];
            }
        }
        std::vector<uint8_t> data(320);
        for (auto& x : data) x = (uint8_t)rnd();
        std::vector<pkt_edit_op_t> ops = {op(PKT_EDIT_REMOVE_AT, 0, 1), op(PKT_EDIT_INSERT, PKT_HDR_IPV6, 2, 280),
                                          op(PKT_EDIT_REMOVE_HDR, 200, 0), op(PKT_EDIT_INSERT, PKT_HDR_STP, PKT_EDIT_END, 285)};
        run(B, ops, data, {}, 300, 300 * 600 - 17, nullptr, false);
        run(B, {}, {}, {}, 33, 33 * 600, nullptr, false);
    }
    // argument errors, and n == 0
    {
        Batch B;
        B.add(1, 20, 0);
        B.finish();
        pkt_batch_t b{};
        b.slab = B.bytes.data(), b.slab_len = B.bytes.size(), b.offsets = B.offs.data(), b.lens = B.lens.data(), b.n = 1;
        pkt_out_t parsed{};
        parsed.status = B.status.data(), parsed.n_hdrs = B.n_hdrs.data(), parsed.hdr_type = B.hdr_type.data();
        parsed.hdr_off = B.hdr_off.data(), parsed.payload_off = B.payload_off.data(), parsed.payload_len = B.payload_len.data();
        uint8_t dst[64];
        const pkt_edit_op_t nine[9] = {}, ins = op(PKT_EDIT_INSERT, PKT_HDR_MPLS, 0, 1), kind = op(4, 0, 0), type = op(PKT_EDIT_INSERT, 22, 0);
        pkt_out_t no_off = parsed;
        no_off.hdr_off = nullptr;
        pkt_batch_t huge = b;
        huge.n = 1ull << 32;
        if (pkt_edit_host(&b, &parsed, nine, 9, nullptr, 0, nullptr, dst, 64, nullptr, 64, nullptr, nullptr, nullptr) != PKT_ERR_INVALID_ARG ||
            pkt_edit_host(&b, &parsed, &kind, 1, nullptr, 0, nullptr, dst, 64, nullptr, 64, nullptr, nullptr, nullptr) != PKT_ERR_INVALID_ARG ||
            pkt_edit_host(&b, &parsed, &type, 1, kMpls.data(), 4, nullptr, dst, 64, nullptr, 64, nullptr, nullptr, nullptr) != PKT_ERR_INVALID_ARG ||
            pkt_edit_host(&b, &parsed, &ins, 1, kMpls.data(), 4, nullptr, dst, 64, nullptr, 64, nullptr, nullptr, nullptr) != PKT_ERR_INVALID_ARG ||
            pkt_edit_host(&b, &parsed, nullptr, 0, nullptr, 0, nullptr, dst, 64, nullptr, 0, nullptr, nullptr, nullptr) != PKT_ERR_INVALID_ARG ||
            pkt_edit_host(&b, &parsed, nullptr, 0, nullptr, 0, nullptr, nullptr, 64, nullptr, 64, nullptr, nullptr, nullptr) != PKT_ERR_INVALID_ARG ||
            pkt_edit_host(&b, &no_off, nullptr, 0, nullptr, 0, nullptr, dst, 64, nullptr, 64, nullptr, nullptr, nullptr) != PKT_ERR_INVALID_ARG ||
            pkt_edit_host(&huge, &parsed, nullptr, 0, nullptr, 0, nullptr, dst, 64, nullptr, 64, nullptr, nullptr, nullptr) != PKT_ERR_INVALID_ARG)
            die("argument errors", 0);
        pkt_batch_t e{};
        pkt_out_t none{};
        if (pkt_edit_host(&e, &none, nullptr, 0, nullptr, 0, nullptr, nullptr, 0, nullptr, 64, nullptr, nullptr, nullptr) != PKT_SUCCESS)
            die("empty batch", 0);
    }
    std::printf("edit OK\n");
    return 0;
}
