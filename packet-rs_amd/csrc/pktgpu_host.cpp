// pktgpu_host.cpp — host-side part of the C ABI: metadata tables, the pcap indexer and the
// host checksum.  No device code.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/pktgpu.h"
#include "pktgpu_batch.hpp"
#include "pktgpu_flow.hpp"
#include "pktgpu_match.hpp"
#include "pktgpu_dispatch.hpp"
#include "pktgpu_lpm.hpp"
#include "pktgpu_fwd.hpp"
#include "pktgpu_frag.hpp"
#include "pktgpu_reasm.hpp"
#include "pktgpu_scan.hpp"
#include "pktgpu_icmp.hpp"
#include "pktgpu_tunnel.hpp"
#include "pktgpu_nat.hpp"
#include "pktgpu_meter.hpp"

namespace {

struct FieldDef {
    const char* name;
    uint16_t start, end;
};
struct HdrDef {
    const char* name;
    int size;
    int nfields;
    FieldDef f[16];
};

// make_header! invocations of the reference (src/headers.rs:529-827).
constexpr HdrDef kHdrs[PKT_HDR_COUNT] = {
    {"", 0, 0, {}},
    {"Ether", 14, 3, {{"dst", 0, 47}, {"src", 48, 95}, {"etype", 96, 111}}},
    {"Vlan", 4, 4, {{"pcp", 0, 2}, {"cfi", 3, 3}, {"vid", 4, 15}, {"etype", 16, 31}}},
    {"IPv4", 20, 12,
     {{"version", 0, 3}, {"ihl", 4, 7}, {"diffserv", 8, 15}, {"total_len", 16, 31},
      {"identification", 32, 47}, {"flags", 48, 50}, {"frag_startset", 51, 63}, {"ttl", 64, 71},
      {"protocol", 72, 79}, {"header_checksum", 80, 95}, {"src", 96, 127}, {"dst", 128, 159}}},
    {"IPv6", 40, 8,
     {{"version", 0, 3}, {"traffic_class", 4, 11}, {"flow_label", 12, 31}, {"payload_len", 32, 47},
      {"next_hdr", 48, 55}, {"hop_limit", 56, 63}, {"src", 64, 191}, {"dst", 192, 319}}},
    {"ICMP", 4, 3, {{"icmp_type", 0, 7}, {"icmp_code", 8, 15}, {"chksum", 16, 31}}},
    {"TCP", 20, 10,
     {{"src", 0, 15}, {"dst", 16, 31}, {"seq_no", 32, 63}, {"ack_no", 64, 95},
      {"data_startset", 96, 99}, {"res", 100, 103}, {"flags", 104, 111}, {"window", 112, 127},
      {"checksum", 128, 143}, {"urgent_ptr", 144, 159}}},
    {"UDP", 8, 4, {{"src", 0, 15}, {"dst", 16, 31}, {"length", 32, 47}, {"checksum", 48, 63}}},
    {"ARP", 28, 9,
     {{"hwtype", 0, 15}, {"proto_type", 16, 31}, {"hwlen", 32, 39}, {"proto_len", 40, 47},
      {"opcode", 48, 63}, {"sender_hw_addr", 64, 111}, {"sender_proto_addr", 112, 143},
      {"target_hw_addr", 144, 191}, {"target_proto_addr", 192, 223}}},
    {"Vxlan", 8, 4, {{"flags", 0, 7}, {"reserved", 8, 31}, {"vni", 32, 55}, {"reserved2", 56, 63}}},
    {"Dot3", 14, 3, {{"dst", 0, 47}, {"src", 48, 95}, {"length", 96, 111}}},
    {"LLC", 3, 3, {{"dsap", 0, 7}, {"ssap", 8, 15}, {"ctrl", 16, 23}}},
    {"SNAP", 5, 2, {{"oui", 0, 23}, {"code", 24, 39}}},
    {"GRE", 4, 9,
     {{"chksum_present", 0, 0}, {"routing_present", 1, 1}, {"key_present", 2, 2},
      {"seqnum_present", 3, 3}, {"strict_route_src", 4, 4}, {"recurse", 5, 7}, {"flags", 8, 12},
      {"version", 13, 15}, {"proto", 16, 31}}},
    {"GREChksumOffset", 4, 2, {{"chksum", 0, 15}, {"offset", 16, 31}}},
    {"GRESequenceNum", 4, 1, {{"seqnum", 0, 31}}},
    {"GREKey", 4, 1, {{"key", 0, 31}}},
    {"ERSPAN2", 8, 8,
     {{"version", 0, 3}, {"vlan", 4, 15}, {"cos", 16, 18}, {"en", 19, 20}, {"t", 21, 21},
      {"session_id", 22, 31}, {"reserved", 32, 43}, {"index", 44, 63}}},
    {"ERSPAN3", 12, 14,
     {{"version", 0, 3}, {"vlan", 4, 15}, {"cos", 16, 18}, {"bos", 19, 20}, {"t", 21, 21},
      {"session_id", 22, 31}, {"timestamp", 32, 63}, {"sgt", 64, 79}, {"p", 80, 80}, {"ft", 81, 85},
      {"hw_id", 86, 91}, {"d", 92, 92}, {"gra", 93, 94}, {"o", 95, 95}}},
    {"ERSPANPLATFORM", 8, 2, {{"id", 0, 5}, {"info", 6, 63}}},
    {"STP", 35, 14,
     {{"proto", 0, 15}, {"version", 16, 23}, {"bpdu_type", 24, 31}, {"flags", 32, 39},
      {"root_id", 40, 55}, {"root_mac", 56, 103}, {"root_path_cost", 104, 135},
      {"bridge_id", 136, 151}, {"bridge_mac", 152, 199}, {"port_id", 200, 215},
      {"message_age", 216, 231}, {"max_age", 232, 247}, {"hello_time", 248, 263},
      {"fwd_delay", 264, 279}}},
    {"MPLS", 4, 4, {{"label", 0, 19}, {"exp", 20, 22}, {"bos", 23, 23}, {"ttl", 24, 31}}},
};

constexpr bool sizes_agree() {
    for (int t = 0; t < PKT_HDR_COUNT; t++)
        if (kHdrs[t].size != kHdrSizes[t]) return false;
    return true;
}
static_assert(sizes_agree(), "kHdrs[].size and PKT_HDR_SIZE_LIST (pktgpu_batch.hpp) differ");

// a host model's refusal of a batch with n > 0: the device entry points' rules, less the slab's alignment
bool bad_batch(const pkt_batch_t* b) { return batch_null_slab(b) || batch_index_error(b); }

const char* kEntryNames[PKT_ENTRY_COUNT] = {
    "parse", "parse_dot3", "parse_llc", "parse_snap", "parse_ethernet", "parse_vlan",
    "parse_mpls", "parse_mpls_bos", "parse_ipv4", "parse_ipv6", "parse_gre", "parse_erspan2",
    "parse_erspan3", "parse_arp", "parse_icmp", "parse_tcp", "parse_udp", "parse_vxlan"};

const char* kStatusNames[3] = {"OK", "TRUNCATED", "DEPTH_LIMIT"};

inline uint32_t rd_le32(const uint8_t* p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

}  // namespace

extern "C" {

int pkt_abi_version(void) { return PKTGPU_ABI_VERSION; }
size_t pkt_sizeof_batch(void) { return sizeof(pkt_batch_t); }
size_t pkt_sizeof_out(void) { return sizeof(pkt_out_t); }
size_t pkt_sizeof_field_spec(void) { return sizeof(pkt_field_spec_t); }
size_t pkt_sizeof_cmp_summary(void) { return sizeof(pkt_cmp_summary_t); }
size_t pkt_sizeof_edit_op(void) { return sizeof(pkt_edit_op_t); }

const char* pkt_hdr_name(int t) { return (t > 0 && t < PKT_HDR_COUNT) ? kHdrs[t].name : nullptr; }
int pkt_hdr_size(int t) { return (t > 0 && t < PKT_HDR_COUNT) ? kHdrs[t].size : 0; }
int pkt_hdr_field_count(int t) { return (t > 0 && t < PKT_HDR_COUNT) ? kHdrs[t].nfields : 0; }

int pkt_hdr_field(int t, int idx, const char** name, uint16_t* start, uint16_t* end) {
    if (t <= 0 || t >= PKT_HDR_COUNT || idx < 0 || idx >= kHdrs[t].nfields) return PKT_ERR_INVALID_ARG;
    if (name) *name = kHdrs[t].f[idx].name;
    if (start) *start = kHdrs[t].f[idx].start;
    if (end) *end = kHdrs[t].f[idx].end;
    return PKT_SUCCESS;
}

const char* pkt_status_name(int s) { return (s >= 0 && s < 3) ? kStatusNames[s] : nullptr; }
const char* pkt_entry_name(int e) { return (e >= 0 && e < PKT_ENTRY_COUNT) ? kEntryNames[e] : nullptr; }

// tests/pcap.rs:7-37: 24-byte global header (LE magic d4 c3 b2 a1), then per record a 16-byte
// header {ts_sec, ts_usec, incl_len, orig_len} followed by incl_len bytes.
int pkt_pcap_index(const uint8_t* buf, uint64_t len, uint64_t* offsets, uint32_t* lens, uint64_t cap,
                   uint64_t* n_out) {
    if (!buf || !n_out || (cap && (!offsets || !lens))) return PKT_ERR_INVALID_ARG;
    *n_out = 0;
    if (len < 24 || buf[0] != 0xD4 || buf[1] != 0xC3 || buf[2] != 0xB2 || buf[3] != 0xA1)
        return PKT_ERR_INVALID_ARG;
    uint64_t off = 24, n = 0;
    while (off + 16 <= len) {
        uint32_t incl = rd_le32(buf + off + 8);
        if (off + 16 + (uint64_t)incl > len) return PKT_ERR_INVALID_ARG;
        if (n < cap) {
            offsets[n] = off + 16;
            lens[n] = incl;
        }
        n++;
        off += 16 + (uint64_t)incl;
    }
    *n_out = n;
    return PKT_SUCCESS;
}

// pkt_pcap_write on host pointers (the CPU model of pktgpu_pcapw.hip): tests/pcap.rs:7-37 over the
// selected packets of the batch, in batch order.  Two passes: the totals, then the bytes.
int pkt_pcap_write_host(const pkt_batch_t* b, const uint8_t* select, uint32_t snaplen, uint32_t tv_sec,
                        uint32_t tv_usec, const uint32_t* ts_sec, const uint32_t* ts_usec, uint8_t* dst, uint64_t dst_len,
                        uint64_t* rec_offsets, uint32_t* rec_lens, uint32_t* src_index, uint64_t* bytes_out,
                        uint64_t* n_out) {
    static const uint8_t kGlobal[24] = {0xD4, 0xC3, 0xB2, 0xA1, 0x2, 0x0, 0x4, 0x0, 0, 0, 0, 0,
                                        0,    0,    0,    0,    0xFF, 0xFF, 0, 0, 1, 0, 0, 0};
    if (bytes_out) *bytes_out = 0;
    if (n_out) *n_out = 0;
    if (!b || b->n >= (1ull << 32) || (dst_len && !dst)) return PKT_ERR_INVALID_ARG;
    if (b->n && bad_batch(b)) return PKT_ERR_INVALID_ARG;
    const BatchSrc src = batch_src(b);
    auto pkt = [&](uint64_t i, uint64_t& off, uint32_t& len, uint32_t& incl) {
        off = pkt_off(src, i);
        len = pkt_len(src, i, off);
        incl = snaplen && len > snaplen ? snaplen : len;
    };
    uint64_t total = 24, cnt = 0;
    for (uint64_t i = 0; i < b->n; i++) {
        if (select && !select[i]) continue;
        uint64_t off;
        uint32_t len, incl;
        pkt(i, off, len, incl);
        total += 16 + (uint64_t)incl;
        cnt++;
    }
    if (bytes_out) *bytes_out = total;
    if (n_out) *n_out = cnt;
    if (total > dst_len) return PKT_ERR_INVALID_ARG;  // the size to retry with is in *bytes_out
    memcpy(dst, kGlobal, 24);
    uint64_t pos = 24, k = 0;
    for (uint64_t i = 0; i < b->n; i++) {
        if (select && !select[i]) continue;
        uint64_t off;
        uint32_t len, incl;
        pkt(i, off, len, incl);
        const uint32_t hdr[4] = {ts_sec ? ts_sec[i] : tv_sec, ts_usec ? ts_usec[i] : tv_usec, incl, len};
        for (int j = 0; j < 4; j++)
            for (int x = 0; x < 4; x++) dst[pos + 4 * j + x] = (uint8_t)(hdr[j] >> (8 * x));
        if (incl) memcpy(dst + pos + 16, b->slab + off, incl);
        if (rec_offsets) rec_offsets[k] = pos + 16;
        if (rec_lens) rec_lens[k] = incl;
        if (src_index) src_index[k] = (uint32_t)i;
        pos += 16 + (uint64_t)incl;
        k++;
    }
    return PKT_SUCCESS;
}

// pkt_compare_batch on host pointers (the CPU model of pktgpu_compare.hip): Packet::compare
// (packet.rs:326-358) of packet i of `a` against packet i of `b`, byte by byte.
int pkt_compare_host(const pkt_batch_t* a, const pkt_batch_t* b, const pkt_chain_t* chain, const pkt_field_spec_t* ignore,
                     uint32_t nignore, uint8_t* result, uint32_t* matching, uint32_t* first_diff,
                     pkt_cmp_summary_t* summary) {
    if (summary) *summary = pkt_cmp_summary_t{0, 0, 0, 0};
    if (!a || !b || a->n != b->n || a->n >= (1ull << 32) || nignore > 16) return PKT_ERR_INVALID_ARG;
    if (nignore && (!ignore || !chain || !chain->n_hdrs || !chain->hdr_type || !chain->hdr_off)) return PKT_ERR_INVALID_ARG;
    for (uint32_t k = 0; k < nignore; k++)
        if (ignore[k].end < ignore[k].start) return PKT_ERR_INVALID_ARG;
    const uint64_t n = a->n;
    if (n && (bad_batch(a) || bad_batch(b))) return PKT_ERR_INVALID_ARG;
    const BatchSrc sa = batch_src(a), sb = batch_src(b);
    auto pkt = [](const BatchSrc& s, uint64_t i, uint32_t& len) -> const uint8_t* {
        const uint64_t off = pkt_off(s, i);
        len = pkt_len(s, i, off);
        return len ? s.slab + off : nullptr;
    };
    pkt_cmp_summary_t sum{0, 0, 0, n};
    for (uint64_t i = 0; i < n; i++) {
        uint32_t la, lb;
        const uint8_t* pa = pkt(sa, i, la);
        const uint8_t* pb = pkt(sb, i, lb);
        const uint32_t m = la < lb ? la : lb;
        // the specs' bit ranges in packet i, first > last where its chain lacks the header
        uint32_t lo[16], hi[16];
        for (uint32_t k = 0; k < nignore; k++) {
            lo[k] = 1, hi[k] = 0;
            uint32_t nh = chain->n_hdrs[i], seen = 0;
            nh = nh > PKT_MAX_HDRS ? PKT_MAX_HDRS : nh;
            for (uint32_t j = 0; j < nh; j++) {
                if (chain->hdr_type[j * n + i] != ignore[k].hdr_type) continue;
                if (seen++ == ignore[k].occurrence) {
                    lo[k] = 8u * chain->hdr_off[j * n + i] + ignore[k].start;
                    hi[k] = 8u * chain->hdr_off[j * n + i] + ignore[k].end;
                    break;
                }
            }
        }
        uint32_t cnt = 0, fd = m;
        for (uint32_t j = 0; j < m; j++) {
            uint8_t d = pa[j] ^ pb[j];
            for (uint32_t k = 0; d && k < nignore; k++) {
                if (lo[k] > hi[k] || hi[k] < 8u * j || lo[k] > 8u * j + 7u) continue;
                const uint32_t l = lo[k] > 8u * j ? lo[k] - 8u * j : 0u, h = hi[k] < 8u * j + 7u ? hi[k] - 8u * j : 7u;
                d &= (uint8_t)~((0xFFu >> l) & (0xFFu << (7u - h)));  // bit t of the byte, MSB-first
            }
            if (!d)
                cnt++;
            else if (fd == m)
                fd = j;
        }
        const uint8_t r = la != lb ? PKT_CMP_LEN : cnt != la ? PKT_CMP_BYTES : PKT_CMP_EQUAL;
        if (result) result[i] = r;
        if (matching) matching[i] = cnt;
        if (first_diff) first_diff[i] = fd;
        (r == PKT_CMP_EQUAL ? sum.n_equal : r == PKT_CMP_LEN ? sum.n_len : sum.n_bytes)++;
        if (r != PKT_CMP_EQUAL && sum.first_bad == n) sum.first_bad = i;
    }
    if (summary) *summary = sum;
    return PKT_SUCCESS;
}

// pkt_edit_batch on host pointers (the CPU model of pktgpu_edit.hip): Packet::push / insert / pop /
// remove (packet.rs:117-164) on every packet's header list, then to_vec (385-392), packet by packet.
int pkt_edit_host(const pkt_batch_t* b, const pkt_out_t* parsed, const pkt_edit_op_t* ops, uint32_t nops,
                  const uint8_t* hdr_data, uint32_t hdr_data_len, const uint8_t* select, uint8_t* dst, uint64_t dst_len,
                  const uint64_t* dst_offsets, uint32_t slot, uint32_t* out_len, uint8_t* edit_status,
                  const pkt_out_t* out_chain) {
    if (!b || !parsed || nops > 8 || (nops && !ops) || hdr_data_len > 320 || slot == 0 || b->n >= (1ull << 32))
        return PKT_ERR_INVALID_ARG;
    for (uint32_t k = 0; k < nops; k++) {
        if (ops[k].kind > PKT_EDIT_INSERT) return PKT_ERR_INVALID_ARG;
        if (ops[k].kind != PKT_EDIT_INSERT) continue;
        if (ops[k].hdr_type == 0 || ops[k].hdr_type >= PKT_HDR_COUNT || !hdr_data ||
            (uint64_t)ops[k].data_off + kHdrs[ops[k].hdr_type].size > hdr_data_len)
            return PKT_ERR_INVALID_ARG;
    }
    const uint64_t n = b->n;
    if (n == 0) return PKT_SUCCESS;
    if (!dst || !parsed->status || !parsed->n_hdrs || !parsed->hdr_type || !parsed->hdr_off || !parsed->payload_off ||
        !parsed->payload_len)
        return PKT_ERR_INVALID_ARG;
    if (bad_batch(b)) return PKT_ERR_INVALID_ARG;
    const BatchSrc src = batch_src(b);
    struct Ent {
        uint8_t type, konst;  // konst: the bytes are hdr_data[at ..], else the packet's [at ..]
        uint32_t at, size;
    };
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t off = pkt_off(src, i);
        const uint32_t len = pkt_len(src, i, off);
        const uint64_t o = dst_offsets ? dst_offsets[i] : i * slot;
        const uint64_t room = o >= dst_len ? 0 : (dst_len - o < slot ? dst_len - o : slot);
        // a slice of the packet, clamped to [0, len)
        auto clamp = [len](uint32_t at, uint32_t size, uint32_t& a, uint32_t& s) {
            a = at > len ? len : at;
            s = size > len - a ? len - a : size;
        };
        Ent L[PKT_MAX_HDRS + 1];
        uint32_t cnt = 0, st = parsed->status[i] == PKT_OK ? PKT_EDIT_OK : PKT_EDIT_SKIPPED;
        uint32_t pay_at = 0, pay_len = 0;
        if (st == PKT_EDIT_OK) {
            uint32_t nh = parsed->n_hdrs[i];
            nh = nh > PKT_MAX_HDRS ? PKT_MAX_HDRS : nh;
            for (uint32_t j = 0; j < nh; j++) {
                Ent& e = L[cnt++];
                e.type = parsed->hdr_type[j * n + i];
                e.konst = 0;
                clamp(parsed->hdr_off[j * n + i], e.type < PKT_HDR_COUNT ? kHdrs[e.type].size : 0, e.at, e.size);
            }
            clamp(parsed->payload_off[i], parsed->payload_len[i], pay_at, pay_len);
            const uint32_t run = select && !select[i] ? 0 : nops;
            for (uint32_t k = 0; k < run && st == PKT_EDIT_OK; k++) {
                const pkt_edit_op_t& op = ops[k];
                uint32_t at = cnt;  // the entry to remove, cnt = none
                if (op.kind == PKT_EDIT_POP) {
                    at = cnt ? cnt - 1 : cnt;
                } else if (op.kind == PKT_EDIT_REMOVE_AT) {
                    at = op.index < cnt ? op.index : cnt;
                } else if (op.kind == PKT_EDIT_REMOVE_HDR) {
                    uint32_t seen = 0;
                    for (uint32_t j = 0; j < cnt && at == cnt; j++)
                        if (L[j].type == op.hdr_type && seen++ == op.index) at = j;
                } else {
                    const uint32_t pos = op.index == PKT_EDIT_END || op.index > cnt ? cnt : op.index;
                    for (uint32_t j = cnt; j > pos; j--) L[j] = L[j - 1];
                    L[pos] = Ent{op.hdr_type, 1, op.data_off, (uint32_t)kHdrs[op.hdr_type].size};
                    if (++cnt > PKT_MAX_HDRS) st = PKT_EDIT_DEPTH;
                    continue;
                }
                if (at < cnt) {
                    for (uint32_t j = at; j + 1 < cnt; j++) L[j] = L[j + 1];
                    cnt--;
                }
            }
        }
        uint32_t total = pay_len;
        for (uint32_t j = 0; j < cnt; j++) total += L[j].size;
        if (st == PKT_EDIT_OK && (total > room || total > 65535)) st = PKT_EDIT_NO_ROOM;
        if (st != PKT_EDIT_OK) cnt = total = pay_len = 0;
        uint32_t pos = 0, mask = 0;
        for (uint32_t j = 0; j < cnt; j++) {
            if (L[j].size) memcpy(dst + o + pos, (L[j].konst ? hdr_data : b->slab + off) + L[j].at, L[j].size);
            if (out_chain && out_chain->hdr_type) out_chain->hdr_type[j * n + i] = L[j].type;
            if (out_chain && out_chain->hdr_off) out_chain->hdr_off[j * n + i] = (uint16_t)pos;
            mask |= L[j].type < 32 ? 1u << L[j].type : 0u;
            pos += L[j].size;
        }
        if (pay_len) memcpy(dst + o + pos, b->slab + off + pay_at, pay_len);
        if (out_len) out_len[i] = total;
        if (edit_status) edit_status[i] = (uint8_t)st;
        if (out_chain) {
            const uint8_t cs = st == PKT_EDIT_OK ? PKT_OK : st == PKT_EDIT_SKIPPED ? parsed->status[i]
                             : st == PKT_EDIT_DEPTH ? PKT_DEPTH_LIMIT : PKT_TRUNCATED;
            if (out_chain->status) out_chain->status[i] = cs;
            if (out_chain->n_hdrs) out_chain->n_hdrs[i] = (uint8_t)cnt;
            if (out_chain->payload_off) out_chain->payload_off[i] = (uint16_t)pos;
            if (out_chain->payload_len) out_chain->payload_len[i] = (uint16_t)pay_len;
            if (out_chain->hdr_mask) out_chain->hdr_mask[i] = mask;
        }
    }
    return PKT_SUCCESS;
}

// pkt_l4_checksum_batch on host pointers (the CPU model of pktgpu_l4csum.hip): the RFC 1071 checksum of
// every packet's TCP / UDP / ICMP segment with its pseudo-header, word by word.
int pkt_l4_checksum_host(const pkt_batch_t* b, const pkt_chain_t* chain, uint32_t which, uint32_t flags, uint16_t* calc,
                         uint16_t* stored, uint8_t* l4_status) {
    if (!b || !chain) return PKT_ERR_INVALID_ARG;
    if (b->n >= (1ull << 32) || (flags & ~(PKT_L4_UPDATE | PKT_L4_KEEP_ZERO_UDP))) return PKT_ERR_INVALID_ARG;
    if ((flags & PKT_L4_KEEP_ZERO_UDP) && !(flags & PKT_L4_UPDATE)) return PKT_ERR_INVALID_ARG;
    if (which >= PKT_MAX_HDRS && which != PKT_L4_LAST) return PKT_ERR_INVALID_ARG;
    const uint64_t n = b->n;
    if (n == 0) return PKT_SUCCESS;
    if (bad_batch(b) || !chain->n_hdrs || !chain->hdr_type || !chain->hdr_off) return PKT_ERR_INVALID_ARG;
    const BatchSrc src = batch_src(b);
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t off = pkt_off(src, i);
        const uint32_t len = pkt_len(src, i, off);
        uint32_t nh = chain->n_hdrs[i], seen = 0, slot = PKT_MAX_HDRS;
        nh = nh > PKT_MAX_HDRS ? PKT_MAX_HDRS : nh;
        for (uint32_t j = 0; j < nh; j++) {
            const uint8_t t = chain->hdr_type[j * n + i];
            if (t != PKT_HDR_TCP && t != PKT_HDR_UDP && t != PKT_HDR_ICMP) continue;
            if (which == PKT_L4_LAST || seen == which) slot = j;
            seen++;
        }
        uint32_t st = PKT_L4_ABSENT, c = 0, sv = 0, field = 0;
        if (slot < PKT_MAX_HDRS) {
            const uint8_t t = chain->hdr_type[slot * n + i], ipt = slot ? chain->hdr_type[(slot - 1) * n + i] : 0;
            const uint32_t s = chain->hdr_off[slot * n + i], ip = slot ? chain->hdr_off[(slot - 1) * n + i] : 0u;
            const bool v4 = ipt == PKT_HDR_IPV4;
            const uint8_t* p = b->slab + off;
            if (!v4 && ipt != PKT_HDR_IPV6) {
                st = PKT_L4_NO_IP;
            } else if (ip + (v4 ? 20u : 40u) > len) {
                st = PKT_L4_SPAN;
            } else if (v4 && ((((uint32_t)p[ip + 6] << 8) | p[ip + 7]) & 0x3FFFu)) {
                st = PKT_L4_FRAGMENT;
            } else {
                const uint32_t e = v4 ? ip + (((uint32_t)p[ip + 2] << 8) | p[ip + 3])
                                      : ip + 40u + (((uint32_t)p[ip + 4] << 8) | p[ip + 5]);
                if (e > len || e < s + kHdrs[t].size) {
                    st = PKT_L4_SPAN;
                } else {
                    const uint32_t seg = e - s;
                    field = s + (t == PKT_HDR_TCP ? 16u : t == PKT_HDR_UDP ? 6u : 2u);
                    const uint32_t proto = t == PKT_HDR_TCP ? 6u : t == PKT_HDR_UDP ? 17u : 58u;
                    uint64_t sum = 0;
                    if (v4 && t != PKT_HDR_ICMP) {
                        for (uint32_t k = 12; k < 20; k += 2) sum += ((uint32_t)p[ip + k] << 8) | p[ip + k + 1];
                        sum += proto + seg;
                    } else if (!v4) {
                        for (uint32_t k = 8; k < 40; k += 2) sum += ((uint32_t)p[ip + k] << 8) | p[ip + k + 1];
                        sum += proto + seg;  // seg < 2^16: the length's upper word is 0
                    }
                    for (uint32_t k = s; k < e; k += 2) {
                        if (k == field) continue;
                        sum += ((uint32_t)p[k] << 8) | (k + 1 < e ? p[k + 1] : 0u);
                    }
                    while (sum >> 16) sum = (sum & 0xFFFFu) + (sum >> 16);
                    c = (uint32_t)~sum & 0xFFFFu;
                    if (t == PKT_HDR_UDP && c == 0) c = 0xFFFFu;
                    sv = ((uint32_t)p[field] << 8) | p[field + 1];
                    if (t == PKT_HDR_UDP && sv == 0)
                        st = v4 ? PKT_L4_UNCHECKED : PKT_L4_BAD;
                    else
                        st = sv == c || (sv == 0xFFFFu && c == 0) ? PKT_L4_OK : PKT_L4_BAD;
                    if ((flags & PKT_L4_UPDATE) && !(st == PKT_L4_UNCHECKED && (flags & PKT_L4_KEEP_ZERO_UDP))) {
                        uint8_t* w = const_cast<uint8_t*>(p);
                        w[field] = (uint8_t)(c >> 8);
                        w[field + 1] = (uint8_t)c;
                    }
                }
            }
        }
        if (calc) calc[i] = (uint16_t)c;
        if (stored) stored[i] = (uint16_t)sv;
        if (l4_status) l4_status[i] = (uint8_t)st;
    }
    return PKT_SUCCESS;
}

// pkt_flow_key_batch on host pointers (the CPU model of pktgpu_flow.hip's key kernel), byte by byte.
int pkt_flow_key_host(const pkt_batch_t* b, const pkt_chain_t* chain, uint32_t which_ip, uint32_t flags, uint64_t seed,
                      const uint8_t rss_key[40], pkt_flow_key_t* keys, uint64_t* hash, uint32_t* rss, uint8_t* dir,
                      uint32_t* plen, uint8_t* status) {
    if (!b || !chain) return PKT_ERR_INVALID_ARG;
    if (b->n >= (1ull << 32) || (flags & ~(PKT_FLOW_SYMMETRIC | PKT_FLOW_NO_PORTS))) return PKT_ERR_INVALID_ARG;
    if (which_ip >= PKT_MAX_HDRS && which_ip != PKT_FLOW_LAST) return PKT_ERR_INVALID_ARG;
    if ((rss && !rss_key) || ((uintptr_t)keys & 1)) return PKT_ERR_INVALID_ARG;
    const uint64_t n = b->n;
    if (n == 0) return PKT_SUCCESS;
    if (bad_batch(b) || !chain->n_hdrs || !chain->hdr_type || !chain->hdr_off) return PKT_ERR_INVALID_ARG;
    const BatchSrc src = batch_src(b);
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t off = pkt_off(src, i);
        const uint32_t len = pkt_len(src, i, off);
        uint32_t nh = chain->n_hdrs[i], seen = 0, slot = PKT_MAX_HDRS;
        nh = nh > PKT_MAX_HDRS ? PKT_MAX_HDRS : nh;
        for (uint32_t j = 0; j < nh; j++) {
            const uint8_t t = chain->hdr_type[j * n + i];
            if (t != PKT_HDR_IPV4 && t != PKT_HDR_IPV6) continue;
            if (which_ip == PKT_FLOW_LAST || seen == which_ip) slot = j;
            seen++;
        }
        uint8_t k[40] = {};  // the key as it lies in memory
        uint32_t st = PKT_FLOW_NO_IP, d = 0, r = 0;
        uint64_t h = 0;
        if (slot < PKT_MAX_HDRS) {
            const bool v4 = chain->hdr_type[slot * n + i] == PKT_HDR_IPV4;
            const uint32_t ip = chain->hdr_off[slot * n + i], alen = v4 ? 4u : 16u;
            const uint8_t* p = b->slab + off;
            st = PKT_FLOW_OK;
            bool ports = false;
            uint32_t l4 = 0;
            if (ip + (v4 ? 20u : 40u) > len) {
                st = PKT_FLOW_SPAN;
            } else {
                const uint8_t nt = slot + 1 < nh ? chain->hdr_type[(slot + 1) * n + i] : 0;
                l4 = slot + 1 < nh ? chain->hdr_off[(slot + 1) * n + i] : 0u;
                ports = (nt == PKT_HDR_TCP || nt == PKT_HDR_UDP) && !(flags & PKT_FLOW_NO_PORTS) &&
                        !(v4 && ((((uint32_t)p[ip + 6] << 8) | p[ip + 7]) & 0x3FFFu));
                if (ports && l4 + 4u > len) st = PKT_FLOW_SPAN;
            }
            if (st == PKT_FLOW_OK) {
                const uint8_t* a = p + ip + (v4 ? 12 : 8);
                uint8_t e0[18] = {}, e1[18] = {};  // src | sport, dst | dport: big-endian byte strings
                memcpy(e0, a, alen);
                memcpy(e1, a + alen, alen);
                if (ports) {
                    memcpy(e0 + 16, p + l4, 2);
                    memcpy(e1 + 16, p + l4 + 2, 2);
                }
                if ((flags & PKT_FLOW_SYMMETRIC) && memcmp(e0, e1, 18) > 0) {
                    uint8_t t[18];
                    memcpy(t, e0, 18);
                    memcpy(e0, e1, 18);
                    memcpy(e1, t, 18);
                    d = 1;
                }
                memcpy(k, e0, 16);
                memcpy(k + 16, e1, 16);
                k[32] = e0[17];  // sport and dport as little-endian values
                k[33] = e0[16];
                k[34] = e1[17];
                k[35] = e1[16];
                k[36] = p[ip + (v4 ? 9 : 6)];
                k[37] = v4 ? 4 : 6;
                uint64_t w[5];
                for (int q = 0; q < 5; q++) {
                    w[q] = 0;
                    for (int z = 7; z >= 0; z--) w[q] = w[q] << 8 | k[8 * q + z];
                }
                h = flow_hash(seed, w);
                if (rss) {
                    uint8_t in[36];
                    uint32_t m = 0;
                    memcpy(in, e0, alen);
                    memcpy(in + alen, e1, alen);
                    m = 2 * alen;
                    if (ports) {
                        memcpy(in + m, e0 + 16, 2);
                        memcpy(in + m + 2, e1 + 16, 2);
                        m += 4;
                    }
                    // bit by bit: the 32 key bits that start at input bit 8 * x + y
                    for (uint32_t x = 0; x < m; x++)
                        for (uint32_t y = 0; y < 8; y++) {
                            if (!(in[x] & (0x80u >> y))) continue;
                            uint32_t win = 0;
                            for (uint32_t z = 0; z < 32; z++) {
                                const uint32_t bit = 8 * x + y + z;
                                const uint32_t kb = bit < 320 ? (rss_key[bit >> 3] >> (7 - (bit & 7))) & 1u : 0u;
                                win = win << 1 | kb;
                            }
                            r ^= win;
                        }
                }
            }
        }
        if (keys) memcpy(reinterpret_cast<uint8_t*>(keys) + 40 * i, k, 40);
        if (hash) hash[i] = h;
        if (rss) rss[i] = r;
        if (dir) dir[i] = (uint8_t)d;
        if (plen) plen[i] = len;
        if (status) status[i] = (uint8_t)st;
    }
    return PKT_SUCCESS;
}

// ---- the flow table: the public calls, and the host table as a sequential loop (the device table: pktgpu_flow.hip)
size_t pkt_sizeof_flow_key(void) { return sizeof(pkt_flow_key_t); }
size_t pkt_sizeof_flow_record(void) { return sizeof(pkt_flow_record_t); }

int pkt_flow_table_create_host(uint64_t slots, pkt_flow_table_t** out) {
    if (!out) return PKT_ERR_INVALID_ARG;
    *out = nullptr;
    if (slots < kFlowMinSlots || slots > kFlowMaxSlots || (slots & (slots - 1))) return PKT_ERR_INVALID_ARG;
    pkt_flow_table* t = new pkt_flow_table;
    t->slots = slots;
    t->e = static_cast<FlowEntry*>(aligned_alloc(alignof(FlowEntry), slots * sizeof(FlowEntry)));
    if (!t->e) {
        delete t;
        return PKT_ERR_UNSUPPORTED;
    }
    *out = t;
    return pkt_flow_table_clear(t, nullptr);
}

int pkt_flow_table_set_tag_bits(pkt_flow_table_t* t, uint32_t bits) {
    if (!t) return PKT_ERR_INVALID_ARG;
    if (bits < 1 || bits > 64) return flow_fail(t, PKT_ERR_INVALID_ARG, "pkt_flow_table_set_tag_bits: bits not in 1..64");
    if (t->touched) return flow_fail(t, PKT_ERR_INVALID_ARG, "pkt_flow_table_set_tag_bits: the table is not empty");
    t->tag_bits = bits;
    return PKT_SUCCESS;
}

int pkt_flow_table_update(pkt_flow_table_t* t, const pkt_flow_key_t* keys, const uint64_t* hash, const uint8_t* dir,
                          const uint32_t* weight, const uint8_t* status, uint64_t n, uint64_t base, uint32_t* flow_id,
                          uint8_t* upd_status, void* stream) {
    if (!t) return PKT_ERR_INVALID_ARG;
    if (n >= (1ull << 32)) return flow_fail(t, PKT_ERR_INVALID_ARG, "pkt_flow_table_update: n >= 2^32");
    if (base < t->hwm || base + n < base)
        return flow_fail(t, PKT_ERR_INVALID_ARG, "pkt_flow_table_update: base below the previous update's base + n");
    if (n && (!keys || !hash)) return flow_fail(t, PKT_ERR_INVALID_ARG, "pkt_flow_table_update: null keys or hash");
    if ((uintptr_t)keys & 7) return flow_fail(t, PKT_ERR_INVALID_ARG, "pkt_flow_table_update: keys not 8-byte aligned");
    const FlowUpdate u{keys, hash, dir, weight, status, n, base, flow_id, upd_status};
    if (n && t->ops) {
        const int rc = t->ops->update(t, u, stream);
        if (rc != PKT_SUCCESS) return rc;
    }
    for (uint64_t i = 0; !t->ops && i < n; i++) {  // the host table
        uint32_t id = kFlowNone, st = PKT_FLOW_UPD_FULL;
        if (status && status[i]) {
            st = PKT_FLOW_UPD_SKIPPED;
        } else {
            uint64_t w[5];
            memcpy(w, reinterpret_cast<const uint8_t*>(keys) + 40 * i, 40);
            const uint64_t tag = flow_tag(hash[i], t->tag_bits);
            uint64_t pos = flow_home(tag, t->slots);
            for (uint64_t probes = 0; probes < t->slots; probes++, pos = (pos + 1) & (t->slots - 1)) {
                FlowEntry& e = t->e[pos];
                if (e.tag == 0) {  // in index order: the first packet to reach an entry is its lowest index
                    e.tag = tag;
                    e.first = base + i;
                    memcpy(e.key, w, 40);
                }
                if (e.tag != tag) continue;
                if (memcmp(e.key, w, 40) != 0) {
                    st = PKT_FLOW_UPD_COLLISION;
                } else {
                    const uint32_t d = dir ? dir[i] & 1u : 0u;
                    e.pkts[d] += 1;
                    e.bytes[d] += weight ? weight[i] : 0u;
                    id = (uint32_t)pos;
                    st = PKT_FLOW_UPD_OK;
                }
                break;
            }
        }
        if (flow_id) flow_id[i] = id;
        if (upd_status) upd_status[i] = (uint8_t)st;
    }
    t->hwm = base + n;
    if (n) t->touched = true;
    return PKT_SUCCESS;
}

int pkt_flow_table_export(pkt_flow_table_t* t, pkt_flow_record_t* records, uint64_t cap, uint64_t* n_out, void* stream) {
    if (!t || !n_out) return PKT_ERR_INVALID_ARG;
    if (cap && !records) return flow_fail(t, PKT_ERR_INVALID_ARG, "pkt_flow_table_export: null records");
    if (t->ops) return t->ops->scan(t, records, cap, n_out, stream);
    uint64_t k = 0;
    for (uint64_t s = 0; s < t->slots; s++) {
        const FlowEntry& e = t->e[s];
        if (!e.tag) continue;
        if (k < cap) {
            pkt_flow_record_t& r = records[k];
            memcpy(&r.key, e.key, 40);
            r.first = e.first;
            for (int d = 0; d < 2; d++) {
                r.pkts[d] = e.pkts[d];
                r.bytes[d] = e.bytes[d];
            }
        }
        k++;
    }
    *n_out = k;
    return PKT_SUCCESS;
}

int pkt_flow_table_count(pkt_flow_table_t* t, uint64_t* flows, void* stream) {
    return pkt_flow_table_export(t, nullptr, 0, flows, stream);
}

int pkt_flow_table_clear(pkt_flow_table_t* t, void* stream) {
    if (!t) return PKT_ERR_INVALID_ARG;
    if (t->ops) {
        const int rc = t->ops->clear(t, stream);
        if (rc != PKT_SUCCESS) return rc;
    } else {
        memset(static_cast<void*>(t->e), 0, t->slots * sizeof(FlowEntry));
        for (uint64_t s = 0; s < t->slots; s++) t->e[s].first = ~0ull;
    }
    t->hwm = 0;
    t->touched = false;
    return PKT_SUCCESS;
}

int pkt_flow_table_destroy(pkt_flow_table_t* t) {
    if (!t) return PKT_ERR_INVALID_ARG;
    int rc = PKT_SUCCESS;
    if (t->ops)
        rc = t->ops->destroy(t);
    else
        free(t->e);
    delete t;
    return rc;
}

const char* pkt_flow_table_last_error(const pkt_flow_table_t* t) { return t ? t->err.c_str() : "null table"; }

// ---- pkt_match_batch on host pointers (the CPU model of pktgpu_match.hip), straight from the source terms and
// rules: every rule, every term, byte by byte.
size_t pkt_sizeof_match_term(void) { return sizeof(pkt_match_term_t); }
size_t pkt_sizeof_match_rule(void) { return sizeof(pkt_match_rule_t); }

int pkt_match_host(const pkt_match_term_t* terms, uint32_t nterms, const pkt_match_rule_t* rules, uint32_t nrules,
                   uint32_t default_action, const pkt_batch_t* b, const pkt_chain_t* chain, uint8_t* rule,
                   uint32_t* action, uint8_t* select, uint64_t* matched, uint64_t* hits, uint64_t* bytes) {
    if (match_program_error(terms, nterms, rules, nrules)) return PKT_ERR_INVALID_ARG;
    if (!b || !chain) return PKT_ERR_INVALID_ARG;
    if (b->n >= (1ull << 32)) return PKT_ERR_INVALID_ARG;
    if (((uintptr_t)matched | (uintptr_t)hits | (uintptr_t)bytes) & 7) return PKT_ERR_INVALID_ARG;
    const uint64_t n = b->n;
    if (n == 0) return PKT_SUCCESS;
    if (bad_batch(b) || !chain->n_hdrs || !chain->hdr_type || !chain->hdr_off) return PKT_ERR_INVALID_ARG;
    const BatchSrc src = batch_src(b);
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t off = pkt_off(src, i);
        const uint32_t len = pkt_len(src, i, off);
        const uint8_t* p = b->slab + off;
        uint32_t nh = chain->n_hdrs[i];
        nh = nh > PKT_MAX_HDRS ? PKT_MAX_HDRS : nh;
        uint64_t bits = 0;
        for (uint32_t r = 0; r < nrules; r++) {
            bool all = true;
            for (uint32_t k = 0; k < rules[r].nterms && all; k++) {
                const pkt_match_term_t& m = terms[rules[r].first_term + k];
                bool raw;
                if (m.op == PKT_MATCH_LEN) {
                    raw = m.a <= len && len <= m.b;
                } else {
                    int64_t ho = -1;
                    for (uint32_t j = 0, c = 0; j < nh; j++)
                        if (chain->hdr_type[j * n + i] == m.field.hdr_type && c++ == m.field.occurrence) {
                            ho = chain->hdr_off[j * n + i];
                            break;
                        }
                    raw = ho >= 0 && (uint64_t)ho + kHdrs[m.field.hdr_type].size <= len;
                    if (raw && m.op != PKT_MATCH_HAS) {
                        uint64_t v = 0;  // bits [start..=end], MSB first (width <= 64)
                        for (uint32_t q = m.field.start; q <= m.field.end; q++)
                            v = v << 1 | ((p[ho + (q >> 3)] >> (7 - (q & 7))) & 1u);
                        const uint64_t wm = match_width_mask(m.field.end - m.field.start + 1u);
                        raw = m.op == PKT_MATCH_EQ ? ((v ^ m.a) & m.b & wm) == 0 : (m.a <= v && v <= m.b);
                    }
                }
                all = raw != ((m.flags & PKT_MATCH_NOT) != 0);
            }
            if (all) bits |= 1ull << r;
        }
        const uint32_t first = bits ? (uint32_t)__builtin_ctzll(bits) : PKT_MATCH_NONE;
        const uint32_t act = bits ? rules[first].action : default_action;
        if (rule) rule[i] = (uint8_t)first;
        if (action) action[i] = act;
        if (select) select[i] = act != 0;
        if (matched) matched[i] = bits;
        if (hits) hits[bits ? first : nrules] += 1;
        if (bytes) bytes[bits ? first : nrules] += len;
    }
    return PKT_SUCCESS;
}

// ---- pkt_dispatch_batch / pkt_reorder_batch on host pointers (the CPU models of pktgpu_dispatch.hip): a counting
// sort in index order, and the gather a position at a time.
int pkt_dispatch_host(uint32_t nbuckets, const uint16_t* table, uint32_t table_len, const uint32_t* key,
                      const uint8_t* select, uint64_t n, uint16_t* bucket, uint32_t* perm, uint32_t* rank,
                      uint64_t* start) {
    if (dispatch_create_error(nbuckets, table, table_len, 0, false)) return PKT_ERR_INVALID_ARG;
    if (dispatch_call_error(key, n, 0xFFFFFFFFull, start)) return PKT_ERR_INVALID_ARG;
    if (!bucket && !perm && !rank && !start) return PKT_SUCCESS;
    const uint32_t mask = table ? table_len - 1 : 0;
    uint64_t at[PKT_DISPATCH_MAX_BUCKETS + 2] = {};  // at[b + 1] = bucket b's count, then its next position
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t b = dispatch_bucket(key[i], !select || select[i], nbuckets, table, mask);
        at[b + 1]++;
        if (bucket) bucket[i] = (uint16_t)(b < nbuckets ? b : PKT_DISPATCH_DROP);
    }
    uint64_t sum = 0;
    for (uint32_t b = 0; b <= nbuckets; b++) {  // at[b] = the packets before bucket b
        const uint64_t c = at[b + 1];
        at[b] = sum;
        if (start) start[b] = sum;
        sum += c;
    }
    if (start) start[nbuckets + 1] = n;
    if (!perm && !rank) return PKT_SUCCESS;
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t b = dispatch_bucket(key[i], !select || select[i], nbuckets, table, mask);
        const uint64_t pos = at[b]++;
        if (perm) perm[pos] = (uint32_t)i;
        if (rank) rank[i] = (uint32_t)pos;
    }
    return PKT_SUCCESS;
}

int pkt_reorder_host(const pkt_batch_t* b, const pkt_out_t* cols, const uint32_t* perm, uint64_t m,
                     const uint64_t* seg_start, uint32_t nseg, uint8_t* dst, uint64_t dst_len, uint32_t slot,
                     uint32_t* out_len, const pkt_out_t* out_cols) {
    if (reorder_error(b, cols, perm, m, seg_start, nseg, dst, dst_len, slot, out_len, out_cols, false))
        return PKT_ERR_INVALID_ARG;
    if (m == 0) return PKT_SUCCESS;
    uint64_t seg[PKT_REORDER_MAX_SEGS + 1] = {};
    for (uint32_t s = 0; s <= nseg && nseg; s++) seg[s] = seg_start[s] < m ? seg_start[s] : m;
    const BatchSrc src = batch_src(b);
    const uint8_t* nhc = static_cast<const uint8_t*>(reorder_col(cols, kReorderNHdrs));
    for (uint64_t k = 0; k < m; k++) {
        const ReorderSeg sg = reorder_seg(seg, nseg, (uint32_t)k, (uint32_t)m);
        if (!sg.live) continue;
        const uint64_t p = perm[k];
        const bool empty = p >= b->n;
        if (dst) {
            uint32_t len = 0;
            if (!empty) {
                const uint64_t off = pkt_off(src, p);
                len = pkt_len(src, p, off);
                len = len < slot ? len : slot;
                if (len) memcpy(dst + k * slot, b->slab + off, len);
            }
            const uint32_t up = (len + 15u) & ~15u;
            if (up > len) memset(dst + k * slot + len, 0, up - len);
            if (out_len) out_len[k] = len;
        }
        uint32_t rows = PKT_MAX_HDRS;
        if (nhc && !empty) rows = nhc[p] < PKT_MAX_HDRS ? nhc[p] : PKT_MAX_HDRS;
        for (int c = 0; c < kReorderCols; c++) {
            const uint8_t* in = static_cast<const uint8_t*>(reorder_col(cols, c));
            uint8_t* out = static_cast<uint8_t*>(reorder_col(out_cols, c));
            if (!in || !out) continue;
            const uint32_t sz = kReorderColSize[c];
            if (c == kReorderHdrType || c == kReorderHdrOff) {
                for (uint32_t j = 0; j < rows; j++) {
                    uint8_t* o = out + ((uint64_t)PKT_MAX_HDRS * sg.s0 + (uint64_t)j * sg.ns + (k - sg.s0)) * sz;
                    if (empty) memset(o, 0, sz);
                    else memcpy(o, in + ((uint64_t)j * b->n + p) * sz, sz);
                }
            } else if (empty) {
                memset(out + k * sz, 0, sz);
            } else {
                memcpy(out + k * sz, in + p * sz, sz);
            }
        }
    }
    return PKT_SUCCESS;
}

// ---- pkt_lpm_*: the public calls, and the host handle's sequential loops (the device handle: pktgpu_lpm.hip).
// The compile and the walk are pktgpu_lpm.hpp's, shared with the kernel.
size_t pkt_sizeof_lpm_route(void) { return sizeof(pkt_lpm_route_t); }

static thread_local std::string t_lpm_create_err;  // pkt_lpm_last_error(NULL): the thread's last failed create_host

int pkt_lpm_create_host(const pkt_lpm_route_t* routes, uint32_t nroutes, uint32_t default_nexthop, uint64_t max_bytes,
                        pkt_lpm_t** out) {
    if (!out) {
        t_lpm_create_err = "pkt_lpm_create_host: null argument";
        return PKT_ERR_INVALID_ARG;
    }
    *out = nullptr;
    LpmImage img;
    const int rc = lpm_compile(routes, nroutes, max_bytes, img, t_lpm_create_err);
    if (rc != PKT_SUCCESS) return rc;
    pkt_lpm* t = new pkt_lpm;
    t->info = img.info;
    t->host_words.swap(img.words);
    t->view = img.view(t->host_words.data(), default_nexthop);
    *out = t;
    return PKT_SUCCESS;
}

int pkt_lpm_info(const pkt_lpm_t* t, pkt_lpm_info_t* info) {
    if (!t || !info) return PKT_ERR_INVALID_ARG;
    *info = t->info;
    return PKT_SUCCESS;
}

static void lpm_store(const LpmCall& c, uint64_t i, const LpmResult& r) {
    if (c.route) c.route[i] = r.route;
    if (c.nexthop) c.nexthop[i] = r.nexthop;
    if (c.plen) c.plen[i] = (uint8_t)r.plen;
    if (c.status) c.status[i] = (uint8_t)r.status;
}

static uint32_t rd_be32(const uint8_t* p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }

int pkt_lpm_lookup_batch(pkt_lpm_t* t, const pkt_batch_t* b, const pkt_chain_t* chain, uint32_t which_ip, uint32_t flags,
                         uint32_t* route, uint32_t* nexthop, uint8_t* plen, uint8_t* status, void* stream) {
    if (!t) return PKT_ERR_INVALID_ARG;
    if (!b || !chain) return lpm_fail(t, PKT_ERR_INVALID_ARG, "pkt_lpm_lookup_batch: null argument");
    if (b->n >= (1ull << 32)) return lpm_fail(t, PKT_ERR_INVALID_ARG, "pkt_lpm_lookup_batch: n >= 2^32");
    if (flags & ~PKT_LPM_SRC) return lpm_fail(t, PKT_ERR_INVALID_ARG, "pkt_lpm_lookup_batch: unknown flag bits");
    if (which_ip >= PKT_MAX_HDRS && which_ip != PKT_FLOW_LAST)
        return lpm_fail(t, PKT_ERR_INVALID_ARG, "pkt_lpm_lookup_batch: which_ip is neither below 16 nor PKT_FLOW_LAST");
    const uint64_t n = b->n;
    if (n == 0) return PKT_SUCCESS;
    if (!chain->n_hdrs || !chain->hdr_type || !chain->hdr_off)
        return lpm_fail(t, PKT_ERR_INVALID_ARG, "pkt_lpm_lookup_batch: null chain column");
    const char* msg = t->ops ? batch_slab16_error(b) : batch_null_slab(b) ? "null slab" : nullptr;
    if (!msg) msg = batch_index_error(b);
    if (msg) {
        t->err = std::string("pkt_lpm_lookup_batch: ") + msg;
        return PKT_ERR_INVALID_ARG;
    }
    if (!route && !nexthop && !plen && !status) return PKT_SUCCESS;
    const LpmCall c{false,   batch_src(b), n,     chain->n_hdrs, chain->hdr_type, chain->hdr_off, nullptr, nullptr,
                    which_ip, flags,       route, nexthop,       plen,            status};
    if (t->ops) return t->ops->lookup(t, c, stream);
    const bool need_rec = nexthop || plen;
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t off = pkt_off(c.src, i);
        const uint32_t len = pkt_len(c.src, i, off);
        uint32_t nh = chain->n_hdrs[i], seen = 0, slot = PKT_MAX_HDRS;
        nh = nh > PKT_MAX_HDRS ? PKT_MAX_HDRS : nh;
        for (uint32_t j = 0; j < nh; j++) {
            const uint8_t ty = chain->hdr_type[j * n + i];
            if (ty != PKT_HDR_IPV4 && ty != PKT_HDR_IPV6) continue;
            if (which_ip == PKT_FLOW_LAST || seen == which_ip) slot = j;
            seen++;
        }
        LpmResult r = lpm_miss(t->view, PKT_LPM_NO_IP);
        if (slot < PKT_MAX_HDRS) {
            const bool v4 = chain->hdr_type[slot * n + i] == PKT_HDR_IPV4;
            const uint32_t ip = chain->hdr_off[slot * n + i];
            if (ip + (v4 ? 20u : 40u) > len) {
                r.status = PKT_LPM_SPAN;
            } else {
                const bool src = flags & PKT_LPM_SRC;
                const uint8_t* a = b->slab + off + ip + (v4 ? (src ? 12u : 16u) : (src ? 8u : 24u));
                uint32_t w[4] = {rd_be32(a), 0, 0, 0};
                for (uint32_t q = 1; q < 4 && !v4; q++) w[q] = rd_be32(a + 4 * q);
                r = lpm_lookup(w, v4, t->view, need_rec);
            }
        }
        lpm_store(c, i, r);
    }
    return PKT_SUCCESS;
}

int pkt_lpm_lookup_keys(pkt_lpm_t* t, const pkt_flow_key_t* keys, const uint8_t* key_status, uint64_t n, uint32_t flags,
                        uint32_t* route, uint32_t* nexthop, uint8_t* plen, uint8_t* status, void* stream) {
    if (!t) return PKT_ERR_INVALID_ARG;
    if (n >= (1ull << 32)) return lpm_fail(t, PKT_ERR_INVALID_ARG, "pkt_lpm_lookup_keys: n >= 2^32");
    if (flags & ~PKT_LPM_SRC) return lpm_fail(t, PKT_ERR_INVALID_ARG, "pkt_lpm_lookup_keys: unknown flag bits");
    if ((uintptr_t)keys & 1) return lpm_fail(t, PKT_ERR_INVALID_ARG, "pkt_lpm_lookup_keys: keys not 2-byte aligned");
    if (n == 0) return PKT_SUCCESS;
    if (!keys) return lpm_fail(t, PKT_ERR_INVALID_ARG, "pkt_lpm_lookup_keys: null keys");
    if (!route && !nexthop && !plen && !status) return PKT_SUCCESS;
    const LpmCall c{true,  BatchSrc{}, n,     nullptr, nullptr, nullptr, reinterpret_cast<const uint8_t*>(keys), key_status,
                    0,     flags,      route, nexthop, plen,    status};
    if (t->ops) return t->ops->lookup(t, c, stream);
    const bool need_rec = nexthop || plen;
    for (uint64_t i = 0; i < n; i++) {
        const uint8_t* k = c.keys + 40 * i;
        const uint32_t ver = k[37];
        LpmResult r = lpm_miss(t->view, PKT_LPM_SKIPPED);
        if (!(key_status && key_status[i]) && (ver == 4 || ver == 6)) {
            const uint8_t* a = k + (flags & PKT_LPM_SRC ? 0 : 16);
            uint32_t w[4] = {rd_be32(a), 0, 0, 0};
            for (uint32_t q = 1; q < 4 && ver == 6; q++) w[q] = rd_be32(a + 4 * q);
            r = lpm_lookup(w, ver == 4, t->view, need_rec);
        }
        lpm_store(c, i, r);
    }
    return PKT_SUCCESS;
}

int pkt_lpm_destroy(pkt_lpm_t* t) {
    if (!t) return PKT_ERR_INVALID_ARG;
    const int rc = t->ops ? t->ops->destroy(t) : PKT_SUCCESS;
    delete t;
    return rc;
}

const char* pkt_lpm_last_error(const pkt_lpm_t* t) { return t ? t->err.c_str() : t_lpm_create_err.c_str(); }

// ---- pkt_scan_*: the public calls (the device handle: pktgpu_scan.hip).  The compile, the walk, the refusals and the
// host handle's loop are pktgpu_scan.hpp's, shared with the kernel.
size_t pkt_sizeof_scan_pattern(void) { return sizeof(pkt_scan_pattern_t); }

static thread_local std::string t_scan_create_err;  // pkt_scan_last_error(NULL): the thread's last failed create_host

int pkt_scan_create_host(const uint8_t* bytes, uint64_t nbytes, const pkt_scan_pattern_t* pats, uint32_t npats,
                         uint32_t default_action, pkt_scan_t** out) {
    if (!out) {
        t_scan_create_err = "pkt_scan_create_host: null argument";
        return PKT_ERR_INVALID_ARG;
    }
    *out = nullptr;
    ScanImage img;
    const int rc = scan_compile(bytes, nbytes, pats, npats, img, t_scan_create_err);
    if (rc != PKT_SUCCESS) return rc;
    pkt_scan* s = new pkt_scan;
    s->info = img.info;
    s->host_words.swap(img.words);
    s->view = img.view(s->host_words.data(), default_action);
    *out = s;
    return PKT_SUCCESS;
}

int pkt_scan_info(const pkt_scan_t* s, pkt_scan_info_t* info) {
    if (!s || !info) return PKT_ERR_INVALID_ARG;
    *info = s->info;
    return PKT_SUCCESS;
}

int pkt_scan_batch(pkt_scan_t* s, const pkt_batch_t* b, const pkt_chain_t* chain, uint32_t region, const uint8_t* select,
                   uint8_t* status, uint32_t* pat, uint16_t* off, uint32_t* action, uint8_t* sel, uint32_t* count,
                   uint64_t* matched, uint64_t* hits, void* stream) {
    if (!s) return PKT_ERR_INVALID_ARG;
    if (const char* msg = scan_batch_error(b, chain, region, matched, hits, s->ops != nullptr)) return scan_fail(s, msg);
    if (b->n == 0) return PKT_SUCCESS;
    if (!status && !pat && !off && !action && !sel && !count && !matched && !hits) return PKT_SUCCESS;
    const bool pay = region == PKT_SCAN_PAYLOAD;
    const ScanCall c{batch_src(b), b->n, pay ? chain->n_hdrs : nullptr, pay ? chain->hdr_type : nullptr,
                     pay ? chain->hdr_off : nullptr, region, select, status, pat, off, action, sel, count, matched, hits};
    if (s->ops) return s->ops->run(s, c, stream);
    scan_host_run(s->view, c);
    return PKT_SUCCESS;
}

int pkt_scan_destroy(pkt_scan_t* s) {
    if (!s) return PKT_ERR_INVALID_ARG;
    const int rc = s->ops ? s->ops->destroy(s) : PKT_SUCCESS;
    delete s;
    return rc;
}

const char* pkt_scan_last_error(const pkt_scan_t* s) { return s ? s->err.c_str() : t_scan_create_err.c_str(); }

// ---- pkt_fwd_batch on host pointers (the CPU twin of pktgpu_fwd.hip): a sequential loop over the packets with the
// decision, the checksum arithmetic and the refusals of pktgpu_fwd.hpp, which the kernel shares; the packet's bytes
// are read and written a byte at a time.
size_t pkt_sizeof_fwd_adj(void) { return sizeof(pkt_fwd_adj_t); }

int pkt_fwd_host(const pkt_fwd_adj_t* adj, uint32_t nadj, const pkt_batch_t* b, const pkt_chain_t* chain, uint32_t which_ip,
                 uint32_t flags, pkt_lpm_t* lpm, const uint32_t* nexthop, const uint8_t* select, uint8_t* status,
                 uint32_t* port, uint32_t* adj_index, uint64_t* hits, uint64_t* bytes) {
    if (fwd_adj_error(adj, nadj)) return PKT_ERR_INVALID_ARG;
    if (fwd_call_error(b, chain, which_ip, flags, lpm, nexthop, hits, bytes, false, 0)) return PKT_ERR_INVALID_ARG;
    const uint64_t n = b->n;
    if (n == 0) return PKT_SUCCESS;
    if (fwd_batch_error(b, chain, false)) return PKT_ERR_INVALID_ARG;
    const bool keep_l2 = flags & PKT_FWD_KEEP_L2, write = !(flags & PKT_FWD_NO_WRITE);
    if (!status && !port && !adj_index && !hits && !bytes && !write) return PKT_SUCCESS;
    const BatchSrc src = batch_src(b);
    uint8_t* slab = const_cast<uint8_t*>(b->slab);
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t off = pkt_off(src, i);
        const uint32_t len = pkt_len(src, i, off);
        uint32_t st = PKT_FWD_SKIPPED, out_port = PKT_FWD_NONE, out_adj = PKT_FWD_NONE;
        if (!select || select[i]) {
            uint32_t nh = chain->n_hdrs[i];
            nh = nh > PKT_MAX_HDRS ? PKT_MAX_HDRS : nh;
            FwdFind f;
            for (uint32_t j = 0; j < nh; j++) fwd_find_step(f, which_ip, chain->hdr_type[j * n + i], chain->hdr_off[j * n + i]);
            st = fwd_find_status(f, len, keep_l2);
            if (st == PKT_FWD_OK) {
                const bool v4 = f.ipt == PKT_HDR_IPV4;
                uint8_t* ip = slab + off + f.ipo;
                uint32_t h[3];
                for (uint32_t k = 0; k < 3; k++) h[k] = ip[4 * k] | (uint32_t)ip[4 * k + 1] << 8 | (uint32_t)ip[4 * k + 2] << 16 | (uint32_t)ip[4 * k + 3] << 24;
                const FwdIp fi = fwd_ip_fields(h, v4);
                if (fi.t <= 1u) {
                    st = PKT_FWD_TTL;
                } else {
                    uint32_t a;
                    if (lpm) {
                        const uint8_t* d = ip + (v4 ? 16 : 24);
                        uint32_t w[4] = {rd_be32(d), 0, 0, 0};
                        for (uint32_t q = 1; q < 4 && !v4; q++) w[q] = rd_be32(d + 4 * q);
                        a = lpm_lookup(w, v4, lpm->view, true).nexthop;
                    } else {
                        a = nexthop[i];
                    }
                    out_adj = a;
                    if (a >= nadj) {
                        st = PKT_FWD_NO_ADJ;
                    } else {
                        const FwdAdj e = fwd_pack(adj[a]);
                        st = fwd_adj_status(e.w[4], fi.l3len);
                        if (st == PKT_FWD_OK) {
                            out_port = e.w[3];
                            if (write) {
                                if (!keep_l2) {
                                    memcpy(slab + off + f.eth, adj[a].dmac, 6);
                                    memcpy(slab + off + f.eth + 6, adj[a].smac, 6);
                                }
                                if (v4) {
                                    const uint32_t nw = fwd_v4_word(h[2]);
                                    ip[8] = (uint8_t)nw;
                                    ip[10] = (uint8_t)(nw >> 16);
                                    ip[11] = (uint8_t)(nw >> 24);
                                } else {
                                    ip[7] = (uint8_t)(fi.t - 1u);
                                }
                            }
                        }
                    }
                }
            }
        }
        if (status) status[i] = (uint8_t)st;
        if (port) port[i] = out_port;
        if (adj_index) adj_index[i] = out_adj;
        if (hits) hits[st] += 1;
        if (bytes) bytes[st] += len;
    }
    return PKT_SUCCESS;
}

// ---- pkt_nat_*: the public calls, and the host handle, which is the sequential model of include/pktgpu.h itself (the
// device handle: pktgpu_nat.hip).  The decision, the arithmetic and the stores are pktgpu_nat.hpp's, which the kernels
// share.
size_t pkt_sizeof_nat_static(void) { return sizeof(pkt_nat_static_t); }
size_t pkt_sizeof_nat_record(void) { return sizeof(pkt_nat_record_t); }

static thread_local std::string t_nat_create_err;  // pkt_nat_last_error(NULL): the thread's last failed create_host

namespace {

// the slot of `key` in a host forward table, claimed when `claim` and there is room; kNatNoSlot: none
uint32_t nat_host_slot(NatView& v, uint64_t key, bool claim) {
    uint64_t pos = nat_home(key, v.slots);
    for (uint64_t probes = 0; probes < v.slots; probes++, pos = (pos + 1) & (v.slots - 1)) {
        if (v.fkey[pos] == key) return (uint32_t)pos;
        if (v.fkey[pos] == 0) {
            if (!claim) return kNatNoSlot;
            v.fkey[pos] = key;
            return (uint32_t)pos;
        }
    }
    return kNatNoSlot;
}

// the empty forward table with the statics and the mapped entries in it
void nat_host_rebuild(pkt_nat* t) {
    NatView& v = t->v;
    std::fill(t->h_fkey.begin(), t->h_fkey.end(), 0ull);
    std::fill(t->h_fval.begin(), t->h_fval.end(), PKT_NAT_NONE);
    for (uint32_t k = 0; k < v.nstatic; k++) v.fval[nat_host_slot(v, v.st_in[k], true)] = PKT_NAT_STATIC | k;
    for (uint32_t ent = 0; ent < 3 * v.E; ent++)
        if (v.rev[ent]) v.fval[nat_host_slot(v, v.rev[ent], true)] = ent;
}

void nat_host_clear(pkt_nat* t) {
    std::fill(t->h_rev.begin(), t->h_rev.end(), 0ull);
    std::fill(t->h_seen.begin(), t->h_seen.end(), 0u);
    std::fill(t->h_used.begin(), t->h_used.end(), 0u);
    std::fill(t->h_cursor.begin(), t->h_cursor.end(), 0u);
    nat_host_rebuild(t);
}

int nat_host_batch(pkt_nat* t, const NatCall& c) {
    NatView& v = t->v;
    const uint64_t n = c.n;
    uint8_t* slab = const_cast<uint8_t*>(c.src.slab);
    std::vector<uint8_t> st1(n, PKT_NAT_OK), made(n, 0);
    std::vector<uint32_t> ent1(n, PKT_NAT_NONE);
    bool none_free[3] = {false, false, false};  // nothing is freed within a call
    for (uint64_t i = 0; i < n; i++) {  // the OUT packets in index order
        if (nat_dir(c, i) != PKT_NAT_OUT) continue;
        const uint64_t off = pkt_off(c.src, i);
        const NatPkt k = nat_classify(slab + off, pkt_len(c.src, i, off), c.n_hdrs, c.hdr_type, c.hdr_off, n, i, c.which, 0);
        if (k.st != PKT_NAT_OK) continue;
        const uint32_t slot = nat_host_slot(v, k.key, true);
        if (slot == kNatNoSlot) {
            st1[i] = PKT_NAT_TABLE_FULL;
            continue;
        }
        if (v.fval[slot] == PKT_NAT_NONE) {  // no session: the first free entry at or after the cursor, circularly
            uint32_t e = v.E;
            uint32_t* used = v.used + k.p * v.W;
            for (uint32_t s = 0; s < v.E && !none_free[k.p]; s++) {
                const uint32_t x = (v.cursor[k.p] + s) % v.E;
                if (!(used[x >> 5] >> (x & 31u) & 1u)) {
                    e = x;
                    break;
                }
            }
            if (e == v.E) {
                none_free[k.p] = true;
                st1[i] = PKT_NAT_EXHAUSTED;
                continue;
            }
            used[e >> 5] |= 1u << (e & 31u);
            v.cursor[k.p] = (e + 1) % v.E;
            v.fval[slot] = k.p * v.E + e;
            v.rev[k.p * v.E + e] = k.key;
            v.seen[k.p * v.E + e] = c.now;
            made[i] = 1;
        }
        ent1[i] = v.fval[slot];
    }
    const bool write = !(c.flags & PKT_NAT_NO_WRITE);
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t off = pkt_off(c.src, i);
        const uint32_t len = pkt_len(c.src, i, off);
        const uint32_t d = nat_dir(c, i);
        uint32_t st = PKT_NAT_SKIPPED, ent = PKT_NAT_NONE;
        if (d < 2) {
            const NatPkt k = nat_classify(slab + off, len, c.n_hdrs, c.hdr_type, c.hdr_off, n, i, c.which, d);
            st = k.st;
            if (st == PKT_NAT_OK) {
                if (d == PKT_NAT_OUT) {
                    st = st1[i];
                    ent = ent1[i];
                } else {
                    ent = nat_in_find(v, k.key, st);
                }
            }
            if (st == PKT_NAT_OK) {
                if (!(ent & PKT_NAT_STATIC) && v.seen[ent] < c.now) v.seen[ent] = c.now;
                if (write) nat_rewrite(slab + off + k.ipo, slab + off + k.l4o, k.p, d, nat_target(v, ent, k.p, d));
            }
        }
        if (c.status) c.status[i] = (uint8_t)st;
        if (c.entry) c.entry[i] = ent;
        if (c.created) c.created[i] = made[i];
        if (c.hits) c.hits[st] += 1;
        if (c.bytes) c.bytes[st] += len;
    }
    return PKT_SUCCESS;
}

}  // namespace

int pkt_nat_create_host(const uint8_t* pool, uint32_t naddr, uint32_t port_lo, uint32_t port_hi, uint64_t slots,
                        const pkt_nat_static_t* statics, uint32_t nstatic, pkt_nat_t** out) {
    if (!out) {
        t_nat_create_err = "pkt_nat_create_host: null argument";
        return PKT_ERR_INVALID_ARG;
    }
    *out = nullptr;
    pkt_nat* t = new pkt_nat;
    if (const char* msg = nat_create_error(pool, naddr, port_lo, port_hi, slots, statics, nstatic, t->img)) {
        t_nat_create_err = std::string("pkt_nat_create_host: ") + msg;
        delete t;
        return PKT_ERR_INVALID_ARG;
    }
    const NatImage& g = t->img;
    t->h_fkey.resize(slots);
    t->h_fval.resize(slots);
    t->h_ffirst.resize(slots, ~0u);
    t->h_rev.resize(3ull * g.E);
    t->h_seen.resize(3ull * g.E);
    t->h_used.resize(3ull * g.W);
    t->h_cursor.resize(3);
    NatView& v = t->v;
    nat_view_config(v, g);
    v.fkey = t->h_fkey.data(), v.fval = t->h_fval.data(), v.ffirst = t->h_ffirst.data();
    v.rev = t->h_rev.data(), v.seen = t->h_seen.data(), v.used = t->h_used.data(), v.cursor = t->h_cursor.data();
    v.pool = g.pool.data(), v.pool_sorted = g.pool_sorted.data();
    v.st_in = g.st_in.data(), v.st_out = g.st_out.data(), v.sin_key = g.sin_key.data(), v.sin_idx = g.sin_idx.data();
    nat_host_clear(t);
    *out = t;
    return PKT_SUCCESS;
}

int pkt_nat_batch(pkt_nat_t* t, const pkt_batch_t* b, const pkt_chain_t* chain, uint32_t which_ip, uint32_t flags,
                  uint32_t dir_all, const uint8_t* dir, const uint8_t* select, uint32_t now, uint8_t* status,
                  uint32_t* entry, uint8_t* created, uint64_t* hits, uint64_t* bytes, void* stream) {
    if (!t) return PKT_ERR_INVALID_ARG;
    if (const char* msg = nat_call_error(b, chain, which_ip, flags, dir_all, dir, hits, bytes))
        return nat_fail(t, "pkt_nat_batch", msg);
    if (b->n == 0) return PKT_SUCCESS;
    if (const char* msg = nat_batch_error(b, chain, t->ops != nullptr)) return nat_fail(t, "pkt_nat_batch", msg);
    const NatCall c{batch_src(b), b->n, chain->n_hdrs, chain->hdr_type, chain->hdr_off, which_ip, flags, dir_all, now,
                    dir, select, status, entry, created, hits, bytes};
    return t->ops ? t->ops->batch(t, c, stream) : nat_host_batch(t, c);
}

int pkt_nat_expire(pkt_nat_t* t, uint32_t now, const uint32_t idle[3], uint64_t* n_expired) {
    if (!t) return PKT_ERR_INVALID_ARG;
    if (!idle) return nat_fail(t, "pkt_nat_expire", "null idle");
    if (t->ops) return t->ops->expire(t, now, idle, n_expired);
    NatView& v = t->v;
    uint64_t gone = 0;
    for (uint32_t p = 0; p < 3; p++)
        for (uint32_t e = 0; e < v.E && idle[p]; e++) {
            const uint32_t ent = p * v.E + e;
            if (!v.rev[ent] || (uint64_t)v.seen[ent] + idle[p] > now) continue;
            v.rev[ent] = 0;
            v.used[p * v.W + (e >> 5)] &= ~(1u << (e & 31u));
            gone++;
        }
    nat_host_rebuild(t);
    if (n_expired) *n_expired = gone;
    return PKT_SUCCESS;
}

int pkt_nat_count(pkt_nat_t* t, uint64_t counts[3]) {
    if (!t) return PKT_ERR_INVALID_ARG;
    if (!counts) return nat_fail(t, "pkt_nat_count", "null counts");
    std::vector<uint32_t> copy;
    const uint32_t* used = t->v.used;
    if (t->ops) {
        const int rc = t->ops->fetch(t, nullptr, nullptr, &copy);
        if (rc != PKT_SUCCESS) return rc;
        used = copy.data();
    }
    for (uint32_t p = 0; p < 3; p++) {
        counts[p] = 0;
        for (uint32_t w = 0; w < t->v.W; w++) counts[p] += nat_popc(used[p * t->v.W + w]);
    }
    return PKT_SUCCESS;
}

int pkt_nat_export(pkt_nat_t* t, pkt_nat_record_t* records, uint64_t cap, uint64_t* n_out) {
    if (!t) return PKT_ERR_INVALID_ARG;
    if (!n_out) return nat_fail(t, "pkt_nat_export", "null n_out");
    if (cap && !records) return nat_fail(t, "pkt_nat_export", "null records");
    const NatView& v = t->v;
    std::vector<uint64_t> rev_copy;
    std::vector<uint32_t> seen_copy;
    const uint64_t* rev = v.rev;
    const uint32_t* seen = v.seen;
    if (t->ops) {  // a blocking housekeeping call: the two maps come back and the records are put together here
        const int rc = t->ops->fetch(t, &rev_copy, &seen_copy, nullptr);
        if (rc != PKT_SUCCESS) return rc;
        rev = rev_copy.data(), seen = seen_copy.data();
    }
    std::vector<pkt_nat_record_t> tmp;
    uint64_t k = 0;
    auto emit = [&](const pkt_nat_record_t& r) {
        if (k < cap) {
            if (t->ops) tmp.push_back(r); else records[k] = r;
        }
        k++;
    };
    for (uint32_t p = 0; p < 3; p++)
        for (uint32_t e = 0; e < v.E; e++)
            if (rev[p * v.E + e]) emit(nat_record(rev[p * v.E + e], nat_key(p, t->img.pool[e / v.nports], v.port_lo + e % v.nports), 0, seen[p * v.E + e]));
    for (uint32_t s = 0; s < v.nstatic; s++) emit(nat_record(t->img.st_in[s], t->img.st_out[s], PKT_NAT_REC_STATIC, 0));
    *n_out = k;
    if (t->ops && !tmp.empty()) return t->ops->put(t, records, tmp.data(), tmp.size());
    return PKT_SUCCESS;
}

int pkt_nat_clear(pkt_nat_t* t, void* stream) {
    if (!t) return PKT_ERR_INVALID_ARG;
    if (t->ops) return t->ops->clear(t, stream);
    nat_host_clear(t);
    return PKT_SUCCESS;
}

int pkt_nat_destroy(pkt_nat_t* t) {
    if (!t) return PKT_ERR_INVALID_ARG;
    const int rc = t->ops ? t->ops->destroy(t) : PKT_SUCCESS;
    delete t;
    return rc;
}

const char* pkt_nat_last_error(const pkt_nat_t* t) { return t ? t->err.c_str() : t_nat_create_err.c_str(); }

// ---- pkt_meter_*: the public calls, and the host handle, which is the sequential model of include/pktgpu.h itself (the
// device handle: pktgpu_meter.hip).  The refill, the decision and the stores are pktgpu_meter.hpp's, which the kernels
// share.
size_t pkt_sizeof_meter_cfg(void) { return sizeof(pkt_meter_cfg_t); }
size_t pkt_sizeof_meter_state(void) { return sizeof(pkt_meter_state_t); }

static thread_local std::string t_meter_create_err;  // pkt_meter_last_error(NULL): the thread's last failed create_host

namespace {

int meter_host_batch(pkt_meter* t, const MeterCall& c) {
    const MeterView& v = t->v;
    for (uint64_t i = 0; i < c.n; i++) {
        const uint64_t off = pkt_off(c.src, i);
        const uint32_t len = pkt_len(c.src, i, off);
        const uint32_t k = meter_of(c, v.nmeters, i);
        uint32_t col = PKT_METER_UNMETERED, w = 0;
        if (k != ~0u) {
            w = v.word[k];
            MeterRun run = meter_run_load(v.st[k]);
            col = meter_run_packet(run, v.cfg[k], w, c.time ? c.time[i] : c.now, meter_cost(len, v.adjust),
                                   meter_in_color(c, w, i), len);
            meter_run_store(v.st[k], run);
        }
        meter_emit(c, i, col, w, off, len);
        if (c.hits) c.hits[col] += 1;
        if (c.bytes) c.bytes[col] += len;
    }
    return PKT_SUCCESS;
}

}  // namespace

int pkt_meter_create_host(const pkt_meter_cfg_t* cfg, uint32_t nmeters, int32_t adjust, pkt_meter_t** out) {
    if (!out) {
        t_meter_create_err = "pkt_meter_create_host: null argument";
        return PKT_ERR_INVALID_ARG;
    }
    *out = nullptr;
    if (const char* msg = meter_create_error(cfg, nmeters)) {
        t_meter_create_err = std::string("pkt_meter_create_host: ") + msg;
        return PKT_ERR_INVALID_ARG;
    }
    pkt_meter* t = new pkt_meter;
    meter_pack(cfg, nmeters, t->h_cfg, t->h_word);
    t->h_st.resize(nmeters);
    t->v = MeterView{t->h_cfg.data(), t->h_word.data(), t->h_st.data(), nmeters, adjust};
    for (uint32_t k = 0; k < nmeters; k++) meter_state_reset(t->h_st[k], t->h_cfg[k]);
    *out = t;
    return PKT_SUCCESS;
}

int pkt_meter_batch(pkt_meter_t* t, const pkt_batch_t* b, const pkt_chain_t* chain, uint32_t which_ip, uint32_t flags,
                    uint32_t meter_all, const uint32_t* meter, uint64_t now_ns, const uint64_t* time_ns,
                    const uint8_t* in_color, const uint8_t* select, uint8_t* color, uint8_t* pass, uint8_t* marked,
                    uint64_t* hits, uint64_t* bytes, void* stream) {
    if (!t) return PKT_ERR_INVALID_ARG;
    if (const char* msg = meter_call_error(b, chain, which_ip, flags, meter, time_ns, hits, bytes))
        return meter_fail(t, "pkt_meter_batch", msg);
    if (b->n == 0) return PKT_SUCCESS;
    if (const char* msg = meter_batch_error(b, chain, flags, t->ops != nullptr)) return meter_fail(t, "pkt_meter_batch", msg);
    const bool mark = flags & PKT_METER_MARK;
    const MeterCall c{batch_src(b), b->n, mark ? chain->n_hdrs : nullptr, mark ? chain->hdr_type : nullptr,
                      mark ? chain->hdr_off : nullptr, which_ip, flags, meter_all, meter, now_ns, time_ns, in_color, select,
                      color, pass, marked, hits, bytes};
    return t->ops ? t->ops->batch(t, c, stream) : meter_host_batch(t, c);
}

int pkt_meter_reset(pkt_meter_t* t, void* stream) {
    if (!t) return PKT_ERR_INVALID_ARG;
    if (t->ops) return t->ops->reset(t, stream);
    for (uint32_t k = 0; k < t->v.nmeters; k++) meter_state_reset(t->h_st[k], t->h_cfg[k]);
    return PKT_SUCCESS;
}

int pkt_meter_export(pkt_meter_t* t, uint32_t first, uint32_t count, pkt_meter_state_t* out) {
    if (!t) return PKT_ERR_INVALID_ARG;
    if (first > t->v.nmeters || count > t->v.nmeters - first) return meter_fail(t, "pkt_meter_export", "first + count above nmeters");
    if (count && !out) return meter_fail(t, "pkt_meter_export", "null out");
    if (t->ops) return t->ops->xport(t, first, count, out);
    if (count) memcpy(out, t->h_st.data() + first, (size_t)count * sizeof(pkt_meter_state_t));
    return PKT_SUCCESS;
}

int pkt_meter_destroy(pkt_meter_t* t) {
    if (!t) return PKT_ERR_INVALID_ARG;
    const int rc = t->ops ? t->ops->destroy(t) : PKT_SUCCESS;
    delete t;
    return rc;
}

const char* pkt_meter_last_error(const pkt_meter_t* t) { return t ? t->err.c_str() : t_meter_create_err.c_str(); }

// ---- pkt_frag_batch on host pointers (the CPU twin of pktgpu_frag.hip): two sequential passes over the packets with
// the decision, the fragment header and the refusals of pktgpu_frag.hpp, which the kernels share.  The first pass
// decides and totals; the second, when the outputs fit, writes them a byte at a time.
namespace {

FragPlan frag_plan_host(const BatchSrc& src, const pkt_chain_t* chain, uint64_t n, uint64_t i, uint32_t which_ip,
                        uint32_t flags, const uint16_t* mtu, uint32_t mtu_all, const uint8_t* select) {
    const uint64_t off = pkt_off(src, i);
    FragPlan p{};
    p.len = pkt_len(src, i, off);
    p.st = PKT_FRAG_SKIPPED;
    if (select && !select[i]) return p;
    uint32_t nh = chain->n_hdrs[i];
    nh = nh > PKT_MAX_HDRS ? PKT_MAX_HDRS : nh;
    FragFind f;
    for (uint32_t j = 0; j < nh; j++) frag_find_step(f, which_ip, j, chain->hdr_type[j * n + i], chain->hdr_off[j * n + i]);
    p.st = frag_find_status(f, p.len);
    if (p.st != PKT_FRAG_FITS) return p;
    const uint8_t* ip = src.slab + off + f.ipo;
    uint32_t h[3];
    for (uint32_t k = 0; k < 3; k++) h[k] = ip[4 * k] | (uint32_t)ip[4 * k + 1] << 8 | (uint32_t)ip[4 * k + 2] << 16 | (uint32_t)ip[4 * k + 3] << 24;
    frag_decide(p, f.ipt, f.ipo, p.len, h, mtu ? mtu[i] : mtu_all);
    frag_finish(p, f, nh, flags);
    return p;
}

}  // namespace

int pkt_frag_host(const pkt_batch_t* b, const pkt_chain_t* chain, uint32_t which_ip, uint32_t flags, const uint16_t* mtu,
                  uint32_t mtu_all, const uint8_t* select, uint8_t* status, uint32_t* nfrag, uint32_t* first, uint8_t* dst,
                  uint64_t dst_len, uint64_t out_cap, uint64_t* out_off, uint32_t* out_len, uint32_t* src_index,
                  uint16_t* frag_index, const pkt_chain_t* out_chain, uint64_t* hits, uint64_t* bytes_out_total,
                  uint64_t* n_out) {
    if (bytes_out_total) *bytes_out_total = 0;
    if (n_out) *n_out = 0;
    if (frag_call_error(b, chain, which_ip, flags, mtu, mtu_all, dst, out_cap, out_off, out_len, hits, false))
        return PKT_ERR_INVALID_ARG;
    const uint64_t n = b->n;
    const bool write = !(flags & PKT_FRAG_NO_WRITE);
    const BatchSrc src = batch_src(b);
    uint64_t q = 0, bytes = 0;
    for (uint64_t i = 0; i < n; i++) {
        const FragPlan p = frag_plan_host(src, chain, n, i, which_ip, flags, mtu, mtu_all, select);
        if (status) status[i] = (uint8_t)p.st;
        if (nfrag) nfrag[i] = p.nout;
        if (first) first[i] = p.nout ? (uint32_t)q : PKT_FRAG_NONE;
        if (hits) hits[p.st] += 1;
        q += p.nout;
        bytes += frag_out_bytes(p);
    }
    if (bytes_out_total) *bytes_out_total = bytes;
    if (n_out) *n_out = q;
    if (!write) return PKT_SUCCESS;
    if (out_overflow(q, bytes, out_cap, dst_len)) return PKT_ERR_INVALID_ARG;
    const OutChainCols oc = out_chain_cols(out_chain);
    q = 0;
    uint64_t pos = 0;
    for (uint64_t i = 0; i < n; i++) {
        const FragPlan p = frag_plan_host(src, chain, n, i, which_ip, flags, mtu, mtu_all, select);
        if (!p.nout) continue;
        const uint8_t* s = src.slab + pkt_off(src, i);
        uint32_t h[3] = {0, 0, 0};
        if (p.st == PKT_FRAG_SPLIT)
            for (uint32_t k = 0; k < 3; k++) {
                const uint8_t* ip = s + p.ipo + 4 * k;
                h[k] = ip[0] | (uint32_t)ip[1] << 8 | (uint32_t)ip[2] << 16 | (uint32_t)ip[3] << 24;
            }
        for (uint32_t j = 0; j < p.nout; j++, q++) {
            const uint32_t ol = frag_out_len(p, j);
            uint8_t* d = dst + pos;
            if (p.st == PKT_FRAG_SPLIT) {
                const uint32_t he = p.ipo + 20u;
                memcpy(d, s, he);
                uint32_t o[3];
                frag_header(p, j, h, o);
                for (uint32_t k = 0; k < 12; k++) d[p.ipo + k] = (uint8_t)(o[k >> 2] >> (8u * (k & 3u)));
                memcpy(d + he, s + he + (uint64_t)j * p.per, ol - he);
            } else if (ol) {
                memcpy(d, s, ol);
            }
            memset(d + ol, 0, out_round16(ol) - ol);
            out_off[q] = pos;
            out_len[q] = ol;
            if (src_index) src_index[q] = (uint32_t)i;
            if (frag_index) frag_index[q] = (uint16_t)j;
            if (oc.nh) oc.nh[q] = (uint8_t)p.nh;
            for (uint32_t r = 0; r < p.nh; r++) {
                if (oc.ty) oc.ty[r * out_cap + q] = chain->hdr_type[r * n + i];
                if (oc.of) oc.of[r * out_cap + q] = chain->hdr_off[r * n + i];
            }
            pos += out_round16(ol);
        }
    }
    out_empty_tail(q, out_cap, out_off, out_len, src_index, frag_index, oc.nh);
    return PKT_SUCCESS;
}

// ---- pkt_reasm_batch on host pointers (the CPU twin of pktgpu_reasm.hip).  The classification, the joined header and
// the refusals are pktgpu_reasm.hpp's, which the kernels share; the grouping is NOT the kernels': the members are
// sorted by (key, s) and each datagram is walked fragment by fragment, which is the tiling of include/pktgpu.h as it
// is written.  The kernels reach the same verdict from five words per datagram (reasm_verdict), so a device run that
// equals this one checks that rule too.
namespace {

ReasmRec reasm_rec_host(const BatchSrc& src, const pkt_chain_t* chain, uint64_t n, uint64_t i, uint32_t which_ip,
                        const uint8_t* select) {
    const uint64_t off = pkt_off(src, i);
    ReasmRec r{};
    r.plen = pkt_len(src, i, off);
    r.st = PKT_REASM_SKIPPED;
    if (select && !select[i]) return r;
    uint32_t nh = chain->n_hdrs[i];
    nh = nh > PKT_MAX_HDRS ? PKT_MAX_HDRS : nh;
    FragFind f;
    for (uint32_t j = 0; j < nh; j++) frag_find_step(f, which_ip, j, chain->hdr_type[j * n + i], chain->hdr_off[j * n + i]);
    r.st = reasm_find_status(f, r.plen);
    if (r.st != PKT_REASM_WHOLE) return r;
    const uint8_t* ip = src.slab + off + f.ipo;
    uint32_t h[5];
    for (uint32_t k = 0; k < 5; k++) h[k] = ip[4 * k] | (uint32_t)ip[4 * k + 1] << 8 | (uint32_t)ip[4 * k + 2] << 16 | (uint32_t)ip[4 * k + 3] << 24;
    reasm_classify(r, f, nh, h);
    return r;
}

struct ReasmGroup {  // a datagram: its members are order[lo, hi), sorted by s
    uint64_t lo, hi;
    uint32_t owner, E;
};

int reasm_host(const pkt_batch_t* b, const pkt_chain_t* chain, uint32_t which_ip, uint32_t flags, const uint8_t* select,
               uint8_t* status, uint32_t* out_index, uint8_t* dst, uint64_t dst_len, uint64_t out_cap, uint64_t* out_off,
               uint32_t* out_len, uint32_t* src_index, uint32_t* nfrag, const pkt_chain_t* out_chain, uint64_t* hits,
               uint64_t* bytes_out_total, uint64_t* n_out) {
    const uint64_t n = b->n;
    const bool write = !(flags & PKT_REASM_NO_WRITE);
    const BatchSrc src = batch_src(b);
    std::vector<ReasmRec> rec(n);
    std::vector<uint32_t> order;  // the members
    for (uint64_t i = 0; i < n; i++) {
        rec[i] = reasm_rec_host(src, chain, n, i, which_ip, select);
        if (rec[i].member) order.push_back((uint32_t)i);
    }
    std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
        const ReasmRec &p = rec[x], &q = rec[y];
        if (p.src != q.src) return p.src < q.src;
        if (p.dst != q.dst) return p.dst < q.dst;
        if (p.idp != q.idp) return p.idp < q.idp;
        if (p.s != q.s) return p.s < q.s;
        return x < y;
    });
    std::vector<ReasmGroup> groups;
    std::vector<uint32_t> gof(n);  // a member's datagram
    for (uint64_t lo = 0, hi; lo < order.size(); lo = hi) {
        const ReasmRec& first = rec[order[lo]];
        for (hi = lo + 1; hi < order.size(); hi++) {
            const ReasmRec& r = rec[order[hi]];
            if (!reasm_same_key(first.src, first.dst, first.idp, r.src, r.dst, r.idp)) break;
        }
        // the walk: s_0 = 0, s_(k+1) = e_k, one final member, and it is the last
        uint32_t finals = 0, owner = 0, at = 0;
        bool tiled = true;
        for (uint64_t k = lo; k < hi; k++) {
            const ReasmRec& r = rec[order[k]];
            tiled = tiled && r.s == at;
            at = r.s + r.len;
            finals += r.mf ? 0u : 1u;
            owner = order[k] > owner ? order[k] : owner;
        }
        const ReasmRec& last = rec[order[hi - 1]];
        const uint32_t E = last.s + last.len;
        const uint32_t verdict = !(tiled && finals == 1u && !last.mf) ? PKT_REASM_PENDING
                                 : 20u + E > 65535u                  ? PKT_REASM_TOO_BIG
                                                                     : PKT_REASM_JOINED;
        for (uint64_t k = lo; k < hi; k++) {
            rec[order[k]].st = verdict;
            gof[order[k]] = (uint32_t)groups.size();
        }
        groups.push_back(ReasmGroup{lo, hi, owner, E});
    }
    // the outputs, in owner order
    std::vector<uint32_t> oq(n, PKT_REASM_NONE);
    uint64_t q = 0, bytes = 0;
    auto out_len_of = [&](uint64_t i) -> uint32_t {
        const ReasmRec& r = rec[i];
        if (r.st == PKT_REASM_WHOLE) return flags & PKT_REASM_ONLY_JOINED ? 0u : r.plen;
        if (r.st != PKT_REASM_JOINED || groups[gof[i]].owner != i) return 0u;
        return rec[order[groups[gof[i]].lo]].ipo + 20u + groups[gof[i]].E;
    };
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t ol = out_len_of(i);
        if (!ol) continue;
        oq[i] = (uint32_t)q++;
        bytes += out_round16(ol);
    }
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t st = rec[i].st;
        if (status) status[i] = (uint8_t)st;
        if (out_index) out_index[i] = st == PKT_REASM_JOINED ? oq[groups[gof[i]].owner] : oq[i];
        if (hits) hits[st] += 1;
    }
    if (bytes_out_total) *bytes_out_total = bytes;
    if (n_out) *n_out = q;
    if (!write) return PKT_SUCCESS;
    if (out_overflow(q, bytes, out_cap, dst_len)) return PKT_ERR_INVALID_ARG;
    const OutChainCols oc = out_chain_cols(out_chain);
    uint64_t pos = 0;
    q = 0;
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t ol = out_len_of(i);
        if (!ol) continue;
        uint8_t* d = dst + pos;
        uint64_t rows_of = i;
        uint32_t members = 1;
        if (rec[i].st == PKT_REASM_WHOLE) {
            memcpy(d, src.slab + pkt_off(src, i), ol);
        } else {
            const ReasmGroup& g = groups[gof[i]];
            rows_of = order[g.lo];
            members = (uint32_t)(g.hi - g.lo);
            const uint32_t ipo0 = rec[rows_of].ipo;
            const uint8_t* s0 = src.slab + pkt_off(src, rows_of);
            memcpy(d, s0, ipo0 + 20u);
            uint32_t h[3], o[3];
            for (uint32_t k = 0; k < 3; k++) {
                const uint8_t* ip = s0 + ipo0 + 4 * k;
                h[k] = ip[0] | (uint32_t)ip[1] << 8 | (uint32_t)ip[2] << 16 | (uint32_t)ip[3] << 24;
            }
            reasm_header(g.E, h, o);
            for (uint32_t k = 0; k < 12; k++) d[ipo0 + k] = (uint8_t)(o[k >> 2] >> (8u * (k & 3u)));
            for (uint64_t k = g.lo; k < g.hi; k++) {
                const ReasmRec& m = rec[order[k]];
                memcpy(d + ipo0 + 20u + m.s, src.slab + pkt_off(src, order[k]) + m.ipo + 20u, m.len);
            }
        }
        memset(d + ol, 0, out_round16(ol) - ol);
        out_off[q] = pos;
        out_len[q] = ol;
        if (src_index) src_index[q] = (uint32_t)i;
        if (nfrag) nfrag[q] = members;
        const uint32_t nh = rec[rows_of].nh;
        if (oc.nh) oc.nh[q] = (uint8_t)nh;
        for (uint32_t r = 0; r < nh; r++) {
            if (oc.ty) oc.ty[r * out_cap + q] = chain->hdr_type[r * n + rows_of];
            if (oc.of) oc.of[r * out_cap + q] = chain->hdr_off[r * n + rows_of];
        }
        pos += out_round16(ol);
        q++;
    }
    out_empty_tail(q, out_cap, out_off, out_len, src_index, nfrag, oc.nh);
    return PKT_SUCCESS;
}

}  // namespace

int pkt_reasm_host(const pkt_batch_t* b, const pkt_chain_t* chain, uint32_t which_ip, uint32_t flags, const uint8_t* select,
                   uint8_t* status, uint32_t* out_index, uint8_t* dst, uint64_t dst_len, uint64_t out_cap, uint64_t* out_off,
                   uint32_t* out_len, uint32_t* src_index, uint32_t* nfrag, const pkt_chain_t* out_chain, uint64_t* hits,
                   uint64_t* bytes_out_total, uint64_t* n_out) {
    if (bytes_out_total) *bytes_out_total = 0;
    if (n_out) *n_out = 0;
    if (reasm_call_error(b, chain, which_ip, flags, dst, out_cap, out_off, out_len, hits, false)) return PKT_ERR_INVALID_ARG;
    try {
        return reasm_host(b, chain, which_ip, flags, select, status, out_index, dst, dst_len, out_cap, out_off, out_len,
                          src_index, nfrag, out_chain, hits, bytes_out_total, n_out);
    } catch (const std::bad_alloc&) {  // the twin keeps O(n) host memory
        return PKT_ERR_UNSUPPORTED;
    }
}

// ---- pkt_icmp_err_batch on host pointers (the CPU twin of pktgpu_icmp.hip): two sequential passes over the packets
// with the find step, the decision, the header builders and the refusals of pktgpu_icmp.hpp, which the kernels share.
// The first pass decides and totals; the second, when the outputs fit, writes them a byte at a time and sums the quote
// with the plain RFC 1071 loop.
namespace {

IcmpPlan icmp_plan_host(const BatchSrc& src, const pkt_chain_t* chain, uint64_t n, uint64_t i, uint32_t which_ip,
                        const IcmpCfg& cfg, const uint8_t* code, uint32_t code_all, const uint16_t* mtu, uint32_t mtu_all,
                        const uint8_t* select) {
    const uint64_t off = pkt_off(src, i);
    const uint32_t len = pkt_len(src, i, off);
    IcmpPlan p{};
    const uint32_t c = code ? code[i] : code_all;
    const uint32_t r = cfg.has_map ? cfg.map[c & 0xFFu] : c;
    p.st = icmp_reason_status(select ? select[i] : 1u, r);
    if (p.st != PKT_ICMPE_SENT) return p;
    uint32_t nh = chain->n_hdrs[i];
    nh = nh > PKT_MAX_HDRS ? PKT_MAX_HDRS : nh;
    IcmpFind f;
    for (uint32_t j = 0; j < nh; j++) icmp_find_step(f, which_ip, j, chain->hdr_type[j * n + i], chain->hdr_off[j * n + i]);
    p.st = icmp_find_status(f, len);
    if (p.st != PKT_ICMPE_SENT) return p;
    const uint8_t* s = src.slab + off;
    const uint32_t H = f.ipt == PKT_HDR_IPV4 ? 20u : 40u;
    uint32_t h[7] = {0, 0, 0, 0, 0, 0, 0};
    for (uint32_t k = 0; k < 28u && k < H; k++) h[k >> 2] |= (uint32_t)s[f.ipo + k] << (8u * (k & 3u));
    const uint32_t tb = f.ipo + H < len ? s[f.ipo + H] : 0u;
    icmp_decide(p, f, len, r, h, tb, s[f.eth], mtu ? mtu[i] : mtu_all, cfg);
    return p;
}

}  // namespace

size_t pkt_sizeof_icmp_cfg(void) { return sizeof(pkt_icmp_cfg_t); }

int pkt_icmp_err_host(const pkt_batch_t* b, const pkt_chain_t* chain, uint32_t which_ip, uint32_t flags,
                      const pkt_icmp_cfg_t* cfg, const uint8_t* code, uint32_t code_all, const uint8_t* map,
                      const uint16_t* mtu, uint32_t mtu_all, const uint8_t* select, uint8_t* status, uint32_t* out_index,
                      uint8_t* dst, uint64_t dst_len, uint64_t out_cap, uint64_t* out_off, uint32_t* out_len,
                      uint32_t* src_index, const pkt_chain_t* out_chain, uint64_t* hits, uint64_t* bytes_out_total,
                      uint64_t* n_out) {
    if (bytes_out_total) *bytes_out_total = 0;
    if (n_out) *n_out = 0;
    if (icmp_call_error(b, chain, which_ip, flags, cfg, code_all, mtu, mtu_all, dst, out_cap, out_off, out_len, hits, false))
        return PKT_ERR_INVALID_ARG;
    const uint64_t n = b->n;
    const bool write = !(flags & PKT_ICMPE_NO_WRITE);
    const BatchSrc src = batch_src(b);
    const IcmpCfg cf = icmp_cfg(*cfg, map);
    uint64_t q = 0, bytes = 0;
    for (uint64_t i = 0; i < n; i++) {
        const IcmpPlan p = icmp_plan_host(src, chain, n, i, which_ip, cf, code, code_all, mtu, mtu_all, select);
        const bool sent = p.st == PKT_ICMPE_SENT;
        if (status) status[i] = (uint8_t)p.st;
        if (out_index) out_index[i] = sent ? (uint32_t)q : PKT_ICMPE_NONE;
        if (hits) hits[p.st] += 1;
        if (sent) {
            q += 1;
            bytes += out_round16(icmp_out_len(p));
        }
    }
    if (bytes_out_total) *bytes_out_total = bytes;
    if (n_out) *n_out = q;
    if (!write) return PKT_SUCCESS;
    if (out_overflow(q, bytes, out_cap, dst_len)) return PKT_ERR_INVALID_ARG;
    const OutChainCols oc = out_chain_cols(out_chain);
    q = 0;
    uint64_t pos = 0;
    for (uint64_t i = 0; i < n; i++) {
        const IcmpPlan p = icmp_plan_host(src, chain, n, i, which_ip, cf, code, code_all, mtu, mtu_all, select);
        if (p.st != PKT_ICMPE_SENT) continue;
        const uint8_t* s = src.slab + pkt_off(src, i);
        const uint32_t P = p.ipo - p.eth, H = icmp_hlen(p), ol = icmp_out_len(p);
        uint8_t* d = dst + pos;
        memcpy(d, s + p.eth, P);
        memcpy(d, s + p.eth + 6, 6);
        memcpy(d + 6, s + p.eth, 6);
        uint32_t w[12];
        const uint32_t part = icmp_headers(p, q, cf, w);
        for (uint32_t k = 0; k < H + 8u; k++) d[P + k] = (uint8_t)(w[k >> 2] >> (8u * (k & 3u)));
        const uint8_t* quote = s + p.ipo;
        memcpy(d + P + H + 8u, quote, p.q);
        uint32_t qs = 0;
        for (uint32_t k = 0; k < p.q; k++) qs += k & 1u ? quote[k] : (uint32_t)quote[k] << 8;
        const uint32_t c = icmp_csum(p, part, qs);
        d[P + H + 2u] = (uint8_t)(c >> 8);
        d[P + H + 3u] = (uint8_t)c;
        memset(d + ol, 0, out_round16(ol) - ol);
        out_off[q] = pos;
        out_len[q] = ol;
        if (src_index) src_index[q] = (uint32_t)i;
        const uint32_t rows = p.e_ip - p.e_eth + 1u;
        if (oc.nh) oc.nh[q] = (uint8_t)(rows + 1u > PKT_MAX_HDRS ? PKT_MAX_HDRS : rows + 1u);
        for (uint32_t r = 0; r < rows; r++) {
            if (oc.ty) oc.ty[r * out_cap + q] = chain->hdr_type[(p.e_eth + r) * n + i];
            if (oc.of) oc.of[r * out_cap + q] = (uint16_t)(chain->hdr_off[(p.e_eth + r) * n + i] - p.eth);
        }
        if (rows < PKT_MAX_HDRS) {
            if (oc.ty) oc.ty[rows * out_cap + q] = PKT_HDR_ICMP;
            if (oc.of) oc.of[rows * out_cap + q] = (uint16_t)(P + H);
        }
        pos += out_round16(ol);
        q++;
    }
    out_empty_tail(q, out_cap, out_off, out_len, src_index, static_cast<uint8_t*>(nullptr), oc.nh);
    return PKT_SUCCESS;
}

// ---- pkt_tunnel_*: the host handle, and encap / decap on host pointers (the CPU twins of pktgpu_tunnel.hip): two
// sequential passes over the packets with the search, the decisions, the header words, the rows and the refusals of
// pktgpu_tunnel.hpp, which the kernels share.  The first pass decides and totals; the second, when the outputs fit,
// writes them a byte at a time and sums the inner bytes with the plain RFC 1071 loop.
static thread_local std::string t_tun_create_err;  // pkt_tunnel_last_error(NULL): the thread's last failed create_host

namespace {

// the bytes [pos, pos + 4 * nw) of a packet of `len` bytes as little-endian dwords, zero past the packet
void tun_read(const uint8_t* s, uint32_t len, uint32_t pos, uint32_t nw, uint32_t* o) {
    for (uint32_t k = 0; k < nw; k++) o[k] = 0;
    for (uint32_t k = 0; k < 4u * nw && pos + k < len; k++) o[k >> 2] |= (uint32_t)s[pos + k] << (8u * (k & 3u));
}

TunFind tun_search_host(const pkt_chain_t* chain, uint64_t n, uint64_t i, uint32_t which_ip, uint32_t& nh) {
    nh = chain->n_hdrs[i];
    nh = nh > PKT_MAX_HDRS ? PKT_MAX_HDRS : nh;
    TunFind f;
    for (uint32_t j = 0; j < nh; j++) tun_find_step(f, which_ip, j, chain->hdr_type[j * n + i], chain->hdr_off[j * n + i]);
    return f;
}

TunPlan tun_encap_plan_host(const BatchSrc& src, const pkt_chain_t* chain, uint64_t n, uint64_t i, uint32_t which_ip,
                            const TunView& v, const uint32_t* tunnel, uint32_t tunnel_all, const uint32_t* entropy,
                            const uint8_t* select) {
    TunPlan p{};
    p.st = PKT_TUNE_SKIPPED;
    if (select && !select[i]) return p;
    const uint32_t t = tunnel ? tunnel[i] : tunnel_all;
    p.st = PKT_TUNE_NO_TUNNEL;
    if (t >= v.n) return p;
    const uint64_t off = pkt_off(src, i);
    const uint32_t len = pkt_len(src, i, off);
    uint32_t nh, rd;
    const TunFind f = tun_search_host(chain, n, i, which_ip, nh);
    const TunEnt& e = v.ent[t];
    p.st = tun_encap_find_status(f, e, len, rd);
    if (p.st != PKT_TUNE_OK) return p;
    uint32_t h[2] = {0, 0};
    if (rd != kTunNoRead) tun_read(src.slab + off, len, rd, 2, h);
    tun_encap_decide(p, f, e, t, nh, len, rd, h, entropy ? entropy[i] : 0u);
    return p;
}

TunPlan tun_decap_plan_host(const BatchSrc& src, const pkt_chain_t* chain, uint64_t n, uint64_t i, uint32_t which_ip,
                            const TunView& v, const uint8_t* select, uint32_t& tout) {
    TunPlan p{};
    tout = PKT_TUN_NONE;
    p.st = PKT_TUND_SKIPPED;
    if (select && !select[i]) return p;
    const uint64_t off = pkt_off(src, i);
    const uint32_t len = pkt_len(src, i, off);
    uint32_t nh;
    const TunFind f = tun_search_host(chain, n, i, which_ip, nh);
    p.st = tun_decap_find_status(f, len);
    if (p.st != PKT_TUND_OK) return p;
    const uint32_t H = f.ipt == PKT_HDR_IPV4 ? 20u : 40u;
    uint32_t ip[10], th[4];
    tun_read(src.slab + off, len, f.ipo, 10, ip);
    tun_read(src.slab + off, len, f.ipo + H, 4, th);
    tun_decap_decide(p, f, nh, len, ip, th, v, tout);
    return p;
}

// the second pass: output q of source packet i at dst + pos, by its plan
void tun_write_host(const TunPlan& p, const TunEnt* e, const uint8_t* s, uint64_t q, uint32_t ident, uint8_t* d) {
    const uint32_t ol = tun_out_len(p);
    memcpy(d, s, p.P);
    if (p.patch) {
        d[p.P - 2u] = p.et6 ? 0x86u : 0x08u;
        d[p.P - 1u] = p.et6 ? 0xDDu : 0x00u;
    }
    const uint8_t* inner = s + p.P + p.S;
    memcpy(d + p.P + p.hl, inner, p.I);
    if (p.hl) {
        uint32_t w[18];
        const uint32_t part = tun_headers(p, *e, q, ident, w);
        for (uint32_t k = 0; k < p.hl; k++) d[p.P + k] = (uint8_t)(w[k >> 2] >> (8u * (k & 3u)));
        if (p.cs) {
            uint32_t sum = 0;
            for (uint32_t k = 0; k < p.I; k++) {
                sum += k & 1u ? inner[k] : (uint32_t)inner[k] << 8;
                sum = (sum & 0xFFFFu) + (sum >> 16);
            }
            const uint32_t c = tun_udp_csum(part, sum), at = 4u * tun_csum_word(*e);
            d[at] = (uint8_t)(c >> 8);
            d[at + 1u] = (uint8_t)c;
        }
    }
    memset(d + ol, 0, out_round16(ol) - ol);
}

void tun_rows_host(const TunPlan& p, const TunEnt* e, const pkt_chain_t* chain, uint64_t n, uint64_t i, const OutChainCols& oc,
                   uint64_t out_cap, uint64_t q) {
    const uint32_t rows = tun_out_rows(p);
    if (oc.nh) oc.nh[q] = (uint8_t)rows;
    for (uint32_t r = 0; r < rows; r++) {
        uint32_t ty = 0, of = 0, j = 0;
        int32_t delta = 0;
        if (!tun_out_row(p, e, r, ty, of, j, delta)) {
            ty = chain->hdr_type[j * n + i];
            of = (uint32_t)((int32_t)chain->hdr_off[j * n + i] + delta);
        }
        if (oc.ty) oc.ty[r * out_cap + q] = (uint8_t)ty;
        if (oc.of) oc.of[r * out_cap + q] = (uint16_t)of;
    }
}

// both twins: plan(i) gives packet i's plan (and sets tout)
extern "C++" template <typename Plan>
int tun_host(const pkt_batch_t* b, const pkt_chain_t* chain, uint32_t flags, const pkt_tunnel* tun, uint32_t ok, uint32_t ident,
             uint8_t* status, uint32_t* out_index, uint32_t* tunnel_out, uint8_t* dst, uint64_t dst_len, uint64_t out_cap,
             uint64_t* out_off, uint32_t* out_len, uint32_t* src_index, const pkt_chain_t* out_chain, uint64_t* hits,
             uint64_t* bytes_out_total, uint64_t* n_out, const Plan& plan) {
    const uint64_t n = b->n;
    const BatchSrc src = batch_src(b);
    uint64_t q = 0, bytes = 0;
    for (uint64_t i = 0; i < n; i++) {
        uint32_t tout = PKT_TUN_NONE;
        const TunPlan p = plan(i, tout);
        const bool sent = p.st == ok;
        if (status) status[i] = (uint8_t)p.st;
        if (out_index) out_index[i] = sent ? (uint32_t)q : PKT_TUN_NONE;
        if (tunnel_out) tunnel_out[i] = tout;
        if (hits) hits[p.st] += 1;
        if (sent) {
            q += 1;
            bytes += out_round16(tun_out_len(p));
        }
    }
    if (bytes_out_total) *bytes_out_total = bytes;
    if (n_out) *n_out = q;
    if (flags & PKT_TUN_NO_WRITE) return PKT_SUCCESS;
    if (out_overflow(q, bytes, out_cap, dst_len)) return PKT_ERR_INVALID_ARG;
    const OutChainCols oc = out_chain_cols(out_chain);
    q = 0;
    uint64_t pos = 0;
    for (uint64_t i = 0; i < n; i++) {
        uint32_t tout;
        const TunPlan p = plan(i, tout);
        if (p.st != ok) continue;
        const TunEnt* e = p.hl ? &tun->v.ent[p.t] : nullptr;
        tun_write_host(p, e, src.slab + pkt_off(src, i), q, ident, dst + pos);
        out_off[q] = pos;
        out_len[q] = tun_out_len(p);
        if (src_index) src_index[q] = (uint32_t)i;
        tun_rows_host(p, e, chain, n, i, oc, out_cap, q);
        pos += out_round16(tun_out_len(p));
        q++;
    }
    out_empty_tail(q, out_cap, out_off, out_len, src_index, static_cast<uint8_t*>(nullptr), oc.nh);
    return PKT_SUCCESS;
}

}  // namespace

size_t pkt_sizeof_tunnel_entry(void) { return sizeof(pkt_tunnel_entry_t); }

int pkt_tunnel_create_host(const pkt_tunnel_entry_t* entries, uint32_t count, pkt_tunnel_t** out) {
    if (!out) {
        t_tun_create_err = "pkt_tunnel_create_host: null argument";
        return PKT_ERR_INVALID_ARG;
    }
    *out = nullptr;
    pkt_tunnel* t = new pkt_tunnel;
    const int rc = tun_compile(entries, count, t->img, t_tun_create_err);
    if (rc != PKT_SUCCESS) {
        delete t;
        return rc;
    }
    t->v = TunView{t->img.ent.data(), t->img.slots.data(), count, (uint32_t)t->img.slots.size() - 1u};
    *out = t;
    return PKT_SUCCESS;
}

int pkt_tunnel_destroy(pkt_tunnel_t* t) {
    if (!t) return PKT_ERR_INVALID_ARG;
    const int rc = t->destroy ? t->destroy(t) : PKT_SUCCESS;
    delete t;
    return rc;
}

const char* pkt_tunnel_last_error(const pkt_tunnel_t* t) { return t ? t->err.c_str() : t_tun_create_err.c_str(); }

int pkt_tunnel_encap_host(const pkt_batch_t* b, const pkt_chain_t* chain, uint32_t which_ip, uint32_t flags,
                          const pkt_tunnel_t* tun, const uint32_t* tunnel, uint32_t tunnel_all, const uint32_t* entropy,
                          uint32_t ident, const uint8_t* select, uint8_t* status, uint32_t* out_index, uint8_t* dst,
                          uint64_t dst_len, uint64_t out_cap, uint64_t* out_off, uint32_t* out_len, uint32_t* src_index,
                          const pkt_chain_t* out_chain, uint64_t* hits, uint64_t* bytes_out_total, uint64_t* n_out) {
    if (bytes_out_total) *bytes_out_total = 0;
    if (n_out) *n_out = 0;
    if (tun) tun->err.clear();
    if (const char* msg = tun_call_error(b, chain, which_ip, flags, tun, tunnel, entropy, dst, out_cap, out_off, out_len, hits,
                                         false, 0)) {
        (tun ? tun->err : t_tun_create_err) = std::string("pkt_tunnel_encap_host: ") + msg;
        return PKT_ERR_INVALID_ARG;
    }
    const BatchSrc src = batch_src(b);
    const auto plan = [&](uint64_t i, uint32_t& tout) {
        tout = PKT_TUN_NONE;
        return tun_encap_plan_host(src, chain, b->n, i, which_ip, tun->v, tunnel, tunnel_all, entropy, select);
    };
    return tun_host(b, chain, flags, tun, PKT_TUNE_OK, ident, status, out_index, nullptr, dst, dst_len, out_cap, out_off,
                    out_len, src_index, out_chain, hits, bytes_out_total, n_out, plan);
}

int pkt_tunnel_decap_host(const pkt_batch_t* b, const pkt_chain_t* chain, uint32_t which_ip, uint32_t flags,
                          const pkt_tunnel_t* tun, const uint8_t* select, uint8_t* status, uint32_t* out_index,
                          uint32_t* tunnel_out, uint8_t* dst, uint64_t dst_len, uint64_t out_cap, uint64_t* out_off,
                          uint32_t* out_len, uint32_t* src_index, const pkt_chain_t* out_chain, uint64_t* hits,
                          uint64_t* bytes_out_total, uint64_t* n_out) {
    if (bytes_out_total) *bytes_out_total = 0;
    if (n_out) *n_out = 0;
    if (tun) tun->err.clear();
    if (const char* msg = tun_call_error(b, chain, which_ip, flags, tun, tunnel_out, nullptr, dst, out_cap, out_off, out_len,
                                         hits, false, 0)) {
        (tun ? tun->err : t_tun_create_err) = std::string("pkt_tunnel_decap_host: ") + msg;
        return PKT_ERR_INVALID_ARG;
    }
    const BatchSrc src = batch_src(b);
    const auto plan = [&](uint64_t i, uint32_t& tout) {
        return tun_decap_plan_host(src, chain, b->n, i, which_ip, tun->v, select, tout);
    };
    return tun_host(b, chain, flags, tun, PKT_TUND_OK, 0, status, out_index, tunnel_out, dst, dst_len, out_cap, out_off,
                    out_len, src_index, out_chain, hits, bytes_out_total, n_out, plan);
}

// The PacketSlice of packet i from host chain columns (lib.rs:136-140: hdrs in `insert` order,
// packet.rs:724-731: insert / set_payload).
int pkt_view(const pkt_out_t* out, uint64_t n, uint64_t i, uint8_t types[PKT_MAX_HDRS], uint16_t offs[PKT_MAX_HDRS],
             uint32_t* n_hdrs, uint16_t* payload_off, uint16_t* payload_len) {
    if (!out || !types || !offs || !n_hdrs || !payload_off || !payload_len || i >= n) return PKT_ERR_INVALID_ARG;
    if (!out->status || !out->n_hdrs || !out->hdr_type || !out->hdr_off || !out->payload_off || !out->payload_len)
        return PKT_ERR_INVALID_ARG;
    *n_hdrs = 0;
    *payload_off = *payload_len = 0;
    const int st = out->status[i];
    if (st != PKT_OK) return st;
    const uint32_t nh = out->n_hdrs[i];
    if (nh > PKT_MAX_HDRS) return PKT_ERR_INVALID_ARG;
    for (uint32_t k = 0; k < nh; k++) {
        types[k] = out->hdr_type[(uint64_t)k * n + i];
        offs[k] = out->hdr_off[(uint64_t)k * n + i];
    }
    *n_hdrs = nh;
    *payload_off = out->payload_off[i];
    *payload_len = out->payload_len[i];
    return st;
}

// Packet::ipv4_checksum (src/packet.rs:93-107), Q1 fold included.
uint16_t pkt_ipv4_checksum_host(const uint8_t* v, size_t len) {
    uint32_t s = 0;
    for (size_t i = 0; i + 1 < len; i += 2) {
        if (i == 10) continue;
        s += ((uint32_t)v[i] << 8) | v[i + 1];
    }
    while (s >> 16) s = ((s >> 16) + s) & 0xFFFFu;
    return (uint16_t)~s;
}

}  // extern "C"
