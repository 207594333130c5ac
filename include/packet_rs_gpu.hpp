// packet_rs_gpu.hpp — C++ host mirror of packet_rs's decode API over the pktgpu C ABI.
//
// Shapes follow the reference so that C++ callers read like packet_rs users:
//   packet_rs::parser::fast::parse(&[u8]) -> PacketSlice      (src/parser/fast.rs:5)
//   PacketSlice::{payload, len, to_vec}, Index<&str>          (src/packet.rs:714-743, 61-67)
//   <Hdr>Slice::<field>() / bytes(msb, lsb) / name() / len()   (src/headers.rs:172-296)
// but work on whole batches: `Parser::parse` runs pkt_parse_batch on the GPU, `BatchResult`
// holds the host copy of the columns, and `BatchResult::slice(i, bytes)` rebuilds packet i's
// PacketSlice over the caller's bytes (zero-copy, like the reference's borrowed views).
// Header-only; link with libpktgpu.so and the HIP runtime.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "pktgpu.h"

namespace packet_rs {
namespace gpu {

inline void check(int rc, const pkt_ctx_t* ctx, const char* what) {
    if (rc != PKT_SUCCESS)
        throw std::runtime_error(std::string(what) + " failed (" + std::to_string(rc) + "): " +
                                 (ctx ? pkt_ctx_last_error(ctx) : ""));
}
inline void lpm_check(int rc, const pkt_lpm_t* t, const char* what) {
    if (rc != PKT_SUCCESS)
        throw std::runtime_error(std::string(what) + " failed (" + std::to_string(rc) + "): " + pkt_lpm_last_error(t));
}
inline void hip_check(hipError_t e, const char* what) {
    if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}

// `<Hdr>Slice<'a>`: a header name plus a borrowed view of its bytes.
class HeaderSlice {
   public:
    HeaderSlice(int type, const uint8_t* p) : type_(type), p_(p) {}
    const char* name() const { return pkt_hdr_name(type_); }            // headers.rs:218-220
    size_t len() const { return (size_t)pkt_hdr_size(type_); }           // headers.rs:215-217
    int type() const { return type_; }
    const uint8_t* as_slice() const { return p_; }                       // headers.rs:221-223
    // headers.rs:253-263 (widths > 64: the release build's result, Q8)
    uint64_t bit_range(size_t msb, size_t lsb) const {
        uint64_t v = 0;
        for (size_t i = lsb; i <= msb; i++) v = (v << 1) | ((p_[i / 8] >> (7 - i % 8)) & 1u);
        const size_t sh = (64 - (msb - lsb + 1)) & 63;
        return v << sh >> sh;
    }
    // headers.rs:202-211
    std::vector<uint8_t> bytes(size_t msb, size_t lsb) const {
        std::vector<uint8_t> out;
        for (size_t i = lsb; i <= msb; i += 8) out.push_back((uint8_t)bit_range(i + 7, i));
        return out;
    }
    // `<Hdr>Slice::<field>()` by name, e.g. h.field("ttl")
    uint64_t field(const char* fname) const {
        for (int k = 0; k < pkt_hdr_field_count(type_); k++) {
            const char* nm;
            uint16_t s, e;
            pkt_hdr_field(type_, k, &nm, &s, &e);
            if (std::strcmp(nm, fname) == 0) return bit_range(e, s);
        }
        throw std::out_of_range(std::string(name()) + " has no field " + fname);
    }

   private:
    int type_;
    const uint8_t* p_;
};

// `PacketSlice<'a>` (lib.rs:136-140).
class PacketSlice {
   public:
    std::vector<HeaderSlice> hdrs;
    const uint8_t* payload_ptr = nullptr;
    size_t payload_len = 0;

    std::pair<const uint8_t*, size_t> payload() const { return {payload_ptr, payload_len}; }
    size_t len() const {  // packet.rs:741-743
        size_t s = payload_len;
        for (const auto& h : hdrs) s += h.len();
        return s;
    }
    std::vector<uint8_t> to_vec() const {  // packet.rs:733-740
        std::vector<uint8_t> v;
        for (const auto& h : hdrs) v.insert(v.end(), h.as_slice(), h.as_slice() + h.len());
        v.insert(v.end(), payload_ptr, payload_ptr + payload_len);
        return v;
    }
    // Index<&str>: the first header with that name (packet.rs:64-66); throws like unwrap().
    const HeaderSlice& operator[](const char* name) const {
        for (const auto& h : hdrs)
            if (std::strcmp(h.name(), name) == 0) return h;
        throw std::out_of_range(std::string("no header ") + name);
    }
};

// Host copy of the chain + field columns of one batch.
struct BatchResult {
    uint64_t n = 0;
    std::vector<uint8_t> status, n_hdrs, hdr_type;
    std::vector<uint16_t> hdr_off, payload_off, payload_len;
    std::vector<uint32_t> hdr_mask;

    // packet i's PacketSlice over its bytes `pkt` (the same bytes that were parsed).
    PacketSlice slice(uint64_t i, const uint8_t* pkt) const {
        if (status[i] != PKT_OK)
            throw std::runtime_error(std::string("packet ") + std::to_string(i) + ": " + pkt_status_name(status[i]));
        PacketSlice s;
        for (int j = 0; j < n_hdrs[i]; j++)
            s.hdrs.emplace_back(hdr_type[(uint64_t)j * n + i], pkt + hdr_off[(uint64_t)j * n + i]);
        s.payload_ptr = pkt + payload_off[i];
        s.payload_len = payload_len[i];
        return s;
    }
};

// A pkt_ctx plus device scratch for the chain columns.
struct DeviceFree {
    void operator()(void* p) const { (void)hipFree(p); }
};

class Parser {
   public:
    explicit Parser(int device = 0) { check(pkt_ctx_create(device, &ctx_), nullptr, "pkt_ctx_create"); }
    ~Parser() { pkt_ctx_destroy(ctx_); }
    Parser(const Parser&) = delete;
    Parser& operator=(const Parser&) = delete;
    pkt_ctx_t* ctx() { return ctx_; }

    // fast::parse_<entry> over a device batch; chain columns only, copied back to the host.
    BatchResult parse_chain(const pkt_batch_t& b, pkt_entry_t entry = PKT_ENTRY_PARSE, hipStream_t s = nullptr) {
        BatchResult r;
        r.n = b.n;
        if (b.n == 0) return r;
        const uint64_t n = b.n;
        void* d = nullptr;
        const size_t bytes = n * (1 + 1 + PKT_MAX_HDRS + 2 * PKT_MAX_HDRS + 2 + 2 + 4) + 64;
        hip_check(hipMalloc(&d, bytes), "hipMalloc");
        // freed on every exit, including a hip_check throw below
        std::unique_ptr<void, DeviceFree> guard(d);
        uint8_t* base = static_cast<uint8_t*>(d);
        pkt_out_t o;
        std::memset(&o, 0, sizeof(o));
        size_t off = 0;
        auto take = [&](size_t nb, size_t align) {
            off = (off + align - 1) / align * align;
            uint8_t* p = base + off;
            off += nb;
            return p;
        };
        o.hdr_mask = reinterpret_cast<uint32_t*>(take(4 * n, 4));
        o.hdr_off = reinterpret_cast<uint16_t*>(take(2 * n * PKT_MAX_HDRS, 2));
        o.payload_off = reinterpret_cast<uint16_t*>(take(2 * n, 2));
        o.payload_len = reinterpret_cast<uint16_t*>(take(2 * n, 2));
        o.status = take(n, 1);
        o.n_hdrs = take(n, 1);
        o.hdr_type = take(n * PKT_MAX_HDRS, 1);
        int rc = pkt_parse_batch(ctx_, &b, entry, &o, s);
        if (rc == PKT_SUCCESS) {
            r.status.resize(n); r.n_hdrs.resize(n); r.hdr_type.resize(n * PKT_MAX_HDRS);
            r.hdr_off.resize(n * PKT_MAX_HDRS); r.payload_off.resize(n); r.payload_len.resize(n);
            r.hdr_mask.resize(n);
            hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
            hip_check(hipMemcpy(r.status.data(), o.status, n, hipMemcpyDeviceToHost), "copy");
            hip_check(hipMemcpy(r.n_hdrs.data(), o.n_hdrs, n, hipMemcpyDeviceToHost), "copy");
            hip_check(hipMemcpy(r.hdr_type.data(), o.hdr_type, n * PKT_MAX_HDRS, hipMemcpyDeviceToHost), "copy");
            hip_check(hipMemcpy(r.hdr_off.data(), o.hdr_off, 2 * n * PKT_MAX_HDRS, hipMemcpyDeviceToHost), "copy");
            hip_check(hipMemcpy(r.payload_off.data(), o.payload_off, 2 * n, hipMemcpyDeviceToHost), "copy");
            hip_check(hipMemcpy(r.payload_len.data(), o.payload_len, 2 * n, hipMemcpyDeviceToHost), "copy");
            hip_check(hipMemcpy(r.hdr_mask.data(), o.hdr_mask, 4 * n, hipMemcpyDeviceToHost), "copy");
        }
        check(rc, ctx_, "pkt_parse_batch");
        return r;
    }

    // tests/pcap.rs:7-37 on the GPU: every record of a pcap capture in host memory through
    // fast::parse_<entry> (pkt_parse_pcap_host: copy in, device index, parse, chain columns back).
    // offsets[i] = record i's data offset in `file`, so BatchResult::slice(i, file + offsets[i]) is
    // its PacketSlice.  Throws like the reference's unwrap on a malformed capture.
    BatchResult parse_pcap(const uint8_t* file, size_t len, std::vector<uint64_t>& offsets,
                           pkt_entry_t entry = PKT_ENTRY_PARSE) {
        uint64_t n = 0;
        check(pkt_pcap_index(file, len, nullptr, nullptr, 0, &n), nullptr, "pkt_pcap_index (malformed capture)");
        BatchResult r;
        r.n = n;
        offsets.assign(n, 0);
        if (n == 0) return r;
        r.status.resize(n); r.n_hdrs.resize(n); r.hdr_type.resize(n * PKT_MAX_HDRS);
        r.hdr_off.resize(n * PKT_MAX_HDRS); r.payload_off.resize(n); r.payload_len.resize(n);
        r.hdr_mask.resize(n);
        std::vector<uint32_t> lens(n);
        pkt_out_t o;
        std::memset(&o, 0, sizeof(o));
        o.status = r.status.data();
        o.n_hdrs = r.n_hdrs.data();
        o.hdr_type = r.hdr_type.data();
        o.hdr_off = r.hdr_off.data();
        o.payload_off = r.payload_off.data();
        o.payload_len = r.payload_len.data();
        o.hdr_mask = r.hdr_mask.data();
        uint64_t m = 0;
        check(pkt_parse_pcap_host(ctx_, file, len, entry, &o, offsets.data(), lens.data(), n, &m), ctx_,
              "pkt_parse_pcap_host");
        return r;
    }

    // tests/pcap.rs:7-37 (`pcap_write`) on the GPU: the packets of a device batch with select[i] != 0
    // (select NULL: all), in batch order, as one capture in the device buffer `dst` (16-byte aligned,
    // dst_len bytes), every record stamped (tv_sec, tv_usec) as the reference stamps one time on the file.
    // Returns the capture's size; *n_out = its record count.  Throws with the size needed when the
    // capture is larger than dst_len.
    uint64_t pcap_write(const pkt_batch_t& b, uint8_t* dst, uint64_t dst_len, const uint8_t* select = nullptr,
                        uint32_t tv_sec = 0, uint32_t tv_usec = 0, uint64_t* n_out = nullptr, hipStream_t s = nullptr) {
        uint64_t total = 0, n = 0;
        const int rc = pkt_pcap_write(ctx_, &b, select, 0, tv_sec, tv_usec, nullptr, nullptr, dst, dst_len, nullptr,
                                      nullptr, nullptr, &total, &n, s);
        if (n_out) *n_out = n;
        if (rc != PKT_SUCCESS && total > dst_len)
            throw std::length_error("pkt_pcap_write: the capture needs " + std::to_string(total) + " bytes");
        check(rc, ctx_, "pkt_pcap_write");
        return total;
    }

    // Packet::compare (packet.rs:326-358) over two device batches: packet i of `a` against packet i of
    // `b` (raw bytes on both sides: run to_vec first for the reference's to_vec order).  result[i] =
    // PKT_CMP_EQUAL / _LEN / _BYTES, matching[i] = the equal positions of the common bytes, first_diff[i]
    // = the first unequal one; device arrays of n, each may be NULL.  `ignore` (at most 16 specs, with
    // chain_a = the chain columns of a parse of `a`) names bit ranges that never count as a difference.
    // Returns the summary: packets per result and the lowest index that is not equal (n if none).
    pkt_cmp_summary_t compare(const pkt_batch_t& a, const pkt_batch_t& b, uint8_t* result = nullptr,
                              uint32_t* matching = nullptr, uint32_t* first_diff = nullptr,
                              const std::vector<pkt_field_spec_t>& ignore = {}, const pkt_chain_t* chain_a = nullptr,
                              hipStream_t s = nullptr) {
        pkt_cmp_summary_t sm{};
        check(pkt_compare_batch(ctx_, &a, &b, chain_a, ignore.data(), (uint32_t)ignore.size(), result, matching,
                                first_diff, &sm, s),
              ctx_, "pkt_compare_batch");
        return sm;
    }

    // Packet::push / insert / pop / remove (packet.rs:117-164) then to_vec (385-392) over a parsed device
    // batch (pkt_edit_batch): the program `ops` (at most 8; an INSERT's bytes are hdr_data[data_off ..],
    // host memory captured at the call) applied to every packet's header list — or only where select[i] !=
    // 0 — and the result written to its slot of `dst` (dst + dst_offsets[i], or i * slot; at most `slot`
    // bytes).  out_len / edit_status (PKT_EDIT_*): device arrays of n, each may be NULL; out_chain: the
    // edited packets' own chain columns, for the calls that follow.  Asynchronous on `s`.
    void edit(const pkt_batch_t& b, const pkt_out_t& parsed, const std::vector<pkt_edit_op_t>& ops,
              const std::vector<uint8_t>& hdr_data, uint8_t* dst, uint64_t dst_len, uint32_t slot,
              const uint64_t* dst_offsets = nullptr, const uint8_t* select = nullptr, uint32_t* out_len = nullptr,
              uint8_t* edit_status = nullptr, const pkt_out_t* out_chain = nullptr, hipStream_t s = nullptr) {
        check(pkt_edit_batch(ctx_, &b, &parsed, ops.data(), (uint32_t)ops.size(), hdr_data.data(),
                             (uint32_t)hdr_data.size(), select, dst, dst_len, dst_offsets, slot, out_len, edit_status,
                             out_chain, s),
              ctx_, "pkt_edit_batch");
    }

    // Every packet's flow key (pkt_flow_key_batch): addresses, ports, protocol and IP version of the
    // which_ip-th IPv4 / IPv6 header of `chain` (PKT_FLOW_LAST: the innermost), its 64-bit hash under `seed`
    // and, with a 40-byte rss_key, the Toeplitz hash NICs compute.  flags: PKT_FLOW_SYMMETRIC | _NO_PORTS.
    // Device arrays of n, each may be NULL; they are what pkt_flow_table_update takes.  Asynchronous on `s`.
    void flow_keys(const pkt_batch_t& b, const pkt_chain_t& chain, pkt_flow_key_t* keys, uint64_t* hash,
                   uint8_t* dir = nullptr, uint32_t* plen = nullptr, uint8_t* status = nullptr,
                   uint32_t which_ip = PKT_FLOW_LAST, uint32_t flags = 0, uint64_t seed = 0, uint32_t* rss = nullptr,
                   const uint8_t* rss_key = nullptr, hipStream_t s = nullptr) {
        check(pkt_flow_key_batch(ctx_, &b, &chain, which_ip, flags, seed, rss_key, keys, hash, rss, dir, plen, status, s),
              ctx_, "pkt_flow_key_batch");
    }

    // A first-match rule table (pkt_match_create): rule r is the AND of terms [first_term, first_term + nterms),
    // a packet takes the action of the lowest rule that matches it, else default_action.  The caller destroys
    // it with pkt_match_destroy after the calls queued on it.
    pkt_match_t* match_program(const std::vector<pkt_match_term_t>& terms, const std::vector<pkt_match_rule_t>& rules,
                               uint32_t default_action = 0) {
        pkt_match_t* m = nullptr;
        check(pkt_match_create(ctx_, terms.data(), (uint32_t)terms.size(), rules.data(), (uint32_t)rules.size(),
                               default_action, &m),
              ctx_, "pkt_match_create");
        return m;
    }

    // The program over a parsed device batch (pkt_match_batch), one pass: rule / action / select / matched are
    // device arrays of n, hits / bytes device uint64_t[nrules + 1] that are added to; each may be NULL.
    // `select` is what pcap_write and edit take.  Asynchronous on `s`.
    void match(pkt_match_t* m, const pkt_batch_t& b, const pkt_chain_t& chain, uint8_t* select, uint8_t* rule = nullptr,
               uint32_t* action = nullptr, uint64_t* matched = nullptr, uint64_t* hits = nullptr,
               uint64_t* bytes = nullptr, hipStream_t s = nullptr) {
        check(pkt_match_batch(m, &b, &chain, rule, action, select, matched, hits, bytes, s), ctx_, "pkt_match_batch");
    }

    // A stable partition of up to max_n packets into nbuckets (1..256) queues (pkt_dispatch_create).  An empty
    // `table` is DIRECT mode (bucket = key when key < nbuckets, else dropped); otherwise it is the RSS indirection
    // table (a power-of-two length up to 4096, entries < nbuckets or PKT_DISPATCH_DROP): bucket = table[key &
    // (len - 1)].  The caller destroys it with pkt_dispatch_destroy after the calls queued on it.
    pkt_dispatch_t* dispatcher(uint32_t nbuckets, const std::vector<uint16_t>& table, uint64_t max_n) {
        pkt_dispatch_t* d = nullptr;
        check(pkt_dispatch_create(ctx_, nbuckets, table.empty() ? nullptr : table.data(), (uint32_t)table.size(), max_n, &d),
              ctx_, "pkt_dispatch_create");
        return d;
    }

    // The partition of n packets by `key` (pkt_dispatch_batch): perm[pos] = source index (buckets in order, source
    // order within a bucket, the dropped last), rank its inverse, bucket[i] the packet's bucket, start (device
    // uint64_t[nbuckets + 2]) the buckets' first positions.  Each may be NULL.  One call at a time per handle.
    // Asynchronous on `s`.
    void dispatch(pkt_dispatch_t* d, const uint32_t* key, uint64_t n, uint32_t* perm, uint64_t* start,
                  uint32_t* rank = nullptr, uint16_t* bucket = nullptr, const uint8_t* select = nullptr,
                  hipStream_t s = nullptr) {
        check(pkt_dispatch_batch(d, key, select, n, bucket, perm, rank, start, s), ctx_, "pkt_dispatch_batch");
    }

    // Packets and columns gathered by `perm` (pkt_reorder_batch): position k takes packet perm[k] into dst + k *
    // slot (out_len[k] = min(length, slot)) and every column that `cols` and `out_cols` both hold.  With seg_start
    // (dispatch's start) and nseg segments the slot columns are laid out per segment, so that segment s is the batch
    // segment(...) below, and positions at or past seg_start[nseg] are not written.  Asynchronous on `s`.
    void reorder(const pkt_batch_t& b, const uint32_t* perm, uint64_t m, uint8_t* dst, uint64_t dst_len, uint32_t slot,
                 uint32_t* out_len, const pkt_out_t* cols = nullptr, const pkt_out_t* out_cols = nullptr,
                 const uint64_t* seg_start = nullptr, uint32_t nseg = 0, hipStream_t s = nullptr) {
        check(pkt_reorder_batch(ctx_, &b, cols, perm, m, seg_start, nseg, dst, dst_len, slot, out_len, out_cols, s), ctx_,
              "pkt_reorder_batch");
    }

    // Segment [s0, s1) (two consecutive values of a HOST copy of dispatch's start) of a segmented reorder as a
    // batch of its own, and its chain in *chain (when the three chain columns were gathered into out_cols).
    static pkt_batch_t segment(uint8_t* dst, uint32_t slot, const uint32_t* out_len, uint64_t s0, uint64_t s1,
                               const pkt_out_t* out_cols = nullptr, pkt_chain_t* chain = nullptr) {
        if (out_cols && chain)
            *chain = pkt_chain_t{out_cols->n_hdrs + s0, out_cols->hdr_type + PKT_MAX_HDRS * s0,
                                 out_cols->hdr_off + PKT_MAX_HDRS * s0};
        return pkt_batch_t{dst + s0 * slot, (s1 - s0) * slot, nullptr, out_len + s0, slot, 0, s1 - s0};
    }

    // A longest-prefix-match route table compiled onto this context's device (pkt_lpm_create; max_bytes 0 = 1 GiB).
    // The caller destroys it with pkt_lpm_destroy after the calls queued on it.
    pkt_lpm_t* lpm(const std::vector<pkt_lpm_route_t>& routes, uint32_t default_nexthop = 0, uint64_t max_bytes = 0) {
        pkt_lpm_t* t = nullptr;
        check(pkt_lpm_create(ctx_, routes.empty() ? nullptr : routes.data(), (uint32_t)routes.size(), default_nexthop,
                             max_bytes, &t), ctx_, "pkt_lpm_create");
        return t;
    }

    // The longest matching route of every packet's destination (flags PKT_LPM_SRC: source) address
    // (pkt_lpm_lookup_batch): route[i] its index (PKT_LPM_NONE: none), nexthop[i], plen[i], status[i]; each may be
    // NULL.  Several lookups on one table may be in flight on different streams.  Asynchronous on `s`.
    static void lpm_lookup(pkt_lpm_t* t, const pkt_batch_t& b, const pkt_chain_t& chain, uint32_t* nexthop,
                           uint32_t* route = nullptr, uint8_t* plen = nullptr, uint8_t* status = nullptr,
                           uint32_t which_ip = 0, uint32_t flags = 0, hipStream_t s = nullptr) {
        lpm_check(pkt_lpm_lookup_batch(t, &b, &chain, which_ip, flags, route, nexthop, plen, status, s), t, "pkt_lpm_lookup_batch");
    }

    // The same over pkt_flow_key_batch's keys and status (pkt_lpm_lookup_keys).
    static void lpm_lookup_keys(pkt_lpm_t* t, const pkt_flow_key_t* keys, const uint8_t* key_status, uint64_t n,
                                uint32_t* nexthop, uint32_t* route = nullptr, uint8_t* plen = nullptr,
                                uint8_t* status = nullptr, uint32_t flags = 0, hipStream_t s = nullptr) {
        lpm_check(pkt_lpm_lookup_keys(t, keys, key_status, n, flags, route, nexthop, plen, status, s), t, "pkt_lpm_lookup_keys");
    }

    // An adjacency table on this context's device (pkt_fwd_create).  The caller destroys it with pkt_fwd_destroy
    // after the calls queued on it.
    pkt_fwd_t* forwarder(const std::vector<pkt_fwd_adj_t>& adj) {
        pkt_fwd_t* f = nullptr;
        check(pkt_fwd_create(ctx_, adj.empty() ? nullptr : adj.data(), (uint32_t)adj.size(), &f), ctx_, "pkt_fwd_create");
        return f;
    }

    // The L3 forwarding rewrite of a routed batch, in place (pkt_fwd_batch): the adjacency index of packet i is
    // nexthop[i], or, with `lpm` (and nexthop NULL), its destination's route in that table; port[i] is the
    // adjacency's port for a forwarded packet and PKT_FWD_NONE otherwise, which pkt_dispatch_batch in DIRECT mode
    // drops.  status / port / adj_index / hits / bytes may each be NULL.  Asynchronous on `s`.
    void forward(pkt_fwd_t* f, const pkt_batch_t& b, const pkt_chain_t& chain, const uint32_t* nexthop, uint32_t* port,
                 uint8_t* status = nullptr, uint32_t* adj_index = nullptr, pkt_lpm_t* lpm = nullptr,
                 const uint8_t* select = nullptr, uint32_t which_ip = 0, uint32_t flags = 0, uint64_t* hits = nullptr,
                 uint64_t* bytes = nullptr, hipStream_t s = nullptr) {
        check(pkt_fwd_batch(f, &b, &chain, which_ip, flags, lpm, nexthop, select, status, port, adj_index, hits, bytes, s),
              ctx_, "pkt_fwd_batch");
    }

    // A NAPT44 session table on this context's device (pkt_nat_create): `pool` holds 4 wire bytes per outside address.
    // The caller destroys it with pkt_nat_destroy after the calls queued on it; pkt_nat_expire / _count / _export /
    // _clear take the handle as it is.
    pkt_nat_t* nat(const std::vector<uint8_t>& pool, uint32_t port_lo, uint32_t port_hi, uint64_t slots,
                   const std::vector<pkt_nat_static_t>& statics = {}) {
        pkt_nat_t* t = nullptr;
        check(pkt_nat_create(ctx_, pool.data(), (uint32_t)(pool.size() / 4), port_lo, port_hi, slots,
                             statics.empty() ? nullptr : statics.data(), (uint32_t)statics.size(), &t), ctx_, "pkt_nat_create");
        return t;
    }

    // The translation of a parsed batch, in place (pkt_nat_batch): packet i goes inside -> outside (PKT_NAT_OUT) or
    // back (PKT_NAT_IN) as dir[i] says, or as dir_all says when `dir` is NULL; `now` is the caller's clock in seconds.
    // status / entry / created / hits / bytes may each be NULL.  Asynchronous on `s`; one call at a time per handle.
    void translate(pkt_nat_t* t, const pkt_batch_t& b, const pkt_chain_t& chain, const uint8_t* dir, uint32_t dir_all,
                   uint32_t now, uint8_t* status = nullptr, uint32_t* entry = nullptr, uint8_t* created = nullptr,
                   const uint8_t* select = nullptr, uint32_t which_ip = 0, uint32_t flags = 0, uint64_t* hits = nullptr,
                   uint64_t* bytes = nullptr, hipStream_t s = nullptr) {
        check(pkt_nat_batch(t, &b, &chain, which_ip, flags, dir_all, dir, select, now, status, entry, created, hits, bytes, s),
              ctx_, "pkt_nat_batch");
    }

    // A table of srTCM / trTCM policers on this context's device (pkt_meter_create); `adjust` is added to every
    // packet's length.  The caller destroys it with pkt_meter_destroy after the calls queued on it; pkt_meter_reset /
    // _export take the handle as it is.
    pkt_meter_t* meters(const std::vector<pkt_meter_cfg_t>& cfg, int32_t adjust = 0) {
        pkt_meter_t* t = nullptr;
        check(pkt_meter_create(ctx_, cfg.data(), (uint32_t)cfg.size(), adjust, &t), ctx_, "pkt_meter_create");
        return t;
    }

    // The metering of a batch (pkt_meter_batch): packet i is coloured against meter[i] (meter_all when `meter` is
    // NULL; an index at or above the table's size leaves it unmetered) at time_ns[i] (now_ns when NULL).  With
    // PKT_METER_MARK in `flags` the REMARK actions write the DSCP in place and `chain` is needed.  color / pass /
    // marked / hits / bytes may each be NULL.  Asynchronous on `s`; one call at a time per handle.
    void meter(pkt_meter_t* t, const pkt_batch_t& b, const uint32_t* meter, uint32_t meter_all, uint64_t now_ns,
               const uint64_t* time_ns = nullptr, uint8_t* color = nullptr, uint8_t* pass = nullptr,
               uint8_t* marked = nullptr, const uint8_t* in_color = nullptr, const uint8_t* select = nullptr,
               const pkt_chain_t* chain = nullptr, uint32_t which_ip = 0, uint32_t flags = 0, uint64_t* hits = nullptr,
               uint64_t* bytes = nullptr, hipStream_t s = nullptr) {
        check(pkt_meter_batch(t, &b, chain, which_ip, flags, meter_all, meter, now_ns, time_ns, in_color, select, color, pass,
                              marked, hits, bytes, s), ctx_, "pkt_meter_batch");
    }

    // What Parser::fragment reports: the outputs and their rounded bytes (the capacities to retry with when `fits`
    // is false: the outputs did not fit out_cap / dst_len, and dst and the per-output arrays are unspecified).
    struct FragTotals {
        uint64_t n_out = 0, bytes = 0;
        bool fits = true;
    };

    // IPv4 fragmentation of a batch to a per-packet MTU (pkt_frag_batch): every packet whose L3 length is above its
    // mtu (mtu[i], or mtu_all when `mtu` is NULL; 0 = no limit) becomes fragments, every other packet that may pass
    // goes through whole, packed at 16-byte-aligned offsets of dst; out_off / out_len (out_cap entries, empty past
    // n_out) make dst an indexed batch and out_chain its chain columns (strided by out_cap).  With
    // PKT_FRAG_NO_WRITE in `flags` only status / nfrag / first / hits and the totals are produced: the sizing pass.
    // Waits for the totals.
    FragTotals fragment(const pkt_batch_t& b, const pkt_chain_t& chain, const uint16_t* mtu, uint32_t mtu_all, uint8_t* dst,
                        uint64_t dst_len, uint64_t out_cap, uint64_t* out_off, uint32_t* out_len,
                        const pkt_chain_t* out_chain = nullptr, uint32_t* src_index = nullptr, uint16_t* frag_index = nullptr,
                        uint8_t* status = nullptr, uint32_t* nfrag = nullptr, uint32_t* first = nullptr,
                        const uint8_t* select = nullptr, uint32_t which_ip = 0, uint32_t flags = 0, uint64_t* hits = nullptr,
                        hipStream_t s = nullptr) {
        FragTotals t;
        const int rc = pkt_frag_batch(ctx_, &b, &chain, which_ip, flags, mtu, mtu_all, select, status, nfrag, first, dst, dst_len,
                                      out_cap, out_off, out_len, src_index, frag_index, out_chain, hits, &t.bytes, &t.n_out, s);
        if (rc == PKT_ERR_INVALID_ARG && (t.n_out || t.bytes)) {
            t.fits = false;
            return t;
        }
        check(rc, ctx_, "pkt_frag_batch");
        return t;
    }

    // ICMP / ICMPv6 errors for the packets a router refuses (pkt_icmp_err_batch): packet i's code is code[i] (or
    // code_all when `code` is NULL), its reason map[code] (or the code itself when `map`, a HOST array of 256 bytes,
    // is NULL), so pkt_fwd_batch's or pkt_frag_batch's status array is `code` as it is.  Every packet that may be
    // answered gives one error packet (swapped MACs, a fresh IP header from `cfg`, the ICMP header, the quote), packed
    // into dst as fragment packs its outputs; out_index[i] is packet i's output.  mtu[i] (or mtu_all) is what a
    // too-big error reports.  With PKT_ICMPE_NO_WRITE in `flags` only status / out_index / hits and the totals are
    // produced.  Waits for the totals.
    FragTotals icmp_errors(const pkt_batch_t& b, const pkt_chain_t& chain, const pkt_icmp_cfg_t& cfg, const uint8_t* code,
                           uint32_t code_all, const uint8_t* map, const uint16_t* mtu, uint32_t mtu_all, uint8_t* dst,
                           uint64_t dst_len, uint64_t out_cap, uint64_t* out_off, uint32_t* out_len,
                           const pkt_chain_t* out_chain = nullptr, uint32_t* src_index = nullptr, uint8_t* status = nullptr,
                           uint32_t* out_index = nullptr, const uint8_t* select = nullptr, uint32_t which_ip = 0,
                           uint32_t flags = 0, uint64_t* hits = nullptr, hipStream_t s = nullptr) {
        FragTotals t;
        const int rc = pkt_icmp_err_batch(ctx_, &b, &chain, which_ip, flags, &cfg, code, code_all, map, mtu, mtu_all, select,
                                          status, out_index, dst, dst_len, out_cap, out_off, out_len, src_index, out_chain, hits,
                                          &t.bytes, &t.n_out, s);
        if (rc == PKT_ERR_INVALID_ARG && (t.n_out || t.bytes)) {
            t.fits = false;
            return t;
        }
        check(rc, ctx_, "pkt_icmp_err_batch");
        return t;
    }

    // A tunnel table on this context's device (pkt_tunnel_create): VXLAN, GRE and IP-in-IP entries that tunnel_encap
    // puts packets into and tunnel_decap takes them out of.  Read-only: calls on several streams share it.  The caller
    // destroys it with pkt_tunnel_destroy after the calls queued on it.
    pkt_tunnel_t* tunnels(const std::vector<pkt_tunnel_entry_t>& entries) {
        pkt_tunnel_t* t = nullptr;
        check(pkt_tunnel_create(ctx_, entries.data(), (uint32_t)entries.size(), &t), ctx_, "pkt_tunnel_create");
        return t;
    }

    // Encapsulation of a parsed batch (pkt_tunnel_encap_batch): packet i goes into entry tunnel[i] (or tunnel_all when
    // `tunnel` is NULL: pkt_lpm_lookup_batch's nexthop or pkt_fwd_batch's adj_index as they are); every packet that may
    // gives one output with correct outer lengths and checksums, packed into dst as fragment packs its outputs, and
    // out_chain holds the outer rows and the source's with their offsets moved.  entropy[i] (NULL: none) spreads
    // VXLAN's UDP source port; the outer IPv4 identification of output q is (ident + q) & 0xFFFF.  With
    // PKT_TUN_NO_WRITE in `flags` only status / out_index / hits and the totals are produced.  Waits for the totals.
    FragTotals tunnel_encap(const pkt_tunnel_t* t, const pkt_batch_t& b, const pkt_chain_t& chain, const uint32_t* tunnel,
                            uint32_t tunnel_all, const uint32_t* entropy, uint32_t ident, uint8_t* dst, uint64_t dst_len,
                            uint64_t out_cap, uint64_t* out_off, uint32_t* out_len, const pkt_chain_t* out_chain = nullptr,
                            uint32_t* src_index = nullptr, uint8_t* status = nullptr, uint32_t* out_index = nullptr,
                            const uint8_t* select = nullptr, uint32_t which_ip = 0, uint32_t flags = 0,
                            uint64_t* hits = nullptr, hipStream_t s = nullptr) {
        FragTotals r;
        const int rc = pkt_tunnel_encap_batch(ctx_, &b, &chain, which_ip, flags, t, tunnel, tunnel_all, entropy, ident, select,
                                              status, out_index, dst, dst_len, out_cap, out_off, out_len, src_index, out_chain,
                                              hits, &r.bytes, &r.n_out, s);
        if (rc == PKT_ERR_INVALID_ARG && (r.n_out || r.bytes)) {
            r.fits = false;
            return r;
        }
        check(rc, ctx_, "pkt_tunnel_encap_batch");
        return r;
    }

    // Decapsulation (pkt_tunnel_decap_batch), the inverse: every packet whose which_ip-th IP entry is the outer header
    // of a tunnel of the table gives its inner packet; tunnel_out[i] is the matched entry (PKT_TUN_NONE: none).  Outer
    // fragments are refused (reassemble first) and no checksum is verified (l4_checksum first).
    FragTotals tunnel_decap(const pkt_tunnel_t* t, const pkt_batch_t& b, const pkt_chain_t& chain, uint8_t* dst,
                            uint64_t dst_len, uint64_t out_cap, uint64_t* out_off, uint32_t* out_len,
                            const pkt_chain_t* out_chain = nullptr, uint32_t* src_index = nullptr, uint8_t* status = nullptr,
                            uint32_t* out_index = nullptr, uint32_t* tunnel_out = nullptr, const uint8_t* select = nullptr,
                            uint32_t which_ip = 0, uint32_t flags = 0, uint64_t* hits = nullptr, hipStream_t s = nullptr) {
        FragTotals r;
        const int rc = pkt_tunnel_decap_batch(ctx_, &b, &chain, which_ip, flags, t, select, status, out_index, tunnel_out, dst,
                                              dst_len, out_cap, out_off, out_len, src_index, out_chain, hits, &r.bytes, &r.n_out,
                                              s);
        if (rc == PKT_ERR_INVALID_ARG && (r.n_out || r.bytes)) {
            r.fits = false;
            return r;
        }
        check(rc, ctx_, "pkt_tunnel_decap_batch");
        return r;
    }

    // IPv4 reassembly of a batch's fragments (pkt_reasm_batch), the inverse of fragment: the fragments are grouped by
    // (src, dst, protocol, identification) and every datagram that is complete in this batch is joined into one packet
    // at the place of its last-arriving member; packets that are no fragments go through whole.  dst, out_off /
    // out_len and out_chain are as fragment's; status[i] == PKT_REASM_PENDING marks the fragments to carry over to
    // the next batch, out_index[i] is the output carrying packet i.  With PKT_REASM_NO_WRITE in `flags` only status /
    // out_index / hits and the totals are produced.  Waits for the totals.
    FragTotals reassemble(const pkt_batch_t& b, const pkt_chain_t& chain, uint8_t* dst, uint64_t dst_len, uint64_t out_cap,
                          uint64_t* out_off, uint32_t* out_len, const pkt_chain_t* out_chain = nullptr,
                          uint32_t* src_index = nullptr, uint32_t* nfrag = nullptr, uint8_t* status = nullptr,
                          uint32_t* out_index = nullptr, const uint8_t* select = nullptr, uint32_t which_ip = 0,
                          uint32_t flags = 0, uint64_t* hits = nullptr, hipStream_t s = nullptr) {
        FragTotals t;
        const int rc = pkt_reasm_batch(ctx_, &b, &chain, which_ip, flags, select, status, out_index, dst, dst_len, out_cap,
                                       out_off, out_len, src_index, nfrag, out_chain, hits, &t.bytes, &t.n_out, s);
        if (rc == PKT_ERR_INVALID_ARG && (t.n_out || t.bytes)) {
            t.fits = false;
            return t;
        }
        check(rc, ctx_, "pkt_reasm_batch");
        return t;
    }

    // A pattern set compiled onto this context's device (pkt_scan_create): `pats[k]` is bytes[off, off + len) of
    // `bytes`, 1..PKT_SCAN_MAX_LEN bytes, with its flags (PKT_SCAN_NOCASE), group and action.  The caller destroys it
    // with pkt_scan_destroy after the calls queued on it.
    pkt_scan_t* scanner(const std::vector<uint8_t>& bytes, const std::vector<pkt_scan_pattern_t>& pats,
                        uint32_t default_action = 0) {
        pkt_scan_t* t = nullptr;
        check(pkt_scan_create(ctx_, bytes.empty() ? nullptr : bytes.data(), bytes.size(), pats.empty() ? nullptr : pats.data(),
                              (uint32_t)pats.size(), default_action, &t), ctx_, "pkt_scan_create");
        return t;
    }

    // Every packet's region searched for the set (pkt_scan_batch): PKT_SCAN_PAYLOAD is the bytes after every header of
    // `chain`, PKT_SCAN_PACKET the whole packet (`chain` may be NULL).  status[i] (PKT_SCAN_HIT / _MISS / ...), pat[i] the
    // lowest occurring pattern (PKT_SCAN_NONE: none), off[i] its first occurrence, action[i], sel[i] = action[i] != 0,
    // count[i] all occurrences, matched[i] the groups; hits[npats + 1] is added to.  Each may be NULL.  Asynchronous on s.
    static void scan(pkt_scan_t* t, const pkt_batch_t& b, const pkt_chain_t* chain, uint8_t* status, uint32_t* pat = nullptr,
                     uint16_t* off = nullptr, uint32_t* action = nullptr, uint8_t* sel = nullptr, uint32_t* count = nullptr,
                     uint64_t* matched = nullptr, uint64_t* hits = nullptr, uint32_t region = PKT_SCAN_PAYLOAD,
                     const uint8_t* select = nullptr, hipStream_t s = nullptr) {
        const int rc = pkt_scan_batch(t, &b, chain, region, select, status, pat, off, action, sel, count, matched, hits, s);
        if (rc != PKT_SUCCESS)
            throw std::runtime_error(std::string("pkt_scan_batch failed (") + std::to_string(rc) + "): " + pkt_scan_last_error(t));
    }

   private:
    pkt_ctx_t* ctx_ = nullptr;
};

}  // namespace gpu
}  // namespace packet_rs
