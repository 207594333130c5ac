// pktgpu_dispatch.hpp — what pkt_dispatch_* / pkt_reorder_batch (pktgpu_dispatch.hip) and their host twins
// (pktgpu_host.cpp) share: the refusal rules with their texts, THE bucket rule, the segment search and the
// element sizes of the 49 columns.  Compiles without a HIP compiler.
#pragma once
#include <cstdint>

#include "pktgpu_batch.hpp"

// ---- pkt_dispatch_*
// What is wrong with a dispatcher's definition, as the refusal's text, or nullptr.
inline const char* dispatch_create_error(uint32_t nbuckets, const uint16_t* table, uint32_t table_len, uint64_t max_n,
                                         bool with_max_n) {
    if (nbuckets < 1 || nbuckets > PKT_DISPATCH_MAX_BUCKETS) return "pkt_dispatch: nbuckets not in 1..256";
    if (table) {
        if (table_len < 1 || table_len > PKT_DISPATCH_MAX_TABLE || (table_len & (table_len - 1)))
            return "pkt_dispatch: table_len not a power of two in 1..4096";
        for (uint32_t k = 0; k < table_len; k++)
            if (table[k] >= nbuckets && table[k] != PKT_DISPATCH_DROP)
                return "pkt_dispatch: a table entry that is neither a bucket nor PKT_DISPATCH_DROP";
    }
    if (with_max_n && (max_n < 1 || max_n >= (1ull << 32))) return "pkt_dispatch: max_n not in 1..2^32-1";
    return nullptr;
}

// What is wrong with one call's arguments (max_n: the handle's; the host twin has none and passes 2^32 - 1).
inline const char* dispatch_call_error(const uint32_t* key, uint64_t n, uint64_t max_n, const uint64_t* start) {
    if (n >= (1ull << 32)) return "pkt_dispatch_batch: n >= 2^32";
    if (n > max_n) return "pkt_dispatch_batch: n above the handle's max_n";
    if ((uintptr_t)start & 7) return "pkt_dispatch_batch: start not 8-byte aligned";
    if (n && !key) return "pkt_dispatch_batch: null key";
    return nullptr;
}

// THE bucket rule, as b' in 0..nbuckets (nbuckets = dropped).  table == nullptr: DIRECT mode; else mask =
// table_len - 1.  sel: select[i] != 0, or true without a select.
PKT_HD uint32_t dispatch_bucket(uint32_t key, bool sel, uint32_t nbuckets, const uint16_t* table, uint32_t mask) {
    if (!sel) return nbuckets;
    const uint32_t b = table ? table[key & mask] : key;
    return b < nbuckets ? b : nbuckets;
}

// ---- pkt_reorder_batch
// Element size of each pkt_out_t column, in declaration order (kColSize of pktgpu_ctx.hpp, which needs the HIP
// headers; pktgpu_dispatch.hip checks the two against each other).
constexpr int kReorderCols = 49;
constexpr int kReorderHdrType = 2, kReorderHdrOff = 3, kReorderNHdrs = 1;
constexpr uint8_t kReorderColSize[kReorderCols] = {1, 1, 1, 2, 2, 2, 4, 8, 8, 2, 1, 1, 2, 2, 1, 1, 1, 2, 2, 1, 2,
                                                   1, 1, 2, 4, 4, 2, 1, 1, 4, 2, 1, 1, 16, 16, 2, 2, 4, 4, 1,
                                                   1, 1, 2, 2, 2, 2, 2, 2, 2};
static_assert(sizeof(pkt_out_t) == kReorderCols * sizeof(void*), "pkt_out_t layout");

// column c's pointer of a pkt_out_t (its members are 49 pointers in declaration order)
inline void* reorder_col(const pkt_out_t* o, int c) { return o ? reinterpret_cast<void* const*>(o)[c] : nullptr; }

// What is wrong with a reorder call, as the refusal's text, or nullptr.  slab16: the device's slab rules (null
// slab, alignment); the host twin refuses a null slab alone.
inline const char* reorder_error(const pkt_batch_t* b, const pkt_out_t* cols, const uint32_t* perm, uint64_t m,
                                 const uint64_t* seg_start, uint32_t nseg, const uint8_t* dst, uint64_t dst_len,
                                 uint32_t slot, const uint32_t* out_len, const pkt_out_t* out_cols, bool slab16) {
    if (!b) return "pkt_reorder_batch: null batch";
    if (m >= (1ull << 32)) return "pkt_reorder_batch: m >= 2^32";
    if (nseg > PKT_REORDER_MAX_SEGS) return "pkt_reorder_batch: nseg above 257";
    if (nseg && !seg_start) return "pkt_reorder_batch: null seg_start with nseg > 0";
    if ((uintptr_t)seg_start & 7) return "pkt_reorder_batch: seg_start not 8-byte aligned";
    if (m && !perm) return "pkt_reorder_batch: null perm";
    if (dst) {
        if (slot < 16 || slot % 16) return "pkt_reorder_batch: slot not a multiple of 16, or below 16";
        if ((uintptr_t)dst & 15) return "pkt_reorder_batch: dst not 16-byte aligned";
        if (dst_len / slot < m) return "pkt_reorder_batch: dst_len below m * slot";
        if (b->n) {
            if (const char* msg = slab16 ? batch_slab16_error(b) : (batch_null_slab(b) ? "null slab" : nullptr)) return msg;
            if (const char* msg = batch_index_error(b)) return msg;
        }
    } else if (out_len) {
        return "pkt_reorder_batch: out_len without dst";
    }
    for (int c = 0; c < kReorderCols; c++)
        if (reorder_col(out_cols, c) && !reorder_col(cols, c)) return "pkt_reorder_batch: an out column without its source column";
    return nullptr;
}

// Where position k's slot rows go.  seg[0..nseg] = seg_start clamped to m.  The segment of k is the number of
// ends seg[1..nseg] at or below k (a search: seg is non-decreasing), checked against its bounds afterwards, so
// that whatever seg holds an element index stays below PKT_MAX_HDRS * m.  nseg == 0: one segment [0, m).
struct ReorderSeg {
    bool live;        // the position is written
    uint32_t s0, ns;  // its segment's first position and size
};
template <typename T>  // T: uint32_t (LDS copy) or uint64_t values already clamped to m
PKT_HD ReorderSeg reorder_seg(const T* seg, uint32_t nseg, uint32_t k, uint32_t m) {
    if (nseg == 0) return ReorderSeg{true, 0u, m};
    uint32_t lo = 0, hi = nseg;  // the count of ends at or below k lies in [lo, hi]
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;  // end mid + 1
        if ((uint32_t)seg[mid + 1] <= k) lo = mid + 1;
        else hi = mid;
    }
    if (lo >= nseg) return ReorderSeg{false, 0u, 0u};
    const uint32_t s0 = (uint32_t)seg[lo], s1 = (uint32_t)seg[lo + 1];
    if (!(s0 <= k && k < s1)) return ReorderSeg{false, 0u, 0u};
    return ReorderSeg{true, s0, s1 - s0};
}
