// pktgpu_scan.hpp — what the two halves of pkt_scan_* share: the handle behind pkt_scan_t, the compiled pattern set
// (two failureless tries: exact patterns, and NOCASE patterns folded; a dense first level, the deeper edges in one
// open-addressed table), its compiler, THE walk from one start position (scan_start), the region rule, the fold,
// the statuses, the per-packet result and the refusals.  pktgpu_host.cpp holds the public pkt_scan_* calls (it
// compiles under g++ alone) and runs a host handle through scan_host_run below; pktgpu_scan.hip holds
// pkt_scan_create and the device handle's kernel, which the handle reaches through `ops`.  The kernel and the host
// loop call the same scan_start, scan_region_* and scan_result, so the CPU tests cover the whole compile-and-walk
// logic, the way pktgpu_lpm.hpp shares the lpm walk.
//
// The image, in 32-bit words:
//   [root 2 x 256]   entry c of trie t (0 exact, 1 folded): the depth-1 state byte c leads to, | kScanOut if a
//                    pattern ends there; 0: no pattern of the trie starts with c
//   [two 2048]       bit (f0 << 8 | f1): some pattern of two bytes or more starts with bytes that fold to f0, f1
//   [deep ...]       the part a small set has in LDS (PKT_SCAN_PLACE_LDS):
//     [slots x 2]      open-addressed, linear probing, at most half full: key = state << 8 | byte, value = the next
//                      state | kScanOut; an empty slot's key is kScanEmpty
//     [nstates + 1]    out_at: state s ends the patterns out_pat[out_at[s] .. out_at[s + 1]), ascending
//     [npats]          out_pat
//     [npats]          group
//   [action npats]   read once per packet
// States 0 and 1 are the two roots; a value of 0 is "no edge".  There are no failure links: a start position walks
// only the patterns that begin there, so the states it passes are exactly the prefixes it spells.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "pktgpu_batch.hpp"

static_assert(sizeof(pkt_scan_pattern_t) == 16 && sizeof(pkt_scan_info_t) == 24, "scan ABI structs");

constexpr uint32_t kScanOut = 0x80000000u;    // an edge's bit 31: the state it leads to ends a pattern
constexpr uint32_t kScanEmpty = 0xFFFFFFFFu;  // an empty slot's key (a key is below 2^26)
constexpr uint32_t kScanFirstWords = 512 + 2048;  // the two root tables and the two-byte bitmap
// PKT_SCAN_PLACE_LDS: the deep part and the block's hit counters together, in words.  With the kernel's static LDS
// (about 24 KiB) a block stays below 64 KiB, the most a launch gets without asking, and a CU holds two blocks.
constexpr uint32_t kScanLdsWords = 8192;

struct alignas(8) ScanSlot {
    uint32_t key, val;
};

// The compiled set as a walk sees it: host or device addresses.
struct ScanView {
    const uint32_t* first;   // root tables, then the bitmap (kScanFirstWords)
    const uint32_t* deep;    // slots, out_at, out_pat, group
    const uint32_t* action;  // [npats]
    uint32_t out_at_w, out_pat_w, group_w, deep_words;  // word offsets inside deep
    uint32_t hshift, hmask;  // slot = key * golden >> hshift; slots - 1
    uint32_t max_len, npats, default_action;
};

// What scan_start reads; the kernel points the parts at LDS.
struct ScanTabs {
    const uint32_t* root;
    const uint32_t* two;
    const ScanSlot* slots;
    const uint32_t* out_at;
    const uint32_t* out_pat;
    uint32_t hshift, hmask, max_len;
};

PKT_HD ScanTabs scan_tabs(const uint32_t* first, const uint32_t* deep, const ScanView& v) {
    return ScanTabs{first, first + 512, reinterpret_cast<const ScanSlot*>(deep), deep + v.out_at_w, deep + v.out_pat_w,
                    v.hshift, v.hmask, v.max_len};
}

// THE fold of PKT_SCAN_NOCASE: 'A'..'Z' to 'a'..'z', nothing else
PKT_HD uint32_t scan_fold(uint32_t c) { return c - 0x41u < 26u ? c + 0x20u : c; }

PKT_HD uint32_t scan_hash(uint32_t key, uint32_t hshift) { return key * 0x9E3779B1u >> hshift; }

// the edge out of state st on byte c: the next state | kScanOut, or 0.  The table is at most half full, so a probe
// sequence ends at an empty slot.
PKT_HD uint32_t scan_next(const ScanTabs& t, uint32_t st, uint32_t c) {
    const uint32_t key = st << 8 | c;
    uint32_t h = scan_hash(key, t.hshift);
    for (;;) {
        const ScanSlot s = t.slots[h];
        if (s.key == key) return s.val;
        if (s.key == kScanEmpty) return 0u;
        h = (h + 1u) & t.hmask;
    }
}

template <class Emit>
PKT_HD void scan_outs(const ScanTabs& t, uint32_t st, Emit& emit) {
    for (uint32_t k = t.out_at[st], e = t.out_at[st + 1u]; k < e; k++) emit(t.out_pat[k]);
}

// THE walk: emit(p) for every pattern p that occurs at p0[0], of which `avail` >= 1 bytes belong to the region (the
// caller guarantees min(avail, 64) readable bytes).  Most starts end at the two root entries or at the bitmap.
template <class Emit>
PKT_HD void scan_start(const ScanTabs& t, const uint8_t* p0, uint32_t avail, Emit& emit) {
    const uint32_t c0 = p0[0], f0 = scan_fold(c0);
    const uint32_t e0 = t.root[c0], e1 = t.root[256u + f0];
    if (!(e0 | e1)) return;
    if (e0 & kScanOut) scan_outs(t, e0 & ~kScanOut, emit);
    if (e1 & kScanOut) scan_outs(t, e1 & ~kScanOut, emit);
    const uint32_t lim = avail < t.max_len ? avail : t.max_len;  // a state at depth max_len has no edge
    if (lim < 2u) return;
    const uint32_t two = f0 << 8 | scan_fold(p0[1]);
    if (!(t.two[two >> 5] >> (two & 31u) & 1u)) return;
    for (uint32_t tr = 0; tr < 2u; tr++) {
        uint32_t st = (tr ? e1 : e0) & ~kScanOut;
        for (uint32_t d = 1; st && d < lim; d++) {
            const uint32_t c = tr ? scan_fold(p0[d]) : p0[d];
            const uint32_t v = scan_next(t, st, c);
            st = v & ~kScanOut;
            if (v & kScanOut) scan_outs(t, st, emit);
        }
    }
}

// ---- the region rule.  PAYLOAD: feed the list's first min(n_hdrs, PKT_MAX_HDRS) entries in order.
struct ScanRegion {
    uint32_t r0 = 0;
    bool bad = false;  // a hdr_type outside 1..21
};

PKT_HD uint32_t scan_hdr_size(uint32_t ty) {
    constexpr uint8_t sz[PKT_HDR_COUNT] = PKT_HDR_SIZE_LIST;
    return sz[ty];
}

PKT_HD void scan_region_step(ScanRegion& r, uint32_t ty, uint32_t of) {
    if (ty - 1u >= (uint32_t)PKT_HDR_COUNT - 1u) {
        r.bad = true;
        return;
    }
    const uint32_t end = of + scan_hdr_size(ty);
    r.r0 = end > r.r0 ? end : r.r0;
}

// PKT_SCAN_MISS: the packet is scanned, over [r.r0, r1)
PKT_HD uint32_t scan_region_status(const ScanRegion& r, uint32_t n_hdrs, uint32_t r1) {
    if (n_hdrs == 0) return PKT_SCAN_NO_CHAIN;
    if (r.bad || r.r0 > r1) return PKT_SCAN_SPAN;
    return PKT_SCAN_MISS;
}

// ---- one packet's outputs from its reductions: count, best = the minimum of (pattern << 16 | s) over its
// occurrences (any value when there is none), matched
struct ScanOut {
    uint32_t status, pat, off, action, count;
    uint64_t matched;
};

constexpr uint64_t kScanNoBest = ~0ull;

PKT_HD ScanOut scan_result(uint32_t region_status, uint32_t count, uint64_t best, uint64_t matched, const ScanView& v) {
    if (region_status != PKT_SCAN_MISS)
        return ScanOut{region_status, PKT_SCAN_NONE, 0u, region_status == PKT_SCAN_SKIPPED ? 0u : v.default_action, 0u, 0ull};
    if (count == 0) return ScanOut{PKT_SCAN_MISS, PKT_SCAN_NONE, 0u, v.default_action, 0u, 0ull};
    const uint32_t p = (uint32_t)(best >> 16);
    return ScanOut{PKT_SCAN_HIT, p, (uint32_t)best & 0xFFFFu, v.action[p], count, matched};
}

// One call's arguments, as the device half takes them.
struct ScanCall {
    BatchSrc src;
    uint64_t n;
    const uint8_t* n_hdrs;
    const uint8_t* hdr_type;
    const uint16_t* hdr_off;
    uint32_t region;
    const uint8_t* select;
    uint8_t* status;
    uint32_t* pat;
    uint16_t* off;
    uint32_t* action;
    uint8_t* sel;
    uint32_t* count;
    uint64_t* matched;
    uint64_t* hits;
};

template <class Call>  // ScanCall, or a kernel's parameter struct with the same output members
PKT_HD void scan_store(const Call& c, uint64_t i, const ScanOut& o) {
    if (c.status) c.status[i] = (uint8_t)o.status;
    if (c.pat) c.pat[i] = o.pat;
    if (c.off) c.off[i] = (uint16_t)o.off;
    if (c.action) c.action[i] = o.action;
    if (c.sel) c.sel[i] = o.action != 0;
    if (c.count) c.count[i] = o.count;
    if (c.matched) c.matched[i] = o.matched;
}

// ------------------------------------------------------------------ the compiler (host code)

struct ScanImage {
    std::vector<uint32_t> words;
    pkt_scan_info_t info{};
    uint32_t slots = 0, deep_words = 0, out_at_w = 0, out_pat_w = 0, group_w = 0;
    uint64_t action_at = 0;  // in words, from the image's start
    bool fits_lds = false;
    ScanView view(const uint32_t* base, uint32_t default_action) const {
        uint32_t lg = 0;
        while ((1u << lg) < slots) lg++;
        return ScanView{base,       base + kScanFirstWords, base + action_at, out_at_w,      out_pat_w,     group_w,
                        deep_words, 32u - lg,               slots - 1u,       info.max_len,  info.npatterns, default_action};
    }
};

inline int scan_refuse(std::string& err, const std::string& msg) {
    err = "pkt_scan_create: " + msg;
    return PKT_ERR_INVALID_ARG;
}

// Validate the patterns and compile them.  PKT_SUCCESS, or the refusal with its text in `err`.
inline int scan_compile(const uint8_t* bytes, uint64_t nbytes, const pkt_scan_pattern_t* pats, uint32_t n, ScanImage& img,
                        std::string& err) {
    if (n > PKT_SCAN_MAX_PATTERNS) return scan_refuse(err, "npats above PKT_SCAN_MAX_PATTERNS");
    if (n && !pats) return scan_refuse(err, "null patterns");
    if (nbytes && !bytes) return scan_refuse(err, "null bytes");
    uint64_t total = 0;
    uint32_t max_len = 0;
    for (uint32_t i = 0; i < n; i++) {
        const pkt_scan_pattern_t& p = pats[i];
        const auto bad = [&](const char* what) { return scan_refuse(err, "pattern " + std::to_string(i) + ": " + what); };
        if (p.len == 0 || p.len > PKT_SCAN_MAX_LEN) return bad("len is not in 1..PKT_SCAN_MAX_LEN");
        if ((uint64_t)p.off + p.len > nbytes) return bad("off + len > nbytes");
        if (p.flags & ~PKT_SCAN_NOCASE) return bad("unknown flag bits");
        if (p.group > 63) return bad("group above 63");
        if (p.reserved) return bad("non-zero reserved");
        total += p.len;
        max_len = p.len > max_len ? p.len : max_len;
    }
    if (total > PKT_SCAN_MAX_BYTES) return scan_refuse(err, "the patterns' lengths sum to more than PKT_SCAN_MAX_BYTES");
    // ---- the two tries: states 0 and 1 are the roots, an edge is (parent << 8 | byte) -> child
    std::unordered_map<uint32_t, uint32_t> edge;
    edge.reserve((size_t)total * 2 + 16);
    std::vector<uint32_t> end_state(n);
    uint32_t nstates = 2;
    for (uint32_t i = 0; i < n; i++) {
        const pkt_scan_pattern_t& p = pats[i];
        const bool fold = p.flags & PKT_SCAN_NOCASE;
        uint32_t st = fold ? 1u : 0u;
        for (uint32_t k = 0; k < p.len; k++) {
            const uint32_t c = fold ? scan_fold(bytes[p.off + k]) : bytes[p.off + k];
            const auto ins = edge.emplace(st << 8 | c, nstates);
            if (ins.second) nstates++;
            st = ins.first->second;
        }
        end_state[i] = st;
    }
    const uint32_t deep_edges = [&] {
        uint32_t k = 0;
        for (const auto& e : edge) k += (e.first >> 8) >= 2u;
        return k;
    }();
    uint32_t slots = 2;
    while (slots < 2u * deep_edges) slots <<= 1;
    img.slots = slots;
    img.out_at_w = 2u * slots;
    img.out_pat_w = img.out_at_w + nstates + 1u;
    img.group_w = img.out_pat_w + n;
    img.deep_words = (img.group_w + n + 1u) & ~1u;
    img.action_at = (uint64_t)kScanFirstWords + img.deep_words;
    img.fits_lds = (uint64_t)img.deep_words + n + 1u <= kScanLdsWords;
    img.info = pkt_scan_info_t{n, nstates, max_len, PKT_SCAN_PLACE_GLOBAL, 4ull * (img.action_at + n)};
    img.words.assign(img.action_at + n, 0u);
    uint32_t* const root = img.words.data();
    uint32_t* const two = root + 512;
    uint32_t* const deep = root + kScanFirstWords;
    uint32_t* const out_at = deep + img.out_at_w;
    uint32_t* const out_pat = deep + img.out_pat_w;
    // the patterns a state ends, ascending: a counting sort by state, stable over the pattern index
    std::vector<uint8_t> has_out(nstates, 0);
    for (uint32_t i = 0; i < n; i++) {
        out_at[end_state[i] + 1u]++;
        has_out[end_state[i]] = 1;
    }
    for (uint32_t s = 0; s < nstates; s++) out_at[s + 1u] += out_at[s];
    {
        std::vector<uint32_t> at(out_at, out_at + nstates);
        for (uint32_t i = 0; i < n; i++) out_pat[at[end_state[i]]++] = i;
    }
    for (uint32_t i = 0; i < n; i++) {
        const pkt_scan_pattern_t& p = pats[i];
        deep[img.group_w + i] = p.group;
        img.words[img.action_at + i] = p.action;
        if (p.len >= 2) {
            const uint32_t b = scan_fold(bytes[p.off]) << 8 | scan_fold(bytes[p.off + 1]);
            two[b >> 5] |= 1u << (b & 31u);
        }
    }
    ScanSlot* const tab = reinterpret_cast<ScanSlot*>(deep);
    for (uint32_t h = 0; h < slots; h++) tab[h] = ScanSlot{kScanEmpty, 0u};
    uint32_t lg = 0;
    while ((1u << lg) < slots) lg++;
    for (const auto& e : edge) {
        const uint32_t parent = e.first >> 8, c = e.first & 0xFFu, val = e.second | (has_out[e.second] ? kScanOut : 0u);
        if (parent < 2u) {
            root[256u * parent + c] = val;
            continue;
        }
        uint32_t h = scan_hash(e.first, 32u - lg);
        while (tab[h].key != kScanEmpty) h = (h + 1u) & (slots - 1u);
        tab[h] = ScanSlot{e.first, val};
    }
    return PKT_SUCCESS;
}

struct pkt_scan;
struct ScanDevOps {
    int (*run)(pkt_scan* s, const ScanCall& c, void* stream);
    int (*destroy)(pkt_scan* s);
};

struct pkt_scan {
    const ScanDevOps* ops = nullptr;  // NULL: a host handle
    ScanView view{};
    pkt_scan_info_t info{};
    std::vector<uint32_t> host_words;  // host handle: the image
    std::string err;
    // device handle
    int device = 0;
    uint32_t* dev_words = nullptr;
};

inline int scan_fail(pkt_scan* s, const char* msg) {
    if (s) s->err = msg;
    return PKT_ERR_INVALID_ARG;
}

// pkt_scan_batch's refusals, for both kinds of handle (the text, or nullptr); `device`: the slab's alignment counts.
inline const char* scan_batch_error(const pkt_batch_t* b, const pkt_chain_t* chain, uint32_t region, const uint64_t* matched,
                                    const uint64_t* hits, bool device) {
    if (!b) return "pkt_scan_batch: null batch";
    if (region != PKT_SCAN_PACKET && region != PKT_SCAN_PAYLOAD) return "pkt_scan_batch: unknown region";
    if (region == PKT_SCAN_PAYLOAD && !chain) return "pkt_scan_batch: null chain with PKT_SCAN_PAYLOAD";
    if (b->n >= (1ull << 32)) return "pkt_scan_batch: n >= 2^32";
    if (((uintptr_t)matched | (uintptr_t)hits) & 7) return "pkt_scan_batch: matched / hits not 8-byte aligned";
    if (b->n == 0) return nullptr;
    if (region == PKT_SCAN_PAYLOAD && (!chain->n_hdrs || !chain->hdr_type || !chain->hdr_off))
        return "pkt_scan_batch: null chain column";
    if (batch_null_slab(b)) return "pkt_scan_batch: null slab";
    if (device && ((uintptr_t)b->slab & 15)) return "pkt_scan_batch: slab not 16-byte aligned";
    if (b->offsets && !b->lens) return "pkt_scan_batch: offsets without lens";
    if (!b->offsets && b->stride == 0) return "pkt_scan_batch: stride 0";
    return nullptr;
}

// A host handle's call: a sequential loop over the packets and their start positions, reading exactly the region's
// bytes.
inline void scan_host_run(const ScanView& v, const ScanCall& c) {
    const ScanTabs t = scan_tabs(v.first, v.deep, v);
    const uint32_t* group = v.deep + v.group_w;
    for (uint64_t i = 0; i < c.n; i++) {
        uint32_t st = PKT_SCAN_SKIPPED, r0 = 0, r1 = 0, count = 0;
        uint64_t off = 0, best = kScanNoBest, matched = 0;
        if (!c.select || c.select[i]) {
            off = pkt_off(c.src, i);
            r1 = pkt_len(c.src, i, off);
            st = PKT_SCAN_MISS;
            if (c.region == PKT_SCAN_PAYLOAD) {
                ScanRegion r;
                const uint32_t n_hdrs = c.n_hdrs[i], nh = n_hdrs > PKT_MAX_HDRS ? PKT_MAX_HDRS : n_hdrs;
                for (uint32_t j = 0; j < nh; j++) scan_region_step(r, c.hdr_type[j * c.n + i], c.hdr_off[j * c.n + i]);
                st = scan_region_status(r, n_hdrs, r1);
                r0 = r.r0;
            }
        }
        if (st == PKT_SCAN_MISS) {
            for (uint32_t s = r0; s < r1; s++) {
                const auto emit = [&](uint32_t p) {
                    count++;
                    const uint64_t key = (uint64_t)p << 16 | s;
                    best = key < best ? key : best;
                    matched |= 1ull << group[p];
                    if (c.hits) c.hits[p]++;
                };
                scan_start(t, c.src.slab + off + s, r1 - s, emit);
            }
            if (c.hits && count == 0) c.hits[v.npats]++;
        }
        scan_store(c, i, scan_result(st, count, best, matched, v));
    }
}
