// pktgpu_meter.hpp — what the two halves of pkt_meter_* share: the handle behind pkt_meter_t, the packed configuration,
// the refill and the decision of one packet in 64-bit words (meter_packet), the DSCP stores (meter_remark), the
// per-packet outputs (meter_emit), the create validation and the argument refusals.  pktgpu_host.cpp holds the public
// pkt_meter_* calls and the host handle, which IS the sequential model of include/pktgpu.h (it compiles under g++
// alone); pktgpu_meter.hip holds pkt_meter_create and the device handle's calls, which the handle reaches through
// `ops`.  Both call the same inline code, so the CPU tests cover the arithmetic.
//
// The model is in unbounded integers; these are the 64-bit words that give its answer for every admissible input:
//   buckets  c <= ccap = cbs * 10^9 and x <= xcap = xbs * 10^9 always, both below 2^26 * 10^9 < 2^56.
//   cost     B = max(0, len + adjust) * 10^9 <= (65535 + 2^31) * 10^9 < 2^62: no clamp is needed, it is compared with a
//            bucket and subtracted only where it is not above it.
//   refill   the model's min(cap, level + rate * dt) only needs min(room, rate * dt), room = cap - level < 2^57
//            (meter_gain): the product's upper 64 bits say whether it is above every room, so no dt (2^64 - 1
//            included) and no rate overflows, and rate 0 gains 0.  srTCM's spill is the same with room = both rooms.
//   counters uint64: 2^32 packets of 65535 bytes a call.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "pktgpu_batch.hpp"
#include "pktgpu_fwd.hpp"

static_assert(sizeof(pkt_meter_cfg_t) == 32 && sizeof(pkt_meter_state_t) == 72, "meter ABI structs");

constexpr uint32_t kMeterFlags = PKT_METER_MARK;
constexpr uint64_t kMeterUnit = 1000000000ull;  // bucket units per byte

// A meter's rates and caps as the walk reads them, and beside it one word: bit 0 = trTCM, bit 1 = colour-aware,
// bits 2 + 2c = action[c], bits 8 + 6c = dscp[c].
struct MeterCfg {
    uint64_t cir, pir, ccap, xcap;
};
PKT_HD uint32_t meter_word_action(uint32_t w, uint32_t col) { return w >> (2u + 2u * col) & 3u; }
PKT_HD uint32_t meter_word_dscp(uint32_t w, uint32_t col) { return w >> (8u + 6u * col) & 63u; }

inline uint32_t meter_word(const pkt_meter_cfg_t& g) {
    uint32_t w = (g.mode == PKT_METER_TRTCM ? 1u : 0u) | (g.flags & PKT_METER_F_COLOR_AWARE ? 2u : 0u);
    for (uint32_t c = 0; c < 3; c++) w |= (uint32_t)g.action[c] << (2u + 2u * c) | (uint32_t)g.dscp[c] << (8u + 6u * c);
    return w;
}

// What the kernels and the host loop read and write: device pointers for a device handle, host pointers for a host one.
struct MeterView {
    const MeterCfg* cfg;    // [nmeters]
    const uint32_t* word;   // [nmeters]
    pkt_meter_state_t* st;  // [nmeters]
    uint32_t nmeters;
    int32_t adjust;
};

// min(room, rate * dt), exact
PKT_HD uint64_t meter_gain(uint64_t rate, uint64_t dt, uint64_t room) {
#ifdef __HIP_DEVICE_COMPILE__
    const uint64_t hi = __umul64hi(rate, dt);
#else
    const uint64_t hi = (uint64_t)(((unsigned __int128)rate * dt) >> 64);
#endif
    const uint64_t lo = rate * dt;
    return hi || lo > room ? room : lo;
}

PKT_HD uint64_t meter_cost(uint32_t len, int32_t adjust) {
    const int64_t v = (int64_t)len + adjust;
    return v < 0 ? 0ull : (uint64_t)v * kMeterUnit;
}

// steps 3 and 4 for one packet of meter (g, w): the state moves on, the colour comes back
struct MeterLive {
    uint64_t c, x, last;
};
// What dt adds, clamped where no state can tell the difference: a = min(cir * dt, ccap + xcap) under srTCM (enough to
// fill both buckets from empty) and min(cir * dt, ccap) under trTCM; gx = min(pir * dt, xcap) under trTCM, else 0.  The
// gains depend on the times alone, so a wave works out 64 of them at once.
PKT_HD void meter_gains(const MeterCfg& g, bool tr, uint64_t dt, uint64_t& a, uint64_t& gx) {
    a = meter_gain(g.cir, dt, tr ? g.ccap : g.ccap + g.xcap);
    gx = tr ? meter_gain(g.pir, dt, g.xcap) : 0ull;
}
PKT_HD void meter_refill(MeterLive& s, const MeterCfg& g, bool tr, uint64_t a, uint64_t gx) {
    const uint64_t up = s.c + a, c2 = up < g.ccap ? up : g.ccap;  // below 2^58
    const uint64_t xu = s.x + (tr ? gx : up - c2);
    s.c = c2;
    s.x = xu < g.xcap ? xu : g.xcap;
}
PKT_HD uint32_t meter_decide(MeterLive& s, bool tr, uint32_t ic, uint64_t B);

PKT_HD uint32_t meter_packet(MeterLive& s, const MeterCfg& g, uint32_t w, uint64_t t, uint64_t B, uint32_t ic) {
    const bool tr = w & 1u;
    if (t > s.last) {
        uint64_t a, gx;
        meter_gains(g, tr, t - s.last, a, gx);
        s.last = t;
        meter_refill(s, g, tr, a, gx);
    }
    return meter_decide(s, tr, ic, B);
}

PKT_HD uint32_t meter_decide(MeterLive& s, bool tr, uint32_t ic, uint64_t B) {
    ic = ic > PKT_METER_RED ? PKT_METER_RED : ic;
    if (tr) {
        if (ic == PKT_METER_RED || s.x < B) return PKT_METER_RED;
        s.x -= B;
        if (ic == PKT_METER_YELLOW || s.c < B) return PKT_METER_YELLOW;
        s.c -= B;
        return PKT_METER_GREEN;
    }
    if (ic == PKT_METER_GREEN && s.c >= B) {
        s.c -= B;
        return PKT_METER_GREEN;
    }
    if (ic <= PKT_METER_YELLOW && s.x >= B) {
        s.x -= B;
        return PKT_METER_YELLOW;
    }
    return PKT_METER_RED;
}

// a run's owner: the meter's state in registers, loaded once and stored once
struct MeterRun {
    MeterLive s;
    uint64_t pk[3], by[3];
};
PKT_HD MeterRun meter_run_load(const pkt_meter_state_t& st) {
    return MeterRun{{st.c, st.x, st.last}, {st.packets[0], st.packets[1], st.packets[2]}, {st.bytes[0], st.bytes[1], st.bytes[2]}};
}
PKT_HD void meter_run_store(pkt_meter_state_t& st, const MeterRun& r) {
    st.c = r.s.c, st.x = r.s.x, st.last = r.s.last;
    for (uint32_t q = 0; q < 3; q++) st.packets[q] = r.pk[q], st.bytes[q] = r.by[q];
}
PKT_HD void meter_run_count(MeterRun& r, uint32_t col, uint32_t len) {
    for (uint32_t q = 0; q < 3; q++) {  // (no dynamic index: the arrays stay in registers)
        r.pk[q] += col == q ? 1u : 0u;
        r.by[q] += col == q ? len : 0u;
    }
}
PKT_HD uint32_t meter_run_packet(MeterRun& r, const MeterCfg& g, uint32_t w, uint64_t t, uint64_t B, uint32_t ic, uint32_t len) {
    const uint32_t col = meter_packet(r.s, g, w, t, B, ic);
    meter_run_count(r, col, len);
    return col;
}

// ---- step 6.  ip: the header's first byte; byte stores, so any alignment
PKT_HD void meter_remark(uint8_t* ip, bool v4, uint32_t dscp) {
    const uint32_t b0 = ip[0], b1 = ip[1];
    if (v4) {
        const uint32_t n1 = dscp << 2 | (b1 & 3u), m = b0 << 8 | b1, m2 = b0 << 8 | n1;
        const uint32_t hc = (uint32_t)ip[10] << 8 | ip[11];
        uint32_t s = (~hc & 0xFFFFu) + (~m & 0xFFFFu) + m2;  // RFC 1624 eq. 3
        s = (s & 0xFFFFu) + (s >> 16);
        s = (s & 0xFFFFu) + (s >> 16);
        s = ~s & 0xFFFFu;
        ip[1] = (uint8_t)n1;
        ip[10] = (uint8_t)(s >> 8), ip[11] = (uint8_t)s;
    } else {
        ip[0] = (uint8_t)((b0 & 0xF0u) | dscp >> 2);
        ip[1] = (uint8_t)((b1 & 0x3Fu) | (dscp & 3u) << 6);
    }
}

// one call of pkt_meter_batch, as the handle's halves take it
struct MeterCall {
    BatchSrc src;
    uint64_t n;
    const uint8_t* n_hdrs;  // the chain's columns, NULL without PKT_METER_MARK
    const uint8_t* hdr_type;
    const uint16_t* hdr_off;
    uint32_t which, flags, meter_all;
    const uint32_t* meter;
    uint64_t now;
    const uint64_t* time;
    const uint8_t* in_color;
    const uint8_t* select;
    uint8_t* color;
    uint8_t* pass;
    uint8_t* marked;
    uint64_t* hits;
    uint64_t* bytes;
};

// step 1: the packet's meter, or ~0u for an unmetered packet
PKT_HD uint32_t meter_of(const MeterCall& c, uint32_t nmeters, uint64_t i) {
    if (c.select && !c.select[i]) return ~0u;
    const uint32_t k = c.meter ? c.meter[i] : c.meter_all;
    return k < nmeters ? k : ~0u;
}
PKT_HD uint32_t meter_in_color(const MeterCall& c, uint32_t w, uint64_t i) {
    return c.in_color && (w & 2u) ? c.in_color[i] : (uint32_t)PKT_METER_GREEN;
}

// steps 5 and 6 for packet i: w = its meter's word (unused for PKT_METER_UNMETERED), off / len = where it lies
PKT_HD void meter_emit(const MeterCall& c, uint64_t i, uint32_t col, uint32_t w, uint64_t off, uint32_t len) {
    const uint32_t act = col == PKT_METER_UNMETERED ? (uint32_t)PKT_METER_PASS : meter_word_action(w, col);
    uint32_t marked = 0;
    if ((c.flags & PKT_METER_MARK) && act == PKT_METER_REMARK) {
        uint32_t nh = c.n_hdrs[i];
        nh = nh > PKT_MAX_HDRS ? PKT_MAX_HDRS : nh;
        FwdFind f;
        for (uint32_t j = 0; j < nh; j++)
            fwd_find_step(f, c.which, c.hdr_type[(uint64_t)j * c.n + i], c.hdr_off[(uint64_t)j * c.n + i]);
        if (f.ipt && f.ipo + (f.ipt == PKT_HDR_IPV4 ? 20u : 40u) <= len) {
            meter_remark(const_cast<uint8_t*>(c.src.slab) + off + f.ipo, f.ipt == PKT_HDR_IPV4, meter_word_dscp(w, col));
            marked = 1;
        }
    }
    if (c.color) c.color[i] = (uint8_t)col;
    if (c.pass) c.pass[i] = act != PKT_METER_DROP;
    if (c.marked) c.marked[i] = (uint8_t)marked;
}

// ---- create: nullptr, or the refusal's text (after "pkt_meter_create: " / "pkt_meter_create_host: ")
inline const char* meter_create_error(const pkt_meter_cfg_t* cfg, uint32_t nmeters) {
    if (nmeters < 1 || nmeters > PKT_METER_MAX_METERS) return "nmeters not in 1..2^24";
    if (!cfg) return "null cfg";
    for (uint32_t k = 0; k < nmeters; k++) {
        const pkt_meter_cfg_t& g = cfg[k];
        if (g.cir > PKT_METER_MAX_RATE || g.pir > PKT_METER_MAX_RATE) return "a rate above 2^40 bytes per second";
        if (g.cbs > PKT_METER_MAX_BURST || g.xbs > PKT_METER_MAX_BURST) return "a burst above 2^26 bytes";
        if (g.mode > PKT_METER_TRTCM) return "a mode that is neither PKT_METER_SRTCM nor PKT_METER_TRTCM";
        if (g.flags & ~PKT_METER_F_COLOR_AWARE) return "unknown cfg flag bits";
        for (uint32_t c = 0; c < 3; c++) {
            if (g.action[c] > PKT_METER_REMARK) return "an action above PKT_METER_REMARK";
            if (g.dscp[c] > 63) return "a dscp above 63";
        }
    }
    return nullptr;
}

inline void meter_pack(const pkt_meter_cfg_t* cfg, uint32_t nmeters, std::vector<MeterCfg>& out, std::vector<uint32_t>& word) {
    out.resize(nmeters);
    word.resize(nmeters);
    for (uint32_t k = 0; k < nmeters; k++) {
        out[k] = MeterCfg{cfg[k].cir, cfg[k].pir, cfg[k].cbs * kMeterUnit, cfg[k].xbs * kMeterUnit};
        word[k] = meter_word(cfg[k]);
    }
}

PKT_HD void meter_state_reset(pkt_meter_state_t& st, const MeterCfg& g) {
    st.c = g.ccap, st.x = g.xcap, st.last = 0;
    for (uint32_t q = 0; q < 3; q++) st.packets[q] = st.bytes[q] = 0;
}

// the refusals of pkt_meter_batch on both handles: the text after "pkt_meter_batch: ", or nullptr.  n == 0 is the
// caller's to take between the two.
inline const char* meter_call_error(const pkt_batch_t* b, const pkt_chain_t* chain, uint32_t which_ip, uint32_t flags,
                                    const uint32_t* meter, const uint64_t* time_ns, const uint64_t* hits, const uint64_t* bytes) {
    if (!b) return "null argument";
    if (b->n >= (1ull << 32)) return "n >= 2^32";
    if (flags & ~kMeterFlags) return "unknown flag bits";
    if (flags & PKT_METER_MARK) {
        if (!chain) return "PKT_METER_MARK with a null chain";
        if (which_ip >= PKT_MAX_HDRS && which_ip != PKT_FLOW_LAST) return "which_ip is neither below 16 nor PKT_FLOW_LAST";
    }
    if (((uintptr_t)hits | (uintptr_t)bytes | (uintptr_t)time_ns) & 7) return "hits / bytes / time_ns not 8-byte aligned";
    if ((uintptr_t)meter & 3) return "meter not 4-byte aligned";
    return nullptr;
}
inline const char* meter_batch_error(const pkt_batch_t* b, const pkt_chain_t* chain, uint32_t flags, bool device) {
    if ((flags & PKT_METER_MARK) && (!chain->n_hdrs || !chain->hdr_type || !chain->hdr_off)) return "null chain column";
    const char* msg = device ? batch_slab16_error(b) : batch_null_slab(b) ? "null slab" : nullptr;
    return msg ? msg : batch_index_error(b);
}

struct pkt_meter;
// the device handle's calls (pktgpu_meter.hip); every refusal that needs no device is made before them
struct MeterDevOps {
    int (*batch)(pkt_meter* t, const MeterCall& c, void* stream);
    int (*reset)(pkt_meter* t, void* stream);
    int (*xport)(pkt_meter* t, uint32_t first, uint32_t count, pkt_meter_state_t* out);
    int (*destroy)(pkt_meter* t);
    void (*refused)(pkt_meter* t);  // t->err also goes to the ctx
};

struct pkt_meter {
    const MeterDevOps* ops = nullptr;  // NULL: a host handle
    MeterView v{};
    std::string err;
    // the packed configuration (the host handle's `v` points into it) and the host handle's state
    std::vector<MeterCfg> h_cfg;
    std::vector<uint32_t> h_word;
    std::vector<pkt_meter_state_t> h_st;
    // device handle
    void* ctx = nullptr;  // pkt_ctx
    int device = 0;
    void* dev_buf = nullptr;       // one allocation behind `v` and the scratch of a chunk of 2^20 packets
    uint32_t* key[2] = {nullptr, nullptr};  // [chunk] x 2: the metered packets' meters, ping and pong of the radix passes
    uint32_t* idx[2] = {nullptr, nullptr};  // [chunk] x 2: their indexes in the chunk, beside the keys
    uint32_t* cnt = nullptr;       // [256][tiles]: a pass's digit counts per tile, then their exclusive prefix
    uint32_t* ctl = nullptr;       // [4]: the chunk's metered packets
    uint8_t* col = nullptr;        // [chunk]: the metered packets' colours
    uint32_t bits = 0;             // of a meter id
};

inline int meter_fail(pkt_meter* t, const char* where, const char* msg) {
    if (t) {
        t->err = std::string(where) + ": " + msg;
        if (t->ops) t->ops->refused(t);
    }
    return PKT_ERR_INVALID_ARG;
}
