// pktgpu_flow.hpp — what the two halves of the flow table share: the handle behind pkt_flow_table_t, an entry's
// layout, the hash and the tag rule.  pktgpu_host.cpp holds the public pkt_flow_table_* calls and the host table
// (a sequential loop, no device: it compiles under g++ alone); pktgpu_flow.hip holds pkt_flow_table_create and the
// device table's calls, which the handle reaches through `ops`.
#pragma once
#include <cstdint>
#include <string>

#include "pktgpu_batch.hpp"

// splitmix64 as include/pktgpu.h spells it out at PKT_GEN_RANDOM
PKT_HD uint64_t flow_mix64(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ z >> 27) * 0x94D049BB133111EBull;
    return z ^ z >> 31;
}

// the hash of a key's five little-endian words
PKT_HD uint64_t flow_hash(uint64_t seed, const uint64_t w[5]) {
    uint64_t h = seed;
    for (int k = 0; k < 5; k++) h = flow_mix64(h ^ w[k]);
    return h;
}

// a packet's tag (never 0: 0 is the empty entry) and where its probing starts
PKT_HD uint64_t flow_tag(uint64_t hash, uint32_t tag_bits) {
    const uint64_t t = tag_bits >= 64 ? hash : hash & ((1ull << tag_bits) - 1);
    return t ? t : 1;
}
PKT_HD uint64_t flow_home(uint64_t tag, uint64_t slots) { return flow_mix64(tag) & (slots - 1); }

// One entry: a 128-byte line.  tag 0 = empty (first = ~0, the rest 0).  The key is stored once, by the packet
// with the lowest base + i of the update that claimed the entry; every entry with a tag has one when that
// update is over.
struct alignas(128) FlowEntry {
    uint64_t tag;
    uint64_t first;
    uint64_t pkts[2];
    uint64_t bytes[2];
    uint64_t key[5];  // pkt_flow_key_t as it lies in memory (at byte 48: 16-byte aligned)
    uint64_t pad[5];
};
static_assert(sizeof(FlowEntry) == 128, "an entry is one 128-byte line");
static_assert(sizeof(pkt_flow_key_t) == 40 && sizeof(pkt_flow_record_t) == 80, "flow ABI structs");

constexpr uint32_t kFlowNone = 0xFFFFFFFFu;  // flow_id of a packet that is not UPD_OK
constexpr uint64_t kFlowMinSlots = 64, kFlowMaxSlots = 1ull << 28;

struct FlowUpdate {
    const pkt_flow_key_t* keys;
    const uint64_t* hash;
    const uint8_t* dir;
    const uint32_t* weight;
    const uint8_t* status;
    uint64_t n, base;
    uint32_t* flow_id;
    uint8_t* upd_status;
};

// the device table's calls (pktgpu_flow.hip); every refusal that needs no device is made before them
struct FlowDevOps {
    int (*update)(pkt_flow_table* t, const FlowUpdate& u, void* stream);
    int (*scan)(pkt_flow_table* t, pkt_flow_record_t* records, uint64_t cap, uint64_t* n_out, void* stream);
    int (*clear)(pkt_flow_table* t, void* stream);
    int (*destroy)(pkt_flow_table* t);
};

struct pkt_flow_table {
    const FlowDevOps* ops = nullptr;  // NULL: a host table
    uint64_t slots = 0;
    uint32_t tag_bits = 64;
    uint64_t hwm = 0;      // the last update's base + n
    bool touched = false;  // an update since create / clear (set_tag_bits is refused then)
    FlowEntry* e = nullptr;
    std::string err;
    // device table
    int device = 0;
    uint32_t* slot_scratch = nullptr;  // [kFlowChunk]: the packets' entries when the caller gives no flow_id
    uint32_t* tile_cnt = nullptr;      // [slots / kFlowTile]: entries per tile, then their exclusive prefix
    uint64_t* total = nullptr;         // pinned host word: the entry count
    uint64_t* total_dev = nullptr;     // the same word as the device addresses it
};

inline int flow_fail(pkt_flow_table* t, int code, const char* msg) {
    if (t) t->err = msg;
    return code;
}
