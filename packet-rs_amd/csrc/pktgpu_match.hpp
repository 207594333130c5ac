// pktgpu_match.hpp — what pkt_match_create (pktgpu_match.hip) and pkt_match_host (pktgpu_host.cpp) share: the
// program's refusal rules with their texts, and the compiled form the kernel reads.  Host code only; compiles
// without a HIP compiler.
#pragma once
#include <cstdint>
#include <cstring>

#include "pktgpu_batch.hpp"

// What is wrong with a match program, as the refusal's text, or nullptr.
inline const char* match_program_error(const pkt_match_term_t* terms, uint32_t nterms, const pkt_match_rule_t* rules,
                                       uint32_t nrules) {
    if (nrules > PKT_MATCH_MAX_RULES) return "pkt_match: more than 64 rules";
    if (nterms > PKT_MATCH_MAX_TERMS) return "pkt_match: more than 256 terms";
    if ((nterms && !terms) || (nrules && !rules)) return "pkt_match: null terms or rules with a non-zero count";
    for (uint32_t r = 0; r < nrules; r++)
        if ((uint32_t)rules[r].first_term + rules[r].nterms > nterms) return "pkt_match: a rule's terms run past nterms";
    for (uint32_t t = 0; t < nterms; t++) {
        const pkt_match_term_t& m = terms[t];
        const pkt_field_spec_t& f = m.field;
        if (m.op > PKT_MATCH_LEN) return "pkt_match: unknown op";
        if (m.flags & ~PKT_MATCH_NOT) return "pkt_match: unknown flag bits";
        if (m.reserved || m.reserved2 || f.reserved) return "pkt_match: non-zero reserved field";
        if (m.op == PKT_MATCH_LEN) {
            if (f.hdr_type || f.occurrence || f.start || f.end) return "pkt_match: a LEN term with a non-zero field";
            continue;
        }
        if (f.hdr_type == 0 || f.hdr_type >= PKT_HDR_COUNT) return "pkt_match: hdr_type outside 1..21";
        if (m.op == PKT_MATCH_HAS) continue;
        if (f.end < f.start || f.end >= 8u * kHdrSizes[f.hdr_type]) return "pkt_match: bits outside the header";
        if (f.end - f.start + 1u > 64u) return "pkt_match: a field wider than 64 bits";
    }
    return nullptr;
}

inline uint64_t match_width_mask(uint32_t width) { return width >= 64 ? ~0ull : (1ull << width) - 1; }

// ---- the compiled program (pkt_match_create): what the kernel stages in LDS
// A distinct (hdr_type, occurrence) of the program: resolved once per packet.
struct MatchRef {
    uint8_t type, occ, size, pad;
};
// A term: the field as a byte span of its header and a right shift; EQ's value and mask already cut to the
// field's width (a = value & mask, b = mask), so the kernel's test is ((v ^ a) & b) == 0.
struct MatchCTerm {     // 32 bytes
    uint64_t a, b;
    uint16_t ref;       // index into the refs (LEN: unused)
    uint16_t b0;        // first byte of the field within the header
    uint8_t op, neg;    // pkt_match_op_t; 1 = PKT_MATCH_NOT
    uint8_t nb, rsh;    // bytes the field touches (1..9); unused bits below it in its last byte
    uint32_t width;     // 1..64
    uint32_t pad;
};
static_assert(sizeof(MatchCTerm) == 32 && sizeof(MatchRef) == 4, "compiled match program layout");

struct MatchCompiled {
    MatchCTerm terms[PKT_MATCH_MAX_TERMS];
    pkt_match_rule_t rules[PKT_MATCH_MAX_RULES];
    MatchRef refs[PKT_MATCH_MAX_TERMS];
    uint32_t nterms, nrules, nrefs;
};

// Compile a validated program.  Each rule gets its own run of compiled terms (shared or overlapping source
// ranges are copied: at most 64 * 256 source terms, but the compiled table holds 256, so a program whose rules
// together reference more than 256 terms keeps the source layout instead, order untouched).  Within a run the
// terms are ordered LEN and HAS first (no field read), then by header reference, so that a rule that fails
// fails early and consecutive terms share their header.
inline void match_compile(const pkt_match_term_t* terms, uint32_t nterms, const pkt_match_rule_t* rules, uint32_t nrules,
                          MatchCompiled& c) {
    memset(&c, 0, sizeof c);
    auto ref_of = [&](const pkt_field_spec_t& f) -> uint16_t {
        for (uint32_t k = 0; k < c.nrefs; k++)
            if (c.refs[k].type == f.hdr_type && c.refs[k].occ == f.occurrence) return (uint16_t)k;
        c.refs[c.nrefs] = MatchRef{f.hdr_type, f.occurrence, kHdrSizes[f.hdr_type], 0};
        return (uint16_t)c.nrefs++;
    };
    auto compile_term = [&](const pkt_match_term_t& m) {
        MatchCTerm t{};
        t.op = m.op;
        t.neg = m.flags & PKT_MATCH_NOT ? 1 : 0;
        t.a = m.a;
        t.b = m.b;
        if (m.op == PKT_MATCH_LEN) return t;
        t.ref = ref_of(m.field);
        if (m.op == PKT_MATCH_HAS) return t;
        const uint32_t start = m.field.start, end = m.field.end;
        t.b0 = (uint16_t)(start >> 3);
        t.nb = (uint8_t)((end >> 3) - (start >> 3) + 1);
        t.rsh = (uint8_t)(7 - (end & 7));
        t.width = end - start + 1;
        if (m.op == PKT_MATCH_EQ) {
            t.b = m.b & match_width_mask(t.width);
            t.a = m.a & t.b;
        }
        return t;
    };
    uint32_t total = 0;
    for (uint32_t r = 0; r < nrules; r++) total += rules[r].nterms;
    c.nrules = nrules;
    if (total > PKT_MATCH_MAX_TERMS) {  // heavily shared terms: the source layout
        for (uint32_t t = 0; t < nterms; t++) c.terms[t] = compile_term(terms[t]);
        for (uint32_t r = 0; r < nrules; r++) c.rules[r] = rules[r];
        c.nterms = nterms;
        return;
    }
    uint32_t at = 0;
    for (uint32_t r = 0; r < nrules; r++) {
        const uint32_t first = at;
        for (uint32_t k = 0; k < rules[r].nterms; k++) c.terms[at++] = compile_term(terms[rules[r].first_term + k]);
        // insertion sort (stable) by (reads a field, header reference)
        auto key = [](const MatchCTerm& t) -> uint32_t {
            return (t.op == PKT_MATCH_LEN || t.op == PKT_MATCH_HAS) ? 0u : 1u + t.ref;
        };
        for (uint32_t i = first + 1; i < at; i++) {
            const MatchCTerm x = c.terms[i];
            uint32_t j = i;
            for (; j > first && key(c.terms[j - 1]) > key(x); j--) c.terms[j] = c.terms[j - 1];
            c.terms[j] = x;
        }
        c.rules[r].first_term = (uint16_t)first;
        c.rules[r].nterms = (uint16_t)(at - first);
        c.rules[r].action = rules[r].action;
    }
    c.nterms = at;
}
