// pktgpu_edit.hip — pkt_edit_batch: Packet::push / insert / pop / remove (packet.rs:117-164) on every
// packet's header list, then to_vec (385-392) of the result, in one launch:
//   phase 1   a wave owns 64 consecutive packets.  Lane p reads packet p's chain row (coalesced, slot-major
//             columns) into its column of an LDS list (one word per entry: source offset, type, size, and
//             whether the bytes are the packet's or hdr_data's), runs the op program on it (<= 8 ops, the
//             same for every packet: a uniform loop whose body shifts the lane's own column), writes the
//             status, the length and the out chain columns, and turns the list into a segment table in
//             place: (source offset, destination end), adjacent ranges of one source merged.  A VLAN
//             strip is [0,14) + [18,len), a decap one segment, an encap the constant bytes and one segment.
//   phase 2   the wave walks the FLATTENED aligned 16-byte destination chunks of its 64 packets, 64 chunks
//             per step and kEdQ steps' loads in flight, as pktgpu_compare.hip walks its pairs: a lane finds
//             its (packet, chunk) in the prefix of the chunk counts, assembles the chunk in registers from
//             at most two aligned 16-byte loads per contributing segment (the first two segments' loads of
//             every step are issued before the first is used; a chunk with more takes the rest in a loop)
//             and stores it whole when it lies inside the packet, else (a packet's first and last chunk)
//             as dwords, halves and bytes.  A 65535-byte packet among 64-byte ones costs its bytes.
// hdr_data travels in the kernel arguments and is copied to LDS by every block; dst is never read.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "pktgpu_ctx.hpp"

namespace {

constexpr uint32_t kEdBlock = 256;
constexpr uint32_t kEdWaves = kEdBlock / 64;
constexpr uint32_t kEdQ = 2;                      // steps of 64 chunks whose loads are issued before the first use
constexpr uint32_t kEdMaxOps = 8;
constexpr uint32_t kEdData = 320;                 // bytes of hdr_data
constexpr uint32_t kEdRows = PKT_MAX_HDRS + 1;    // list: 16 entries and the 17th that makes DEPTH; segments: 16 and the payload
constexpr uint32_t kEdConst = (16 + kEdData + 32) / 16;  // hdr_data in LDS: 16 bytes in front, 32 behind (uint4)
constexpr uint32_t kKonst = 0x80000000u;          // entry / segment: the bytes are hdr_data's

__constant__ uint8_t kEdHdrSize[PKT_HDR_COUNT] = PKT_HDR_SIZE_LIST;

struct EParams {
    BatchSrc src;
    uint64_t n;  // < 2^32
    const uint8_t* status;
    const uint8_t* n_hdrs;
    const uint8_t* hdr_type;   // [PKT_MAX_HDRS][n]
    const uint16_t* hdr_off;   // [PKT_MAX_HDRS][n]
    const uint16_t* payload_off;
    const uint16_t* payload_len;
    const uint8_t* select;
    uint8_t* dst;
    uint64_t dst_len;
    const uint64_t* dst_offsets;
    uint32_t* out_len;
    uint8_t* edit_status;
    uint8_t* o_status;
    uint8_t* o_n_hdrs;
    uint8_t* o_hdr_type;
    uint16_t* o_hdr_off;
    uint16_t* o_payload_off;
    uint16_t* o_payload_len;
    uint32_t* o_hdr_mask;
    uint32_t slot, nops;
    pkt_edit_op_t ops[kEdMaxOps];
    uint32_t data[kEdData / 4];
};

// ones in bytes [0, k) of a dword, k in 0..4
__device__ __forceinline__ uint32_t dword_bytes_below(uint32_t k) { return k >= 4u ? ~0u : (1u << (8u * k)) - 1u; }

// the part of the chunk's byte range [l, h) (0 <= l <= h <= 16) inside dword d, as dword-relative [lo, hi)
__device__ __forceinline__ void dword_range(uint32_t l, uint32_t h, uint32_t d, uint32_t& lo, uint32_t& hi) {
    const uint32_t b = 4u * d;
    lo = l > b ? (l - b > 4u ? 4u : l - b) : 0u;
    hi = h > b ? (h - b > 4u ? 4u : h - b) : 0u;
}

// One segment's share of a chunk: the two aligned source chunks, the shift between them and the chunk's
// byte range [ml, mh) the segment fills (ml >= mh: none).
struct Piece {
    uint4 v0, v1;
    uint32_t sh, ml, mh;
};

struct Wave {
    const uint32_t* sega;   // [kEdRows][64] source offset | kKonst
    const uint16_t* segb;   // [kEdRows][64] destination end, packet-relative (a segment starts where the one before ends)
    const uint64_t* src;    // [64] the packets' slab offsets
    const uint4* konst;     // hdr_data at byte 16
};

// Segment s of packet p against the chunk whose byte 0 is packet-relative destination byte c0 (may be
// negative in the packet's first chunk) and which holds the packet's bytes [lo, hi).  Every load holds
// a byte the segment names: inside the packet, so inside the slab rounded up to 16.
__device__ __forceinline__ Piece fetch(const Wave& w, const uint8_t* slab, uint32_t p, uint32_t s, uint32_t ns, int32_t c0,
                                       uint32_t lo, uint32_t hi) {
    Piece x;
    x.v0 = x.v1 = make_uint4(0, 0, 0, 0);
    x.sh = x.ml = x.mh = 0;
    if (s >= ns) return x;
    const uint32_t A = w.sega[s * 64u + p];
    const uint32_t ds = s ? w.segb[(s - 1u) * 64u + p] : 0u, de = w.segb[s * 64u + p];
    if (ds >= hi || de <= lo) return x;
    const uint32_t a = lo > ds ? lo : ds, b = hi < de ? hi : de;
    x.ml = (uint32_t)((int32_t)a - c0);
    x.mh = (uint32_t)((int32_t)b - c0);
    const int32_t rel = (int32_t)(A & 0xFFFFu) + c0 - (int32_t)ds;  // the source byte under the chunk's byte 0
    if (A & kKonst) {
        const uint32_t T = (uint32_t)(16 + rel);  // >= 1: rel >= -15
        x.sh = T & 15u;
        x.v0 = w.konst[T >> 4];
        x.v1 = w.konst[(T >> 4) + 1u];
    } else {
        const int64_t T = (int64_t)w.src[p] + rel;
        const int64_t T0 = T & ~(int64_t)15;
        x.sh = (uint32_t)T & 15u;
        if (x.sh + x.ml < 16u) x.v0 = *reinterpret_cast<const uint4*>(slab + T0);
        if (x.sh + x.mh > 16u) x.v1 = *reinterpret_cast<const uint4*>(slab + T0 + 16);
    }
    return x;
}

__device__ __forceinline__ void merge(const Piece& x, uint32_t out[4]) {
    if (x.ml >= x.mh) return;
    if (x.ml == 0 && x.mh == 16 && x.sh == 0) {  // the chunk is one aligned source chunk: most of a copy
        out[0] = x.v0.x, out[1] = x.v0.y, out[2] = x.v0.z, out[3] = x.v0.w;
        return;
    }
    uint32_t v[4];
    take16(x.v0, x.v1, x.sh, v);
    if (x.ml == 0 && x.mh == 16) {  // a whole chunk of one segment: no mask
#pragma unroll
        for (uint32_t d = 0; d < 4; d++) out[d] = v[d];
        return;
    }
#pragma unroll
    for (uint32_t d = 0; d < 4; d++) {
        uint32_t l, h;
        dword_range(x.ml, x.mh, d, l, h);
        out[d] |= v[d] & (dword_bytes_below(h) & ~dword_bytes_below(l));
    }
}

// bytes [l, h) of the aligned chunk at q: whole, or dwords, halves and bytes: each byte once, no other
__device__ __forceinline__ void put_chunk(uint8_t* q, const uint32_t out[4], uint32_t l, uint32_t h) {
    if (l == 0 && h == 16) {
        *reinterpret_cast<uint4*>(q) = make_uint4(out[0], out[1], out[2], out[3]);
        return;
    }
#pragma unroll
    for (uint32_t d = 0; d < 4; d++) {
        uint32_t a, b;
        dword_range(l, h, d, a, b);
        if (a >= b) continue;
        uint8_t* qd = q + 4u * d;
        const uint32_t v = out[d];
        if (a == 0 && b == 4) {
            *reinterpret_cast<uint32_t*>(qd) = v;
            continue;
        }
        if (a == 0 && b >= 2) *reinterpret_cast<uint16_t*>(qd) = (uint16_t)v;
        else if (a == 0 && b == 1) qd[0] = (uint8_t)v;
        else if (a == 1) qd[1] = (uint8_t)(v >> 8);
        if (a <= 2 && b == 4) *reinterpret_cast<uint16_t*>(qd + 2) = (uint16_t)(v >> 16);
        else if (a <= 2 && b == 3) qd[2] = (uint8_t)(v >> 16);
        else if (a == 3) qd[3] = (uint8_t)(v >> 24);
    }
}

__global__ __launch_bounds__(kEdBlock) void edit_kernel(EParams P) {
    __shared__ uint4 s_konst[kEdConst];
    __shared__ uint8_t s_size[32];                     // pkt_hdr_size by type: a lane's lookup stays in LDS
    __shared__ uint32_t s_la[kEdWaves][kEdRows * 64];  // the list, then the segments' sources
    __shared__ uint16_t s_lb[kEdWaves][kEdRows * 64];  // the segments' destination ends
    __shared__ uint32_t s_pre[kEdWaves][65];           // exclusive prefix of the packets' chunk counts
    __shared__ uint64_t s_src[kEdWaves][64], s_dst[kEdWaves][64];
    __shared__ uint32_t s_tot[kEdWaves][64];           // new length | segments << 16
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t i = (uint64_t)blockIdx.x * kEdBlock + threadIdx.x;
    const bool in = i < P.n;
    if (threadIdx.x < kEdConst * 4u) {
        const uint32_t t = threadIdx.x;
        reinterpret_cast<uint32_t*>(s_konst)[t] = t >= 4u && t < 4u + kEdData / 4u ? P.data[t - 4u] : 0u;
    }
    if (threadIdx.x >= 128u && threadIdx.x < 160u)
        s_size[threadIdx.x - 128u] = threadIdx.x - 128u < PKT_HDR_COUNT ? kEdHdrSize[threadIdx.x - 128u] : 0;
    __syncthreads();                 // hdr_data is in LDS; from here a wave shares nothing with the others
    uint32_t* la = s_la[wv] + lane;  // entry k of this lane's packet: la[64 k]
    uint16_t* lb = s_lb[wv] + lane;

    // ---- phase 1: the packet, its list, the program
    uint64_t off = 0, o = 0;
    uint32_t len = 0, room = 0, cnt = 0, st = PKT_EDIT_SKIPPED, src_status = 0, pay_at = 0, pay_len = 0;
    uint32_t hb = 0;  // the list's bytes
    bool run = false;
    if (in) {
        off = pkt_off(P.src, i);
        len = pkt_len(P.src, i, off);
        o = P.dst_offsets ? P.dst_offsets[i] : i * P.slot;
        const uint64_t dl = o < P.dst_len ? P.dst_len - o : 0;
        room = dl < P.slot ? (uint32_t)dl : P.slot;
        src_status = P.status[i];
        // n_hdrs and the first four slot rows with the loads above and below, whatever n_hdrs is: one round trip
        // for the common chains; later rows only where a chain has them
        const ChainPre cp = chain_load(P, i);
        uint32_t nh = cp.nh;
        const uint32_t po = P.payload_off[i], pl = P.payload_len[i];
        run = P.select ? P.select[i] != 0 : true;
        if (src_status == PKT_OK) {
            st = PKT_EDIT_OK;
            nh = nh > PKT_MAX_HDRS ? PKT_MAX_HDRS : nh;
            for (uint32_t j = 0; j < nh; j++) {
                uint32_t ty, ho;
                if (j < 4) {
                    ty = j == 0 ? cp.ty[0] : j == 1 ? cp.ty[1] : j == 2 ? cp.ty[2] : cp.ty[3];
                    ho = j == 0 ? cp.of[0] : j == 1 ? cp.of[1] : j == 2 ? cp.of[2] : cp.of[3];
                } else {
                    ty = P.hdr_type[(uint64_t)j * P.n + i];
                    ho = P.hdr_off[(uint64_t)j * P.n + i];
                }
                const uint32_t sz = ty < PKT_HDR_COUNT ? s_size[ty] : 0u;
                const uint32_t a = ho > len ? len : ho;
                const uint32_t s = sz > len - a ? len - a : sz;
                la[64u * j] = a | ty << 16 | s << 24;
                hb += s;
            }
            cnt = nh;
            pay_at = po > len ? len : po;
            pay_len = pl > len - pay_at ? len - pay_at : pl;
        }
    }
    for (uint32_t k = 0; k < P.nops; k++) {  // uniform
        const uint32_t kind = P.ops[k].kind, type = P.ops[k].hdr_type, index = P.ops[k].index;
        if (!run || st != PKT_EDIT_OK) continue;
        if (kind == PKT_EDIT_INSERT) {
            const uint32_t pos = index == PKT_EDIT_END || index > cnt ? cnt : index;
            for (uint32_t j = cnt; j > pos; j--) la[64u * j] = la[64u * (j - 1u)];
            const uint32_t size = s_size[type & 31u];
            la[64u * pos] = P.ops[k].data_off | type << 16 | size << 24 | kKonst;
            hb += size;
            if (++cnt > PKT_MAX_HDRS) st = PKT_EDIT_DEPTH;
            continue;
        }
        uint32_t at = cnt;  // the entry to remove, cnt = none
        if (kind == PKT_EDIT_POP) {
            at = cnt ? cnt - 1u : cnt;
        } else if (kind == PKT_EDIT_REMOVE_AT) {
            at = index < cnt ? index : cnt;
        } else {
            uint32_t seen = 0;
            for (uint32_t j = 0; j < cnt; j++) {
                const bool hit = ((la[64u * j] >> 16) & 0xFFu) == type;
                if (hit && seen == index && at == cnt) at = j;
                seen += hit ? 1u : 0u;
            }
        }
        if (at < cnt) {
            hb -= (la[64u * at] >> 24) & 0x3Fu;
            for (uint32_t j = at; j + 1u < cnt; j++) la[64u * j] = la[64u * (j + 1u)];
            cnt--;
        }
    }
    uint32_t total = hb + pay_len;
    if (st == PKT_EDIT_OK && (total > room || total > 65535u)) st = PKT_EDIT_NO_ROOM;
    if (st != PKT_EDIT_OK) cnt = total = pay_len = 0;

    // ---- the list as segments, in place (segment s is written after entry s was read), and the out chain
    uint32_t ns = 0, pos = 0, mask = 0;
    {
        uint32_t c_src = 0, c_start = 0;  // the open segment: its source and its destination start; it ends at pos
        bool open = false;
        for (uint32_t k = 0; k <= cnt; k++) {
            uint32_t src, size;
            if (k < cnt) {
                const uint32_t e = la[64u * k];
                const uint32_t ty = (e >> 16) & 0xFFu;
                src = e & (0xFFFFu | kKonst);
                size = (e >> 24) & 0x3Fu;
                if (P.o_hdr_type) P.o_hdr_type[(uint64_t)k * P.n + i] = (uint8_t)ty;
                if (P.o_hdr_off) P.o_hdr_off[(uint64_t)k * P.n + i] = (uint16_t)pos;
                mask |= ty < 32u ? 1u << ty : 0u;
            } else {
                src = pay_at;
                size = pay_len;
            }
            if (size && !(open && src == c_src + (pos - c_start))) {
                if (open) {
                    la[64u * ns] = c_src;
                    lb[64u * ns] = (uint16_t)pos;
                    ns++;
                }
                c_src = src;
                c_start = pos;
                open = true;
            }
            if (k < cnt) pos += size;
        }
        if (open) {
            la[64u * ns] = c_src;
            lb[64u * ns] = (uint16_t)(pos + pay_len);
            ns++;
        }
    }
    if (in) {
        if (P.out_len) P.out_len[i] = total;
        if (P.edit_status) P.edit_status[i] = (uint8_t)st;
        if (P.o_status)
            P.o_status[i] = (uint8_t)(st == PKT_EDIT_OK ? PKT_OK : st == PKT_EDIT_SKIPPED ? src_status
                                      : st == PKT_EDIT_DEPTH ? PKT_DEPTH_LIMIT : PKT_TRUNCATED);
        if (P.o_n_hdrs) P.o_n_hdrs[i] = (uint8_t)cnt;
        if (P.o_payload_off) P.o_payload_off[i] = (uint16_t)pos;
        if (P.o_payload_len) P.o_payload_len[i] = (uint16_t)pay_len;
        if (P.o_hdr_mask) P.o_hdr_mask[i] = mask;
    }

    // ---- phase 2: the wave's aligned destination chunks, flattened
    const uint32_t chunks = total ? (((uint32_t)o & 15u) + total + 15u) >> 4 : 0u;
    const uint32_t incl = wave_incl_scan(chunks, lane);
    if (lane == 0) s_pre[wv][0] = 0;
    s_pre[wv][lane + 1] = incl;
    s_src[wv][lane] = off;
    s_dst[wv][lane] = o;
    s_tot[wv][lane] = total | ns << 16;
    wave_sync();
    const uint32_t all = __builtin_amdgcn_readfirstlane(s_pre[wv][64]);  // <= 64 * 4097
    const FlatWalk walk = flat_walk(chunks);
    const Wave W{s_la[wv], s_lb[wv], s_src[wv], s_konst};
    for (uint32_t base = 0; base < all; base += 64u * kEdQ) {  // uniform
        Piece pc[kEdQ][2];
        uint32_t pr[kEdQ], s0[kEdQ], nsq[kEdQ], lo[kEdQ], hi[kEdQ];
        int32_t c0[kEdQ];
        uint8_t* at[kEdQ];
#pragma unroll
        for (uint32_t q = 0; q < kEdQ; q++) {
            const uint32_t f = base + 64u * q + lane;
            pr[q] = 64;  // no chunk
            s0[q] = nsq[q] = lo[q] = hi[q] = 0;
            c0[q] = 0;
            at[q] = nullptr;
            pc[q][0] = pc[q][1] = Piece{make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0), 0, 0, 0};
            if (f >= all) continue;
            const FlatAt pk = locate(walk, s_pre[wv], f);
            const uint32_t p = pk.p, k = pk.k;
            const uint64_t d = s_dst[wv][p];
            const uint32_t tn = s_tot[wv][p], tot = tn & 0xFFFFu, nsp = tn >> 16;
            const int32_t c = (int32_t)(16u * k) - (int32_t)((uint32_t)d & 15u);
            const uint32_t l = c < 0 ? 0u : (uint32_t)c;
            const uint32_t h = (uint32_t)(c + 16) < tot ? (uint32_t)(c + 16) : tot;  // c + 16 >= 1
            uint32_t s = 0;
            while (s < nsp && s_lb[wv][s * 64u + p] <= l) s++;  // the first segment ending past l
            pr[q] = p;
            s0[q] = s;
            nsq[q] = nsp;
            lo[q] = l;
            hi[q] = h;
            c0[q] = c;
            at[q] = P.dst + (d & ~(uint64_t)15) + 16ull * k;
            pc[q][0] = fetch(W, P.src.slab, p, s, nsp, c, l, h);
            pc[q][1] = fetch(W, P.src.slab, p, s + 1u, nsp, c, l, h);
        }
#pragma unroll
        for (uint32_t q = 0; q < kEdQ; q++) {
            if (pr[q] >= 64) continue;
            uint32_t out[4] = {0, 0, 0, 0};
            merge(pc[q][0], out);
            merge(pc[q][1], out);
            for (uint32_t s = s0[q] + 2u; s < nsq[q]; s++) {  // a chunk of three or more segments
                if (s_lb[wv][(s - 1u) * 64u + pr[q]] >= hi[q]) break;
                const Piece more = fetch(W, P.src.slab, pr[q], s, nsq[q], c0[q], lo[q], hi[q]);
                merge(more, out);
            }
            put_chunk(at[q], out, (uint32_t)((int32_t)lo[q] - c0[q]), (uint32_t)((int32_t)hi[q] - c0[q]));
        }
    }
}

}  // namespace

extern "C" int pkt_edit_batch(pkt_ctx_t* ctx, const pkt_batch_t* b, const pkt_out_t* parsed, const pkt_edit_op_t* ops,
                              uint32_t nops, const uint8_t* hdr_data, uint32_t hdr_data_len, const uint8_t* select,
                              uint8_t* dst, uint64_t dst_len, const uint64_t* dst_offsets, uint32_t slot, uint32_t* out_len,
                              uint8_t* edit_status, const pkt_out_t* out_chain, void* stream) {
    if (!ctx || !b || !parsed) return fail(ctx, PKT_ERR_INVALID_ARG, "null argument");
    if (nops > kEdMaxOps) return fail(ctx, PKT_ERR_INVALID_ARG, "pkt_edit_batch: more than 8 ops");
    if (nops && !ops) return fail(ctx, PKT_ERR_INVALID_ARG, "pkt_edit_batch: null ops");
    if (hdr_data_len > kEdData) return fail(ctx, PKT_ERR_INVALID_ARG, "pkt_edit_batch: hdr_data longer than 320 bytes");
    if (slot == 0) return fail(ctx, PKT_ERR_INVALID_ARG, "pkt_edit_batch: slot 0");
    if (b->n >= (1ull << 32)) return fail(ctx, PKT_ERR_INVALID_ARG, "pkt_edit_batch: n >= 2^32");
    for (uint32_t k = 0; k < nops; k++) {
        if (ops[k].kind > PKT_EDIT_INSERT) return fail(ctx, PKT_ERR_INVALID_ARG, "pkt_edit_batch: unknown op kind");
        if (ops[k].kind != PKT_EDIT_INSERT) continue;
        if (ops[k].hdr_type == 0 || ops[k].hdr_type >= PKT_HDR_COUNT)
            return fail(ctx, PKT_ERR_INVALID_ARG, "pkt_edit_batch: insert of an unknown header type");
        if (!hdr_data || (uint64_t)ops[k].data_off + (uint32_t)pkt_hdr_size(ops[k].hdr_type) > hdr_data_len)
            return fail(ctx, PKT_ERR_INVALID_ARG, "pkt_edit_batch: an insert's bytes run past hdr_data_len");
    }
    if (b->n == 0) return PKT_SUCCESS;
    if (!dst || !parsed->status || !parsed->n_hdrs || !parsed->hdr_type || !parsed->hdr_off || !parsed->payload_off ||
        !parsed->payload_len)
        return fail(ctx, PKT_ERR_INVALID_ARG, "pkt_edit_batch: null dst or chain column");
    if ((uintptr_t)dst & 15) return fail(ctx, PKT_ERR_INVALID_ARG, "pkt_edit_batch: dst not 16-byte aligned");
    int rc = check_batch_slab16(ctx, b);
    if (rc == PKT_SUCCESS) rc = check_batch_index(ctx, b);
    if (rc != PKT_SUCCESS) return rc;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    EParams P{};
    P.src = batch_src(b);
    P.n = b->n;
    P.status = parsed->status;
    P.n_hdrs = parsed->n_hdrs;
    P.hdr_type = parsed->hdr_type;
    P.hdr_off = parsed->hdr_off;
    P.payload_off = parsed->payload_off;
    P.payload_len = parsed->payload_len;
    P.select = select;
    P.dst = dst;
    P.dst_len = dst_len;
    P.dst_offsets = dst_offsets;
    P.slot = slot;
    P.out_len = out_len;
    P.edit_status = edit_status;
    if (out_chain) {
        P.o_status = out_chain->status;
        P.o_n_hdrs = out_chain->n_hdrs;
        P.o_hdr_type = out_chain->hdr_type;
        P.o_hdr_off = out_chain->hdr_off;
        P.o_payload_off = out_chain->payload_off;
        P.o_payload_len = out_chain->payload_len;
        P.o_hdr_mask = out_chain->hdr_mask;
    }
    P.nops = nops;
    for (uint32_t k = 0; k < nops; k++) P.ops[k] = ops[k];
    if (hdr_data_len) memcpy(P.data, hdr_data, hdr_data_len);
    const dim3 grid((unsigned)((b->n + kEdBlock - 1) / kEdBlock));
    hipLaunchKernelGGL(edit_kernel, grid, dim3(kEdBlock), 0, reinterpret_cast<hipStream_t>(stream), P);
    if ((e = hipGetLastError()) != hipSuccess) return hip_fail(ctx, e, "edit launch");
    return PKT_SUCCESS;
}
