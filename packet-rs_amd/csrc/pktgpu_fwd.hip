// pktgpu_fwd.hip — pkt_fwd_create / _destroy / _batch: the L3 forwarding rewrite over a routed batch.
//   fwd_kernel<LPM>  a lane owns a packet, a block 256 of them (a tile; a block takes one tile, or several where the
//                    launch caps the grid for the counters).  Lane p reads packet p's offset, length, select byte,
//                    next hop and chain (the first four rows up front, chain_load; later rows only for the chains
//                    that have them), finds the IP entry and the Ether entry before it (fwd_find_step,
//                    pktgpu_fwd.hpp), decides NO_IP / SPAN / NO_ETHER, then loads the one or two aligned 16-byte
//                    slab chunks that hold the IP header's bytes 0..11 (each holds a byte of the packet) and takes
//                    them out with take16; with LPM the destination address arrives the same way and goes through
//                    THE walk of pktgpu_lpm.hpp.  The adjacency entry is two aligned 16-byte loads.  An OK packet's
//                    stores are narrow and go to the Ether header's bytes 0..11 and the IP header's ttl and checksum
//                    bytes alone: the widest aligned pieces the MACs' address allows, one byte for the ttl, two
//                    bytes (one store where they are 2-byte aligned) for the checksum.  Counters: a wave's lanes
//                    with the same status add once to the block's LDS counters (its first four groups; the rest a
//                    lane at a time), and after a barrier thread s adds status s's non-zero count and bytes to the
//                    caller's arrays with one agent-scope atomic each, as match_kernel does.  No lane waits for
//                    another, there are no other atomics, and the LDS holds those counters alone.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "pktgpu_ctx.hpp"
#include "pktgpu_fwd.hpp"

struct pkt_fwd {
    pkt_ctx* ctx;
    int device;
    FwdAdj* adj;  // device
    uint32_t nadj;
};

namespace {

constexpr uint32_t kFBlock = 256;
constexpr uint32_t kWaveGroups = 4;  // distinct statuses a wave adds for as groups
// A counting launch's grid is capped and a block loops over tiles, so that the counters cost one add per block,
// status and counter: match_kernel's measurement for a short per-packet program (pktgpu_match.hip, kCountBlocks),
// taken over as it stands and not measured again for this kernel.
constexpr uint32_t kCountBlocks = 1280;

struct FParams {
    BatchSrc src;
    uint64_t n;  // < 2^32
    const uint8_t* n_hdrs;
    const uint8_t* hdr_type;  // [PKT_MAX_HDRS][n]
    const uint16_t* hdr_off;  // [PKT_MAX_HDRS][n]
    const FwdAdj* adj;
    uint32_t nadj, which, flags;
    LpmView t;
    const uint32_t* nexthop;
    const uint8_t* select;
    uint8_t* status;
    uint32_t* port;
    uint32_t* adj_index;
    uint64_t* hits;
    uint64_t* bytes;
};

// the 12 bytes w[0..2] (as they lie in memory) to p, any alignment: the head up to a 4-byte boundary, two dwords,
// the tail; every store aligned to its size and inside [p, p + 12)
__device__ __forceinline__ void store12(uint8_t* p, const uint32_t w[3]) {
    const uint32_t a = (uint32_t)(uintptr_t)p & 3u;
    if (a == 0) {
        uint32_t* q = reinterpret_cast<uint32_t*>(p);
        q[0] = w[0], q[1] = w[1], q[2] = w[2];
        return;
    }
    const uint32_t hb = 4u - a;  // head bytes, 1..3
    if (hb & 1u) p[0] = (uint8_t)w[0];
    if (hb & 2u) *reinterpret_cast<uint16_t*>(p + (hb & 1u)) = (uint16_t)(w[0] >> (8u * (hb & 1u)));
    uint32_t* q = reinterpret_cast<uint32_t*>(p + hb);
    q[0] = __builtin_amdgcn_alignbyte(w[1], w[0], hb);
    q[1] = __builtin_amdgcn_alignbyte(w[2], w[1], hb);
    uint8_t* tl = p + hb + 8;  // 4-byte aligned; the last `a` bytes
    const uint32_t tv = w[2] >> (8u * hb);
    if (a & 2u) {
        *reinterpret_cast<uint16_t*>(tl) = (uint16_t)tv;
        if (a & 1u) tl[2] = (uint8_t)(tv >> 16);
    } else {
        tl[0] = (uint8_t)tv;
    }
}

template <bool LPM>
__global__ __launch_bounds__(kFBlock) void fwd_kernel(FParams P) {
    __shared__ uint32_t s_hits[PKT_FWD_STATUS_COUNT];
    __shared__ unsigned long long s_bytes[PKT_FWD_STATUS_COUNT];
    const uint32_t t = threadIdx.x, lane = t & 63u;
    const bool counting = P.hits || P.bytes;  // uniform over the grid
    if (counting) {
        if (t < PKT_FWD_STATUS_COUNT) {
            s_hits[t] = 0;
            s_bytes[t] = 0;
        }
        __syncthreads();
    }
    const bool keep_l2 = P.flags & PKT_FWD_KEEP_L2, write = !(P.flags & PKT_FWD_NO_WRITE);
    const uint32_t ntiles = (uint32_t)((P.n + kFBlock - 1) / kFBlock);
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {  // uniform
        const uint64_t i = (uint64_t)tile * kFBlock + t;
        const bool act = i < P.n;
        uint32_t st = PKT_FWD_SKIPPED, len = 0;
        if (act) {
            const uint64_t off = pkt_off(P.src, i);
            len = pkt_len(P.src, i, off);
            const ChainPre c = chain_load(P, i);
            const uint32_t sel = P.select ? P.select[i] : 1u;
            uint32_t a = PKT_FWD_NONE;
            if (!LPM) a = P.nexthop[i];
            uint32_t out_port = PKT_FWD_NONE, out_adj = PKT_FWD_NONE;
            if (sel) {
                const uint32_t nh = c.nh > PKT_MAX_HDRS ? PKT_MAX_HDRS : c.nh;
                FwdFind f;
#pragma unroll
                for (uint32_t j = 0; j < 4; j++)
                    if (j < nh) fwd_find_step(f, P.which, c.ty[j], c.of[j]);
                for (uint32_t j = 4; j < nh; j++) {
                    const uint32_t ty = P.hdr_type[(uint64_t)j * P.n + i];
                    if (!fwd_wants(ty)) continue;
                    fwd_find_step(f, P.which, ty, P.hdr_off[(uint64_t)j * P.n + i]);
                }
                st = fwd_find_status(f, len, keep_l2);
                if (st == PKT_FWD_OK) {
                    const bool v4 = f.ipt == PKT_HDR_IPV4;
                    // The IP header's bytes [S, S + 12) lie inside the packet.  Chunk k of the aligned chunks from
                    // S's on is loaded iff it holds a byte of them, so it lies at or below the slab's last chunk.
                    const uint64_t S = off + f.ipo;
                    const uint32_t sh = (uint32_t)S & 15u;
                    const uint8_t* A = P.src.slab + (S & ~(uint64_t)15);
                    const uint4 c0 = *reinterpret_cast<const uint4*>(A);
                    const uint4 c1 = sh + 12u > 16u ? *reinterpret_cast<const uint4*>(A + 16) : make_uint4(0, 0, 0, 0);
                    uint32_t w[4] = {0, 0, 0, 0};
                    if (LPM) {  // the destination address, as lpm_kernel takes it (inside the header: inside the packet)
                        const uint64_t D = S + (v4 ? 16u : 24u);
                        const uint32_t dh = (uint32_t)D & 15u, span = v4 ? 4u : 16u;
                        const uint8_t* B = P.src.slab + (D & ~(uint64_t)15);
                        const uint4 d0 = *reinterpret_cast<const uint4*>(B);
                        const uint4 d1 = dh + span > 16u ? *reinterpret_cast<const uint4*>(B + 16) : make_uint4(0, 0, 0, 0);
                        uint32_t m[4];
                        take16(d0, d1, dh, m);
                        w[0] = __builtin_bswap32(m[0]);
#pragma unroll
                        for (uint32_t q = 1; q < 4; q++) w[q] = v4 ? 0u : __builtin_bswap32(m[q]);
                    }
                    uint32_t h[4];
                    take16(c0, c1, sh, h);  // (h[3]: bytes 12..15 where they were loaded; not used)
                    const FwdIp ip = fwd_ip_fields(h, v4);
                    if (ip.t <= 1u) {
                        st = PKT_FWD_TTL;
                    } else {
                        if (LPM) a = lpm_lookup(w, v4, P.t, true).nexthop;
                        out_adj = a;
                        if (a >= P.nadj) {
                            st = PKT_FWD_NO_ADJ;
                        } else {
                            const uint4* e = reinterpret_cast<const uint4*>(P.adj + a);
                            const uint4 e0 = e[0], e1 = e[1];
                            st = fwd_adj_status(e1.x, ip.l3len);
                            if (st == PKT_FWD_OK) {
                                out_port = e0.w;
                                if (write) {
                                    if (!keep_l2) {
                                        const uint32_t mac[3] = {e0.x, e0.y, e0.z};
                                        store12(const_cast<uint8_t*>(P.src.slab) + off + f.eth, mac);
                                    }
                                    uint8_t* ipp = const_cast<uint8_t*>(P.src.slab) + S;
                                    if (v4) {
                                        const uint32_t nw = fwd_v4_word(h[2]);  // bytes 8..11 after the rewrite
                                        ipp[8] = (uint8_t)nw;
                                        if (((uint32_t)S & 1u) == 0) {
                                            *reinterpret_cast<uint16_t*>(ipp + 10) = (uint16_t)(nw >> 16);
                                        } else {
                                            ipp[10] = (uint8_t)(nw >> 16);
                                            ipp[11] = (uint8_t)(nw >> 24);
                                        }
                                    } else {
                                        ipp[7] = (uint8_t)(ip.t - 1u);
                                    }
                                }
                            }
                        }
                    }
                }
            }
            if (P.status) P.status[i] = (uint8_t)st;
            if (P.port) P.port[i] = out_port;
            if (P.adj_index) P.adj_index[i] = out_adj;
        }
        // ---- counters: the wave's lanes of one status add once (match_kernel's groups)
        if (counting) {
            uint64_t todo = __ballot(act);
            for (uint32_t g = 0; g < kWaveGroups && todo; g++) {  // uniform
                const uint32_t lead = (uint32_t)__ffsll((unsigned long long)todo) - 1u;
                const uint32_t sl = (uint32_t)__builtin_amdgcn_readlane((int)st, (int)__builtin_amdgcn_readfirstlane((int)lead));
                const bool mine = act && st == sl;
                const uint64_t m = __ballot(mine);
                uint32_t sum = mine ? len : 0u;
#pragma unroll
                for (uint32_t x = 32; x; x >>= 1) sum += (uint32_t)__shfl_xor((int)sum, (int)x, 64);
                if (lane == lead) {
                    atomicAdd(&s_hits[sl], (uint32_t)__popcll((unsigned long long)m));
                    atomicAdd(&s_bytes[sl], (unsigned long long)sum);
                }
                todo &= ~m;
            }
            if ((todo >> lane) & 1ull) {
                atomicAdd(&s_hits[st], 1u);
                atomicAdd(&s_bytes[st], (unsigned long long)len);
            }
        }
    }
    if (!counting) return;
    __syncthreads();
    if (t < PKT_FWD_STATUS_COUNT) {
        const uint32_t h = s_hits[t];
        const uint64_t bsum = s_bytes[t];
        if (P.hits && h) __hip_atomic_fetch_add(P.hits + t, (uint64_t)h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (P.bytes && bsum) __hip_atomic_fetch_add(P.bytes + t, bsum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

int fwd_refuse(pkt_ctx* ctx, const char* where, const char* msg) {
    if (ctx) ctx->err = std::string(where) + ": " + msg;
    return PKT_ERR_INVALID_ARG;
}

}  // namespace

extern "C" int pkt_fwd_create(pkt_ctx_t* ctx, const pkt_fwd_adj_t* adj, uint32_t nadj, pkt_fwd_t** out) {
    if (!ctx || !out) return fwd_refuse(ctx, "pkt_fwd_create", "null argument");
    *out = nullptr;
    if (const char* msg = fwd_adj_error(adj, nadj)) return fwd_refuse(ctx, "pkt_fwd_create", msg);
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    std::vector<FwdAdj> img(nadj);
    for (uint32_t k = 0; k < nadj; k++) img[k] = fwd_pack(adj[k]);
    pkt_fwd* f = new pkt_fwd{ctx, ctx->device, nullptr, nadj};
    if (nadj) {
        e = hipMalloc(reinterpret_cast<void**>(&f->adj), sizeof(FwdAdj) * (size_t)nadj);
        if (e == hipSuccess) e = hipMemcpy(f->adj, img.data(), sizeof(FwdAdj) * (size_t)nadj, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            if (f->adj) (void)hipFree(f->adj);
            delete f;
            return hip_fail(ctx, e, "pkt_fwd_create");
        }
    }
    *out = f;
    return PKT_SUCCESS;
}

extern "C" int pkt_fwd_destroy(pkt_fwd_t* f) {
    if (!f) return PKT_ERR_INVALID_ARG;
    (void)hipSetDevice(f->device);
    const hipError_t e = f->adj ? hipFree(f->adj) : hipSuccess;
    delete f;
    return e == hipSuccess ? PKT_SUCCESS : PKT_ERR_HIP;
}

extern "C" int pkt_fwd_batch(pkt_fwd_t* f, const pkt_batch_t* b, const pkt_chain_t* chain, uint32_t which_ip,
                             uint32_t flags, pkt_lpm_t* lpm, const uint32_t* nexthop, const uint8_t* select,
                             uint8_t* status, uint32_t* port, uint32_t* adj_index, uint64_t* hits, uint64_t* bytes,
                             void* stream) {
    if (!f) return PKT_ERR_INVALID_ARG;
    pkt_ctx* ctx = f->ctx;
    if (const char* msg = fwd_call_error(b, chain, which_ip, flags, lpm, nexthop, hits, bytes, true, f->device))
        return fwd_refuse(ctx, "pkt_fwd_batch", msg);
    if (b->n == 0) return PKT_SUCCESS;
    if (const char* msg = fwd_batch_error(b, chain, true)) return fwd_refuse(ctx, "pkt_fwd_batch", msg);
    if (!status && !port && !adj_index && !hits && !bytes && (flags & PKT_FWD_NO_WRITE)) return PKT_SUCCESS;
    hipError_t e = hipSetDevice(f->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    FParams P{};
    P.src = batch_src(b);
    P.n = b->n;
    P.n_hdrs = chain->n_hdrs;
    P.hdr_type = chain->hdr_type;
    P.hdr_off = chain->hdr_off;
    P.adj = f->adj;
    P.nadj = f->nadj;
    P.which = which_ip;
    P.flags = flags;
    if (lpm) P.t = lpm->view;
    P.nexthop = nexthop;
    P.select = select;
    P.status = status;
    P.port = port;
    P.adj_index = adj_index;
    P.hits = hits;
    P.bytes = bytes;
    const uint64_t tiles = (b->n + kFBlock - 1) / kFBlock;
    const dim3 grid((unsigned)((hits || bytes) && tiles > kCountBlocks ? kCountBlocks : tiles));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (lpm)
        hipLaunchKernelGGL(fwd_kernel<true>, grid, dim3(kFBlock), 0, s, P);
    else
        hipLaunchKernelGGL(fwd_kernel<false>, grid, dim3(kFBlock), 0, s, P);
    if ((e = hipGetLastError()) != hipSuccess) return hip_fail(ctx, e, "fwd_kernel launch");
    return PKT_SUCCESS;
}
