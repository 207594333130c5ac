// pktgpu_lpm.hip — pkt_lpm_create and the device half of pkt_lpm_lookup_batch / pkt_lpm_lookup_keys.
//   lpm_kernel<KEYS>   a lane owns a packet.  Batch source: lane p reads packet p's offset, length and chain (the
//                    first four rows up front, chain_load), finds the IP entry as pkt_flow_key_batch does, decides
//                    NO_IP / SPAN, then loads the one or two aligned 16-byte slab chunks that hold the 4 / 16
//                    address bytes (each holds a byte of the packet) and takes them out with take16.  Keys source:
//                    the address and the version come from a pkt_flow_key_t, by dword loads where the array is
//                    4-byte aligned and by 2-byte loads otherwise.  Then THE walk of pktgpu_lpm.hpp (lpm_walk: the
//                    root entry, then a node entry per level while bit 31 is set, at most the table's depth), the
//                    route's record if nexthop or plen is asked for, and one store per output, lane i to element i.
//                    A latency-bound gather: no LDS, no atomics, no lane waits for another; what hides the chain of
//                    dependent loads is the number of waves in flight, so the kernel keeps its registers low.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pktgpu_ctx.hpp"
#include "pktgpu_lpm.hpp"

namespace {

constexpr uint32_t kLpmBlock = 256;

struct LParams {
    BatchSrc src;
    uint64_t n;  // < 2^32
    const uint8_t* n_hdrs;
    const uint8_t* hdr_type;  // [PKT_MAX_HDRS][n]
    const uint16_t* hdr_off;  // [PKT_MAX_HDRS][n]
    const uint8_t* keys;      // [n][40], 2-byte aligned
    const uint8_t* key_status;
    LpmView t;
    uint32_t which, flags;
    uint32_t* route;
    uint32_t* nexthop;
    uint8_t* plen;
    uint8_t* status;
};

__device__ __forceinline__ bool is_ip(uint32_t t) { return t == PKT_HDR_IPV4 || t == PKT_HDR_IPV6; }

template <bool KEYS>
__global__ __launch_bounds__(kLpmBlock) void lpm_kernel(LParams P) {
    const uint64_t i = (uint64_t)blockIdx.x * kLpmBlock + threadIdx.x;
    if (i >= P.n) return;  // no barrier, no cross-lane step below
    const bool src = P.flags & PKT_LPM_SRC;
    uint32_t w[4] = {0, 0, 0, 0};
    uint32_t st = PKT_LPM_OK;
    bool v4 = true;
    if (KEYS) {
        const uint8_t* k = P.keys + 40ull * i;
        const uint8_t* a = k + (src ? 0u : 16u);
        uint32_t m[4], tail;  // the address as it lies in memory; bytes 36..39 (proto, ipver, zero)
        if (((uintptr_t)P.keys & 3u) == 0) {  // uniform
#pragma unroll
            for (uint32_t q = 0; q < 4; q++) m[q] = reinterpret_cast<const uint32_t*>(a)[q];
            tail = reinterpret_cast<const uint32_t*>(k)[9];
        } else {
            const uint16_t* h = reinterpret_cast<const uint16_t*>(a);
#pragma unroll
            for (uint32_t q = 0; q < 4; q++) m[q] = h[2 * q] | (uint32_t)h[2 * q + 1] << 16;
            tail = reinterpret_cast<const uint16_t*>(k)[18];
        }
        const uint32_t ver = tail >> 8 & 0xFFu;
        v4 = ver == 4;
        if ((P.key_status && P.key_status[i]) || (ver != 4 && ver != 6)) st = PKT_LPM_SKIPPED;
        w[0] = __builtin_bswap32(m[0]);
#pragma unroll
        for (uint32_t q = 1; q < 4; q++) w[q] = v4 ? 0u : __builtin_bswap32(m[q]);
    } else {
        const uint64_t off = pkt_off(P.src, i);
        const uint32_t len = pkt_len(P.src, i, off);
        const ChainPre c = chain_load(P, i);
        const uint32_t nh = c.nh > PKT_MAX_HDRS ? PKT_MAX_HDRS : c.nh;
        // the IP entry: pkt_flow_key_batch's search, less the entry behind it
        uint32_t ipt = 0, ipo = 0, seen = 0;
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            const bool hit = j < nh && is_ip(c.ty[j]);
            const bool take = hit && (P.which == PKT_FLOW_LAST || seen == P.which);
            ipt = take ? c.ty[j] : ipt;
            ipo = take ? c.of[j] : ipo;
            seen += hit ? 1u : 0u;
        }
        for (uint32_t j = 4; j < nh; j++) {
            const uint32_t ty = P.hdr_type[(uint64_t)j * P.n + i];
            if (!is_ip(ty)) continue;
            if (P.which == PKT_FLOW_LAST || seen == P.which) {
                ipt = ty;
                ipo = P.hdr_off[(uint64_t)j * P.n + i];
            }
            seen++;
        }
        v4 = ipt != PKT_HDR_IPV6;
        if (!ipt) {
            st = PKT_LPM_NO_IP;
        } else if (ipo + (v4 ? 20u : 40u) > len) {
            st = PKT_LPM_SPAN;
        } else {
            // The address bytes [S, S + 4 | 16) lie inside the packet.  Chunk k of the aligned chunks from S's on
            // is loaded iff it holds a byte of them, so it lies at or below the slab's last aligned chunk.
            const uint64_t S = off + ipo + (v4 ? (src ? 12u : 16u) : (src ? 8u : 24u));
            const uint32_t sh = (uint32_t)S & 15u, span = v4 ? 4u : 16u;
            const uint8_t* A = P.src.slab + (S & ~(uint64_t)15);
            const uint4 c0 = *reinterpret_cast<const uint4*>(A);
            const uint4 c1 = sh + span > 16u ? *reinterpret_cast<const uint4*>(A + 16) : make_uint4(0, 0, 0, 0);
            uint32_t m[4];
            take16(c0, c1, sh, m);
            w[0] = __builtin_bswap32(m[0]);
#pragma unroll
            for (uint32_t q = 1; q < 4; q++) w[q] = v4 ? 0u : __builtin_bswap32(m[q]);
        }
    }
    LpmResult r = lpm_miss(P.t, st);
    if (st == PKT_LPM_OK) r = lpm_lookup(w, v4, P.t, P.nexthop || P.plen);
    if (P.route) P.route[i] = r.route;
    if (P.nexthop) P.nexthop[i] = r.nexthop;
    if (P.plen) P.plen[i] = (uint8_t)r.plen;
    if (P.status) P.status[i] = (uint8_t)r.status;
}

int lpm_hip_fail(pkt_lpm* t, hipError_t e, const char* what) {
    t->err = std::string(what) + ": " + hipGetErrorString(e);
    return PKT_ERR_HIP;
}

int dev_lookup(pkt_lpm* t, const LpmCall& c, void* stream) {
    hipError_t e = hipSetDevice(t->device);
    if (e != hipSuccess) return lpm_hip_fail(t, e, "hipSetDevice");
    LParams P{};
    P.src = c.src;
    P.n = c.n;
    P.n_hdrs = c.n_hdrs;
    P.hdr_type = c.hdr_type;
    P.hdr_off = c.hdr_off;
    P.keys = c.keys;
    P.key_status = c.key_status;
    P.t = t->view;
    P.which = c.which;
    P.flags = c.flags;
    P.route = c.route;
    P.nexthop = c.nexthop;
    P.plen = c.plen;
    P.status = c.status;
    const dim3 grid((unsigned)((c.n + kLpmBlock - 1) / kLpmBlock));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (c.from_keys)
        hipLaunchKernelGGL(lpm_kernel<true>, grid, dim3(kLpmBlock), 0, s, P);
    else
        hipLaunchKernelGGL(lpm_kernel<false>, grid, dim3(kLpmBlock), 0, s, P);
    if ((e = hipGetLastError()) != hipSuccess) return lpm_hip_fail(t, e, "lpm lookup launch");
    return PKT_SUCCESS;
}

int dev_destroy(pkt_lpm* t) {
    (void)hipSetDevice(t->device);
    (void)hipDeviceSynchronize();
    if (t->dev_words) (void)hipFree(t->dev_words);
    return PKT_SUCCESS;
}

constexpr LpmDevOps kDevOps = {dev_lookup, dev_destroy};

}  // namespace

extern "C" int pkt_lpm_create(pkt_ctx_t* ctx, const pkt_lpm_route_t* routes, uint32_t nroutes, uint32_t default_nexthop,
                              uint64_t max_bytes, pkt_lpm_t** out) {
    if (!ctx || !out) return fail(ctx, PKT_ERR_INVALID_ARG, "pkt_lpm_create: null argument");
    *out = nullptr;
    LpmImage img;
    int rc = lpm_compile(routes, nroutes, max_bytes, img, ctx->err);
    if (rc != PKT_SUCCESS) return rc;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) return hip_fail(ctx, e, "hipSetDevice");
    pkt_lpm* t = new pkt_lpm;
    t->ops = &kDevOps;
    t->device = ctx->device;
    t->info = img.info;
    e = hipMalloc(reinterpret_cast<void**>(&t->dev_words), img.info.bytes);
    if (e == hipSuccess) e = hipMemcpy(t->dev_words, img.words.data(), img.info.bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        rc = hip_fail(ctx, e, "pkt_lpm_create");
        dev_destroy(t);
        delete t;
        return rc;
    }
    t->view = img.view(t->dev_words, default_nexthop);
    *out = t;
    return PKT_SUCCESS;
}
