// pktgpu_outbatch.hip — what pkt_frag_*, pkt_reasm_* and pkt_icmp_err_* run in common (the contract:
// pktgpu_outbatch.hpp): the one-block scan of the tile sums with the overflow verdict, and the call plumbing around
// an entry's launches: the refusal and error texts, the blocking call's one host wait, the queued call and its result.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pktgpu_ctx.hpp"
#include "pktgpu_outbatch.hpp"

namespace {

constexpr uint32_t kOBlock = 256;
constexpr uint32_t kOWaves = kOBlock / 64;
constexpr uint32_t kOScanPer = 16;  // tile sums per thread and round of the scan

// tot: [total rounded bytes, outputs, overflow] on the device; host: the same three words in pinned memory
__global__ __launch_bounds__(kOBlock) void out_scan_kernel(uint64_t* __restrict__ blk_bytes, uint64_t* __restrict__ blk_cnt,
                                                           uint32_t nb, uint32_t no_write, uint64_t out_cap,
                                                           uint64_t dst_len, uint64_t* __restrict__ tot,
                                                           uint64_t* __restrict__ host) {
    __shared__ uint64_t s_w[kOWaves];
    uint64_t cb = 0, cc = 0;
    for (uint64_t base = 0; base < nb; base += (uint64_t)kOBlock * kOScanPer) {
        const uint64_t i0 = base + (uint64_t)threadIdx.x * kOScanPer;
        uint64_t b[kOScanPer], c[kOScanPer], sb = 0, sc = 0;
#pragma unroll
        for (uint32_t j = 0; j < kOScanPer; j++) {
            const bool in = i0 + j < nb;
            b[j] = in ? blk_bytes[i0 + j] : 0;
            c[j] = in ? blk_cnt[i0 + j] : 0;
            sb += b[j];
            sc += c[j];
        }
        uint64_t tb, tc;
        uint64_t eb = cb + block_excl_scan<kOWaves>(sb, s_w, tb);
        uint64_t ec = cc + block_excl_scan<kOWaves>(sc, s_w, tc);
#pragma unroll
        for (uint32_t j = 0; j < kOScanPer; j++) {
            if (i0 + j < nb) {
                blk_bytes[i0 + j] = eb;
                blk_cnt[i0 + j] = ec;
            }
            eb += b[j];
            ec += c[j];
        }
        cb += tb;
        cc += tc;
    }
    if (threadIdx.x == 0) {
        const uint64_t over = !no_write && out_overflow(cc, cb, out_cap, dst_len) ? 1u : 0u;
        tot[0] = cb, tot[1] = cc, tot[2] = over;
        host[0] = cb, host[1] = cc, host[2] = over;
    }
}

void zero_totals(uint64_t* bytes_out_total, uint64_t* n_out) {
    if (bytes_out_total) *bytes_out_total = 0;
    if (n_out) *n_out = 0;
}

}  // namespace

void pktgpu_out_scan_launch(uint64_t* blk_bytes, uint64_t* blk_cnt, uint32_t nb, bool no_write, uint64_t out_cap,
                            uint64_t dst_len, uint64_t* tot, uint64_t* host, hipStream_t s) {
    hipLaunchKernelGGL(out_scan_kernel, dim3(1), dim3(kOBlock), 0, s, blk_bytes, blk_cnt, nb, no_write ? 1u : 0u, out_cap,
                       dst_len, tot, host);
}

int pktgpu_out_refuse(pkt_ctx_t* ctx, const OutEntry& en, const char* msg) {
    if (ctx) ctx->err = std::string(en.batch) + ": " + msg;
    return PKT_ERR_INVALID_ARG;
}

int pktgpu_out_finish(pkt_ctx_t* ctx, const OutEntry& en, uint64_t* bytes_out_total, uint64_t* n_out) {
    const OutScratch& sc = ctx->*en.scratch;
    if (bytes_out_total) *bytes_out_total = sc.ctl[0];
    if (n_out) *n_out = sc.ctl[1];
    if (sc.ctl[2])
        return pktgpu_out_refuse(ctx, en, "the outputs do not fit out_cap / dst_len (the totals are the capacity needed)");
    return PKT_SUCCESS;
}

// (queue refuses a null ctx itself, before anything here touches it)
int pktgpu_out_batch(pkt_ctx_t* ctx, const OutEntry& en, const OutQueue& queue, void* stream, uint64_t* bytes_out_total,
                     uint64_t* n_out) {
    zero_totals(bytes_out_total, n_out);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int rc = queue(s);
    if (rc != PKT_SUCCESS) return rc;
    const hipError_t e = hipStreamSynchronize(s);  // the one host wait, for the totals
    if (e != hipSuccess) return hip_fail(ctx, e, en.batch);
    return pktgpu_out_finish(ctx, en, bytes_out_total, n_out);
}

int pktgpu_out_batch_async(pkt_ctx_t* ctx, const OutEntry& en, const OutQueue& queue, void* stream) {
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int rc = queue(s);
    if (rc != PKT_SUCCESS) return rc;
    (ctx->*en.scratch).mark(s);
    return PKT_SUCCESS;
}

int pktgpu_out_result(pkt_ctx_t* ctx, const OutEntry& en, uint64_t* bytes_out_total, uint64_t* n_out) {
    zero_totals(bytes_out_total, n_out);
    if (!ctx) return PKT_ERR_INVALID_ARG;
    OutScratch& sc = ctx->*en.scratch;
    if (!sc.pending) {
        ctx->err = std::string(en.result) + ": no call queued on this ctx";
        return PKT_ERR_INVALID_ARG;
    }
    const hipError_t e = sc.take();
    if (e != hipSuccess) return hip_fail(ctx, e, en.result);
    return pktgpu_out_finish(ctx, en, bytes_out_total, n_out);
}
