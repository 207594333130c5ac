// pktgpu_ctx.cpp — the life of a pkt_ctx and its knobs (pkt_ctx_* of include/pktgpu.h).  Host code only.
// The ctx's resources (pktgpu_ctx.hpp) are allocated on first use by the sources that use them; all are freed here.
#include <hip/hip_runtime.h>

#include "pktgpu_ctx.hpp"

extern "C" {

int pkt_ctx_create(int device, pkt_ctx_t** out) {
    if (!out) return PKT_ERR_INVALID_ARG;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0) return PKT_ERR_NO_DEVICE;
    if (device < 0 || device >= count) return PKT_ERR_INVALID_ARG;
    pkt_ctx* c = new pkt_ctx();
    c->device = device;  // (the knobs start at their defaults, pktgpu_ctx.hpp)
    *out = c;
    return PKT_SUCCESS;
}

int pkt_ctx_destroy(pkt_ctx_t* ctx) {
    if (!ctx) return PKT_SUCCESS;
    HostPipe& hp = ctx->hp;
    // A ctx that never touched the device makes no HIP call (pkt_pcap_stream_close and error paths destroy
    // such ones).  hp.s[0]: the host pipeline's streams come before any of its buffers and events.
    const bool owns = ctx->tv_flag || ctx->tv_win || ctx->tv_win_ev || ctx->mx.dev || ctx->pc.buf || ctx->pc.ctl ||
                      ctx->pw.buf || ctx->pw.ctl || ctx->fr.buf || ctx->fr.ctl || ctx->rs.buf || ctx->rs.ctl || ctx->ic.buf || ctx->ic.ctl || ctx->te.buf || ctx->te.ctl || ctx->td.buf ||
                      ctx->td.ctl || ctx->cmp.acc || ctx->cmp.ctl || hp.s[0];
    if (owns) {
        (void)hipSetDevice(ctx->device);
        (void)hipDeviceSynchronize();  // nothing queued still uses what is freed below
        (void)hipFree(ctx->tv_flag);
        for (hipEvent_t ev : ctx->tv_ev)
            if (ev) (void)hipEventDestroy(ev);
        (void)hipFree(ctx->tv_win);
        if (ctx->tv_win_ev) (void)hipEventDestroy(ctx->tv_win_ev);
        (void)hipFree(ctx->mx.dev);
        (void)hipHostFree(ctx->mx.host);
        (void)hipFree(ctx->pc.buf);
        (void)hipHostFree(ctx->pc.ctl);
        for (OutScratch* o : {static_cast<OutScratch*>(&ctx->pw), &ctx->fr, &ctx->rs, &ctx->ic, &ctx->te, &ctx->td}) o->release();
        (void)hipFree(ctx->cmp.acc);
        (void)hipHostFree(ctx->cmp.ctl);
        for (int k = 0; k < HostPipe::kSlots; k++) {
            if (hp.s[k]) (void)hipStreamDestroy(hp.s[k]);
            if (hp.ev[k]) (void)hipEventDestroy(hp.ev[k]);
            (void)hipFree(hp.slab[k]);
            (void)hipFree(hp.offs[k]);
            (void)hipFree(hp.lens[k]);
            (void)hipFree(hp.out[k]);
        }
        (void)hipFree(hp.file);
        (void)hipFree(hp.ioffs);
        (void)hipFree(hp.ilens);
        (void)hipFree(hp.pcarry);
        (void)hipFree(hp.pnh);
        (void)hipFree(hp.dcol);
        for (hipEvent_t x : hp.ev_copy)
            if (x) (void)hipEventDestroy(x);
        if (hp.ev_parsed) (void)hipEventDestroy(hp.ev_parsed);
        for (hipEvent_t x : hp.ev_xdone)
            if (x) (void)hipEventDestroy(x);
    }
    delete ctx;
    return PKT_SUCCESS;
}

const char* pkt_ctx_last_error(const pkt_ctx_t* ctx) { return ctx ? ctx->err.c_str() : "null ctx"; }

int pkt_ctx_set_window(pkt_ctx_t* ctx, uint32_t w) {
    if (!ctx) return PKT_ERR_INVALID_ARG;
    ctx->window = w;
    return PKT_SUCCESS;
}

int pkt_ctx_set_fastpath(pkt_ctx_t* ctx, int enable) {
    if (!ctx || enable < 0 || enable > 1) return PKT_ERR_INVALID_ARG;
    ctx->fast = enable;
    return PKT_SUCCESS;
}

int pkt_ctx_set_staging(pkt_ctx_t* ctx, int mode) {
    if (!ctx || mode < 0 || mode > 2) return PKT_ERR_INVALID_ARG;
    ctx->staging = mode;
    return PKT_SUCCESS;
}

int pkt_ctx_set_walk(pkt_ctx_t* ctx, int mode) {
    if (!ctx || mode < 0 || mode > 2) return PKT_ERR_INVALID_ARG;
    ctx->walk = mode;
    return PKT_SUCCESS;
}

int pkt_ctx_set_host_piece(pkt_ctx_t* ctx, uint64_t bytes) {
    if (!ctx || (bytes != 0 && bytes < 4096)) return PKT_ERR_INVALID_ARG;
    ctx->host_piece = bytes;
    return PKT_SUCCESS;
}

int pkt_ctx_set_pcap_scan64(pkt_ctx_t* ctx, int enable) {
    if (!ctx || enable < 0 || enable > 1) return PKT_ERR_INVALID_ARG;
    ctx->pc.scan64 = enable != 0;
    return PKT_SUCCESS;
}

}  // extern "C"
