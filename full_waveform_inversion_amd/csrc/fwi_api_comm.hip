// C-ABI of the engine, the RCCL exchange between the contexts of a job (include/fwi.h: fwi_comm_*, fwi_allreduce_*).
// Host side only.
#include <rccl/rccl.h>

#include <cstring>

#include "fwi_host.h"

#define NCCLCHK(ctx, call)                                                                    \
    do {                                                                                      \
        ncclResult_t r_ = (call);                                                             \
        if (r_ != ncclSuccess) return (ctx)->fail(FWI_ECOMM, "%s: %s", #call, ncclGetErrorString(r_)); \
    } while (0)

extern "C" {

int fwi_comm_unique_id(void *id_out) {
    static_assert(sizeof(ncclUniqueId) == FWI_UNIQUE_ID_BYTES, "ncclUniqueId size");
    if (!id_out) return FWI_EINVAL;
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) return FWI_ECOMM;
    memcpy(id_out, &id, sizeof id);
    return FWI_OK;
}

int fwi_comm_init(fwi_ctx *ctx, int32_t rank, int32_t nranks, const void *id) {
    if (!ctx) return FWI_EINVAL;
    if (!id || nranks < 1 || rank < 0 || rank >= nranks)
        return ctx->fail(FWI_EINVAL, "fwi_comm_init: bad rank %d of %d", rank, nranks);
    (void)hipSetDevice(ctx->cfg.device);
    if (ctx->comm) {
        (void)ncclCommDestroy(ctx->comm);
        ctx->comm = nullptr;
    }
    ncclUniqueId uid;
    memcpy(&uid, id, sizeof uid);
    ncclResult_t r = ncclCommInitRank(&ctx->comm, nranks, uid, rank);
    if (r != ncclSuccess) {
        ctx->comm = nullptr;
        ctx->nranks = 1;
        return ctx->fail(FWI_ECOMM, "ncclCommInitRank(rank %d of %d): %s", rank, nranks, ncclGetErrorString(r));
    }
    ctx->nranks = nranks;
    return FWI_OK;
}

int fwi_comm_info(fwi_ctx *ctx, int32_t *nranks_out, int32_t *rank_out) {
    if (!ctx) return FWI_EINVAL;
    if (!ctx->comm) return ctx->fail(FWI_ESTATE, "fwi_comm_info: call fwi_comm_init first");
    int n = 0, r = -1;
    NCCLCHK(ctx, ncclCommCount(ctx->comm, &n));
    NCCLCHK(ctx, ncclCommUserRank(ctx->comm, &r));
    if (nranks_out) *nranks_out = n;
    if (rank_out) *rank_out = r;
    return FWI_OK;
}

int fwi_comm_abort(fwi_ctx *ctx) {
    if (!ctx) return FWI_EINVAL;
    if (!ctx->comm) return FWI_OK;
    (void)hipSetDevice(ctx->cfg.device);
    ncclComm_t c = ctx->comm;
    ctx->comm = nullptr;
    ctx->nranks = 1;
    NCCLCHK(ctx, ncclCommAbort(c));
    return FWI_OK;
}

int fwi_allreduce_gradient(fwi_ctx *ctx) {
    if (!ctx) return FWI_EINVAL;
    if (!ctx->comm) return ctx->fail(FWI_ESTATE, "fwi_allreduce_gradient: call fwi_comm_init first");
    (void)hipSetDevice(ctx->cfg.device);
    NCCLCHK(ctx, ncclAllReduce(ctx->g_acc, ctx->g_acc, (size_t)ctx->gd.npts,
                               ctx->cfg.dtype == FWI_F32 ? ncclFloat32 : ncclFloat64, ncclSum, ctx->comm,
                               ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return FWI_OK;
}

int fwi_allreduce_illumination(fwi_ctx *ctx) {
    if (!ctx) return FWI_EINVAL;
    if (!ctx->comm) return ctx->fail(FWI_ESTATE, "fwi_allreduce_illumination: call fwi_comm_init first");
    if (!ctx->h_acc) return ctx->fail(FWI_ESTATE, "fwi_allreduce_illumination: illumination is disabled");
    (void)hipSetDevice(ctx->cfg.device);
    NCCLCHK(ctx, ncclAllReduce(ctx->h_acc, ctx->h_acc, (size_t)ctx->gd.npts,
                               ctx->cfg.dtype == FWI_F32 ? ncclFloat32 : ncclFloat64, ncclSum, ctx->comm,
                               ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return FWI_OK;
}

static int allreduce_scalars(fwi_ctx *ctx, double *vals, int32_t n, ncclRedOp_t op, const char *who) {
    if (!ctx) return FWI_EINVAL;
    if (!ctx->comm) return ctx->fail(FWI_ESTATE, "%s: call fwi_comm_init first", who);
    if (!vals || n < 1 || n > 8) return ctx->fail(FWI_EINVAL, "%s: n must be in [1, 8]", who);
    (void)hipSetDevice(ctx->cfg.device);
    HIPCHK(ctx, hipMemcpyAsync(ctx->red, vals, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    NCCLCHK(ctx, ncclAllReduce(ctx->red, ctx->red, (size_t)n, ncclFloat64, op, ctx->comm, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(vals, ctx->red, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return FWI_OK;
}

int fwi_allreduce_f64(fwi_ctx *ctx, double *vals, int32_t n) {
    return allreduce_scalars(ctx, vals, n, ncclSum, "fwi_allreduce_f64");
}

int fwi_allreduce_f64_max(fwi_ctx *ctx, double *vals, int32_t n) {
    return allreduce_scalars(ctx, vals, n, ncclMax, "fwi_allreduce_f64_max");
}

}  // extern "C"
