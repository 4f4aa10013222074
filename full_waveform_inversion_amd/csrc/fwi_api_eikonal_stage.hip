// C-ABI of the engine, walled and slot-started eikonal solves and the pieces that chain two of them into a reflection
// (include/fwi.h: fwi_eikonal_stage, fwi_eikonal_handover, fwi_eikonal_gradient_field, fwi_eikonal_tangent_stage).  Host
// side only: argument checks and the launch loops, which are those of fwi_api_eikonal.hip (fwi_eikonal_host.h).  Works
// on vector slots and the compact velocity; no sweep state is read or written.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "fwi_eikonal.h"
#include "fwi_eikonal_stage.h"
#include "fwi_eikonal_tangent.h"
#include "fwi_host.h"

namespace {

#include "fwi_eikonal_host.h"

template <typename T>
struct Impl : EikHost<T> {
    using EikHost<T>::upload_points;
    using EikHost<T>::iterate;

    // FWI_EINVAL unless the start in `vt` is free of NaNs and negative entries and holds a finite one, outside the wall
    static int check_start(fwi_ctx *ctx, const void *vt, const void *vw) {
        int rc = ensure(ctx, ctx->eik_flags, EIK_BATCH * sizeof(int));
        if (rc) return rc;
        int *flags = (int *)ctx->eik_flags.p, host[2];
        HIPCHK(ctx, hipMemsetAsync(flags, 0, 2 * sizeof(int), ctx->stream));
        HIPCHK(ctx, launch_eikonal_stage_check<T>(ctx->gd, (const T *)vt, (const T *)vw, flags, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(host, flags, 2 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        if (host[0]) return ctx->fail(FWI_EINVAL, "fwi_eikonal_stage: t_slot holds a NaN or a negative entry");
        if (!host[1]) return ctx->fail(FWI_EINVAL, "fwi_eikonal_stage: t_slot holds no finite entry: there is no source");
        return FWI_OK;
    }

    static int stage(fwi_ctx *ctx, void *vt, void *vs, const void *vw, const std::vector<int64_t> &idx,
                     const double *dist, int64_t ref, int32_t max_sweeps, int32_t *launches_out) {
        const GridDesc &g = ctx->gd;
        T *t = (T *)vt, *sc = (T *)vs;
        const T *c = (const T *)ctx->c_dev, *wall = (const T *)vw;
        int rc;
        if (idx.empty()) {
            if ((rc = check_start(ctx, vt, vw))) return rc;
        } else {
            if ((rc = upload_points(ctx, idx, dist))) return rc;
            HIPCHK(ctx, launch_eikonal_fill<T>(g, t, ctx->stream));
            HIPCHK(ctx, launch_eikonal_fill<T>(g, sc, ctx->stream));
            HIPCHK(ctx, launch_eikonal_init<T>(t, sc, c, (const int64_t *)ctx->eik_idx.p, (const T *)ctx->eik_val.p, ref,
                                               (int)idx.size(), ctx->stream));
        }
        if (idx.empty() || wall) HIPCHK(ctx, launch_eikonal_stage_start<T>(g, t, sc, wall, ctx->stream));
        const double h = ctx->cfg.h;
        hipStream_t s = ctx->stream;
        if (!wall)  // the launches of fwi_eikonal
            return iterate(ctx, "fwi_eikonal_stage", t, sc, max_sweeps, launches_out, [&](T *in, T *out, int K, int *flag) {
                return launch_eikonal_sweep<T>(g, in, out, c, h, K, flag, s);
            });
        return iterate(ctx, "fwi_eikonal_stage", t, sc, max_sweeps, launches_out, [&](T *in, T *out, int K, int *flag) {
            return launch_eikonal_stage_sweep<T>(g, in, out, c, wall, h, K, flag, s);
        });
    }

    static int handover(fwi_ctx *ctx, const void *vt, const void *vi, void *vo, double beta) {
        HIPCHK(ctx, launch_eikonal_handover<T>(ctx->gd, (const T *)vt, (const T *)vi, (const T *)ctx->c_dev, (T *)vo,
                                               ctx->cfg.h, beta, ctx->stream));
        return FWI_OK;
    }

    static int gradient_field(fwi_ctx *ctx, int32_t wrt, const void *vt, const void *vl, void *vo, double beta) {
        HIPCHK(ctx, launch_eikonal_gradient<T>(ctx->gd, (const T *)vt, (const T *)vl, (const T *)ctx->c_dev, (T *)vo,
                                               ctx->cfg.h, beta, wrt == FWI_WRT_VELOCITY, nullptr, nullptr, 0, 0,
                                               ctx->stream));
        return FWI_OK;
    }

    static int tangent(fwi_ctx *ctx, int32_t wrt, const void *vt, const void *vd, const void *vb, void *vo, void *vs,
                       const std::vector<int64_t> &idx, const double *dist, int64_t ref, int32_t max_sweeps,
                       int32_t *launches_out) {
        const GridDesc &g = ctx->gd;
        const T *t = (const T *)vt, *dm = (const T *)vd, *b0 = (const T *)vb, *c = (const T *)ctx->c_dev;
        int rc = idx.empty() ? FWI_OK : upload_points(ctx, idx, dist);
        if (rc) return rc;
        const double h = ctx->cfg.h;
        const int wv = wrt == FWI_WRT_VELOCITY;
        hipStream_t s = ctx->stream;
        HIPCHK(ctx, launch_eikonal_stage_tangent_init<T>(g, t, dm, b0, c, (T *)vo, (T *)vs, h, wv,
                                                         (const int64_t *)ctx->eik_idx.p, (const T *)ctx->eik_val.p, ref,
                                                         (int)idx.size(), s));
        if (!b0)  // the launches of fwi_eikonal_tangent
            return iterate(ctx, "fwi_eikonal_tangent_stage", (T *)vo, (T *)vs, max_sweeps, launches_out,
                           [&](T *in, T *out, int K, int *flag) {
                               return launch_eikonal_tangent_sweep<T>(g, t, dm, in, out, c, h, wv, K, flag, s);
                           });
        return iterate(ctx, "fwi_eikonal_tangent_stage", (T *)vo, (T *)vs, max_sweeps, launches_out,
                       [&](T *in, T *out, int K, int *flag) {
                           return launch_eikonal_stage_tangent_sweep<T>(g, t, dm, b0, in, out, c, h, wv, K, flag, s);
                       });
    }
};

// FWI_EINVAL, naming the later of the two, when two of the n named slots are the same one
int distinct_slots(fwi_ctx *ctx, const char *who, int n, void *const *p, const char *const *name, const int32_t *slot) {
    for (int i = 1; i < n; ++i)
        for (int j = 0; j < i; ++j)
            if (p[i] && p[i] == p[j])
                return ctx->fail(FWI_EINVAL, "%s: %s is %s (slot %d)", who, name[i], name[j], (int)slot[i]);
    return FWI_OK;
}

}  // namespace

extern "C" {

int fwi_eikonal_stage(fwi_ctx *ctx, int32_t t_slot, int32_t scratch_slot, int32_t wall_slot, int32_t n_init,
                      const int32_t *init_idx, const double *init_dist, const int32_t *ref_idx, int32_t max_sweeps,
                      int32_t *launches_out) {
    if (!ctx) return FWI_EINVAL;
    VEC_OR_FAIL(ctx, vt, t_slot);
    VEC_OR_FAIL(ctx, vs, scratch_slot);
    void *vw = nullptr;
    if (wall_slot != -1 && !(vw = vec_slot(ctx, wall_slot)))
        return ctx->fail(FWI_EINVAL, "fwi_eikonal_stage: wall_slot: vector slot %d does not exist", (int)wall_slot);
    void *const p[] = {vt, vs, vw};
    const char *const names[] = {"t_slot", "scratch_slot", "wall_slot"};
    const int32_t slots[] = {t_slot, scratch_slot, wall_slot};
    int rc = distinct_slots(ctx, "fwi_eikonal_stage", 3, p, names, slots);
    if (rc) return rc;
    if (n_init < 0) return ctx->fail(FWI_EINVAL, "fwi_eikonal_stage: n_init = %d must be >= 0", (int)n_init);
    std::vector<int64_t> nodes;
    int64_t ref = 0;
    if (n_init > 0 && (rc = init_list(ctx, "fwi_eikonal_stage", n_init, init_idx, init_dist, ref_idx, nodes, &ref)))
        return rc;
    if (!ctx->have_model) return ctx->fail(FWI_ESTATE, "fwi_eikonal_stage: no model set");
    (void)hipSetDevice(ctx->cfg.device);
    return DISPATCH_CALL(ctx, stage, vt, vs, vw, nodes, init_dist, ref, max_sweeps, launches_out);
}

int fwi_eikonal_handover(fwi_ctx *ctx, int32_t t_slot, int32_t in_slot, int32_t out_slot, double beta) {
    if (!ctx) return FWI_EINVAL;
    VEC_OR_FAIL(ctx, vt, t_slot);
    VEC_OR_FAIL(ctx, vi, in_slot);
    VEC_OR_FAIL(ctx, vo, out_slot);
    void *const p[] = {vt, vi, vo};
    const char *const names[] = {"t_slot", "in_slot", "out_slot"};
    const int32_t slots[] = {t_slot, in_slot, out_slot};
    int rc = distinct_slots(ctx, "fwi_eikonal_handover", 3, p, names, slots);
    if (rc) return rc;
    if (!std::isfinite(beta)) return ctx->fail(FWI_EINVAL, "fwi_eikonal_handover: beta = %g must be finite", beta);
    if (!ctx->have_model) return ctx->fail(FWI_ESTATE, "fwi_eikonal_handover: no model set");
    (void)hipSetDevice(ctx->cfg.device);
    return DISPATCH_CALL(ctx, handover, vt, vi, vo, beta);
}

int fwi_eikonal_gradient_field(fwi_ctx *ctx, int32_t wrt, int32_t t_slot, int32_t lam_slot, int32_t out_slot,
                               double beta) {
    if (!ctx) return FWI_EINVAL;
    VEC_OR_FAIL(ctx, vt, t_slot);
    VEC_OR_FAIL(ctx, vl, lam_slot);
    VEC_OR_FAIL(ctx, vo, out_slot);
    if (wrt != FWI_WRT_VELOCITY && wrt != FWI_WRT_SLOWNESS2)
        return ctx->fail(FWI_EINVAL, "fwi_eikonal_gradient_field: unknown parametrisation wrt = %d", (int)wrt);
    if (vo == vt || vo == vl)
        return ctx->fail(FWI_EINVAL, "fwi_eikonal_gradient_field: out_slot is %s (slot %d)", vo == vt ? "t_slot" : "lam_slot",
                         (int)out_slot);
    if (!std::isfinite(beta)) return ctx->fail(FWI_EINVAL, "fwi_eikonal_gradient_field: beta = %g must be finite", beta);
    if (!ctx->have_model) return ctx->fail(FWI_ESTATE, "fwi_eikonal_gradient_field: no model set");
    (void)hipSetDevice(ctx->cfg.device);
    return DISPATCH_CALL(ctx, gradient_field, wrt, vt, vl, vo, beta);
}

int fwi_eikonal_tangent_stage(fwi_ctx *ctx, int32_t wrt, int32_t t_slot, int32_t dm_slot, int32_t b0_slot,
                              int32_t out_slot, int32_t scratch_slot, int32_t n_init, const int32_t *init_idx,
                              const double *init_dist, const int32_t *ref_idx, int32_t max_sweeps,
                              int32_t *launches_out) {
    if (!ctx) return FWI_EINVAL;
    VEC_OR_FAIL(ctx, vt, t_slot);
    VEC_OR_FAIL(ctx, vd, dm_slot);
    VEC_OR_FAIL(ctx, vo, out_slot);
    VEC_OR_FAIL(ctx, vs, scratch_slot);
    void *vb = nullptr;
    if (b0_slot != -1 && !(vb = vec_slot(ctx, b0_slot)))
        return ctx->fail(FWI_EINVAL, "fwi_eikonal_tangent_stage: b0_slot: vector slot %d does not exist", (int)b0_slot);
    if (wrt != FWI_WRT_VELOCITY && wrt != FWI_WRT_SLOWNESS2)
        return ctx->fail(FWI_EINVAL, "fwi_eikonal_tangent_stage: unknown parametrisation wrt = %d", (int)wrt);
    void *const p[] = {vt, vd, vb, vo, vs};
    const char *const names[] = {"t_slot", "dm_slot", "b0_slot", "out_slot", "scratch_slot"};
    const int32_t slots[] = {t_slot, dm_slot, b0_slot, out_slot, scratch_slot};
    int rc = distinct_slots(ctx, "fwi_eikonal_tangent_stage", 5, p, names, slots);
    if (rc) return rc;
    if (n_init < 0) return ctx->fail(FWI_EINVAL, "fwi_eikonal_tangent_stage: n_init = %d must be >= 0", (int)n_init);
    std::vector<int64_t> nodes;
    int64_t ref = 0;
    if (n_init > 0 &&
        (rc = init_list(ctx, "fwi_eikonal_tangent_stage", n_init, init_idx, init_dist, ref_idx, nodes, &ref)))
        return rc;
    if (!ctx->have_model) return ctx->fail(FWI_ESTATE, "fwi_eikonal_tangent_stage: no model set");
    (void)hipSetDevice(ctx->cfg.device);
    return DISPATCH_CALL(ctx, tangent, wrt, vt, vd, vb, vo, vs, nodes, init_dist, ref, max_sweeps, launches_out);
}

}  // extern "C"
