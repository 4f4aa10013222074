// C-ABI of the engine, first-arrival traveltimes (include/fwi.h: fwi_eikonal*, fwi_vec_scatter_points,
// fwi_vec_gather_points).  Host side only: argument checks, the launch loops of the three block-Jacobi iterations and
// their stopping rule.  Works on vector slots and the compact velocity; no sweep state is read or written.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "fwi_eikonal.h"
#include "fwi_eikonal_tangent.h"
#include "fwi_host.h"

namespace {

#include "fwi_eikonal_host.h"

template <typename T>
struct Impl : EikHost<T> {
    using EikHost<T>::upload_points;
    using EikHost<T>::iterate;

    static int eikonal(fwi_ctx *ctx, void *vt, void *vs, const std::vector<int64_t> &idx, const double *dist, int64_t ref,
                       int32_t max_sweeps, int32_t *launches_out) {
        const GridDesc &g = ctx->gd;
        T *t = (T *)vt, *sc = (T *)vs;
        const T *c = (const T *)ctx->c_dev;
        int rc = upload_points(ctx, idx, dist);
        if (rc) return rc;
        HIPCHK(ctx, launch_eikonal_fill<T>(g, t, ctx->stream));
        HIPCHK(ctx, launch_eikonal_fill<T>(g, sc, ctx->stream));
        HIPCHK(ctx, launch_eikonal_init<T>(t, sc, c, (const int64_t *)ctx->eik_idx.p, (const T *)ctx->eik_val.p, ref,
                                           (int)idx.size(), ctx->stream));
        const double h = ctx->cfg.h;
        hipStream_t s = ctx->stream;
        return iterate(ctx, "fwi_eikonal", t, sc, max_sweeps, launches_out, [&](T *in, T *out, int K, int *flag) {
            return launch_eikonal_sweep<T>(g, in, out, c, h, K, flag, s);
        });
    }

    static int adjoint(fwi_ctx *ctx, const void *vt, const void *vb, void *vl, void *vs, int32_t max_sweeps,
                       int32_t *launches_out) {
        const GridDesc &g = ctx->gd;
        const T *t = (const T *)vt, *b = (const T *)vb, *c = (const T *)ctx->c_dev;
        HIPCHK(ctx, hipMemcpyAsync(vl, vb, (size_t)g.npts * sizeof(T), hipMemcpyDeviceToDevice, ctx->stream));
        const double h = ctx->cfg.h;
        hipStream_t s = ctx->stream;
        return iterate(ctx, "fwi_eikonal_adjoint", (T *)vl, (T *)vs, max_sweeps, launches_out,
                       [&](T *in, T *out, int K, int *flag) {
                           return launch_eikonal_adjoint_sweep<T>(g, t, b, in, out, c, h, K, flag, s);
                       });
    }

    static int tangent(fwi_ctx *ctx, int32_t wrt, const void *vt, const void *vd, void *vo, void *vs,
                       const std::vector<int64_t> &idx, const double *dist, int64_t ref, int32_t max_sweeps,
                       int32_t *launches_out) {
        const GridDesc &g = ctx->gd;
        const T *t = (const T *)vt, *dm = (const T *)vd, *c = (const T *)ctx->c_dev;
        int rc = upload_points(ctx, idx, dist);
        if (rc) return rc;
        const double h = ctx->cfg.h;
        const int wv = wrt == FWI_WRT_VELOCITY;
        hipStream_t s = ctx->stream;
        HIPCHK(ctx, launch_eikonal_tangent_init<T>(g, t, dm, c, (T *)vo, (T *)vs, h, wv, (const int64_t *)ctx->eik_idx.p,
                                                   (const T *)ctx->eik_val.p, ref, (int)idx.size(), s));
        return iterate(ctx, "fwi_eikonal_tangent", (T *)vo, (T *)vs, max_sweeps, launches_out,
                       [&](T *in, T *out, int K, int *flag) {
                           return launch_eikonal_tangent_sweep<T>(g, t, dm, in, out, c, h, wv, K, flag, s);
                       });
    }

    static int gradient(fwi_ctx *ctx, int32_t wrt, const void *vt, const void *vl, void *vo, double beta,
                        const std::vector<int64_t> &idx, const double *dist, int64_t ref) {
        int rc = upload_points(ctx, idx, dist);
        if (rc) return rc;
        HIPCHK(ctx, launch_eikonal_gradient<T>(ctx->gd, (const T *)vt, (const T *)vl, (const T *)ctx->c_dev, (T *)vo,
                                               ctx->cfg.h, beta, wrt == FWI_WRT_VELOCITY, (const int64_t *)ctx->eik_idx.p,
                                               (const T *)ctx->eik_val.p, ref, (int)idx.size(), ctx->stream));
        return FWI_OK;
    }

    static int scatter(fwi_ctx *ctx, void *vx, const std::vector<int64_t> &idx, const double *val, double beta) {
        int rc = idx.empty() ? FWI_OK : upload_points(ctx, idx, val);
        if (rc) return rc;
        HIPCHK(ctx, launch_scatter_points<T>((T *)vx, ctx->gd.npts, beta, (const int64_t *)ctx->eik_idx.p,
                                             (const T *)ctx->eik_val.p, (int)idx.size(), ctx->stream));
        return FWI_OK;
    }

    static int gather(fwi_ctx *ctx, const void *vx, const std::vector<int64_t> &idx, double *out) {
        const size_t n = idx.size();
        int rc = upload_points(ctx, idx, nullptr);
        if (rc || (rc = ensure(ctx, ctx->eik_out, n * sizeof(double)))) return rc;
        HIPCHK(ctx, launch_gather_points<T>((const T *)vx, (const int64_t *)ctx->eik_idx.p, (double *)ctx->eik_out.p,
                                            (int)n, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(out, ctx->eik_out.p, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        return FWI_OK;
    }
};

}  // namespace

extern "C" {

int fwi_vec_scatter_points(fwi_ctx *ctx, int32_t slot, int32_t n, const int32_t *idx, const double *values, double beta) {
    if (!ctx) return FWI_EINVAL;
    VEC_OR_FAIL(ctx, vx, slot);
    if (n < 0) return ctx->fail(FWI_EINVAL, "fwi_vec_scatter_points: n = %d must be >= 0", (int)n);
    if (n > 0 && (!idx || !values)) return ctx->fail(FWI_EINVAL, "fwi_vec_scatter_points: null %s", !idx ? "idx" : "values");
    if (!std::isfinite(beta)) return ctx->fail(FWI_EINVAL, "fwi_vec_scatter_points: beta = %g must be finite", beta);
    for (int32_t k = 0; k < n; ++k)
        if (!std::isfinite(values[k]))
            return ctx->fail(FWI_EINVAL, "fwi_vec_scatter_points: values[%d] = %g must be finite", (int)k, values[k]);
    std::vector<int64_t> nodes;
    int rc = compact_nodes(ctx, "fwi_vec_scatter_points", "idx", n, idx, true, nodes);
    if (rc) return rc;
    (void)hipSetDevice(ctx->cfg.device);
    return DISPATCH_CALL(ctx, scatter, vx, nodes, values, beta);
}

int fwi_vec_gather_points(fwi_ctx *ctx, int32_t slot, int32_t n, const int32_t *idx, double *out) {
    if (!ctx) return FWI_EINVAL;
    VEC_OR_FAIL(ctx, vx, slot);
    if (n < 0) return ctx->fail(FWI_EINVAL, "fwi_vec_gather_points: n = %d must be >= 0", (int)n);
    if (n == 0) return FWI_OK;
    if (!idx || !out) return ctx->fail(FWI_EINVAL, "fwi_vec_gather_points: null %s", !idx ? "idx" : "out");
    std::vector<int64_t> nodes;
    int rc = compact_nodes(ctx, "fwi_vec_gather_points", "idx", n, idx, false, nodes);
    if (rc) return rc;
    (void)hipSetDevice(ctx->cfg.device);
    return DISPATCH_CALL(ctx, gather, vx, nodes, out);
}

int fwi_eikonal(fwi_ctx *ctx, int32_t t_slot, int32_t scratch_slot, int32_t n_init, const int32_t *init_idx,
                const double *init_dist, const int32_t *ref_idx, int32_t max_sweeps, int32_t *launches_out) {
    if (!ctx) return FWI_EINVAL;
    VEC_OR_FAIL(ctx, vt, t_slot);
    VEC_OR_FAIL(ctx, vs, scratch_slot);
    if (vt == vs) return ctx->fail(FWI_EINVAL, "fwi_eikonal: scratch_slot is t_slot (slot %d)", (int)t_slot);
    std::vector<int64_t> nodes;
    int64_t ref = 0;
    int rc = init_list(ctx, "fwi_eikonal", n_init, init_idx, init_dist, ref_idx, nodes, &ref);
    if (rc) return rc;
    if (!ctx->have_model) return ctx->fail(FWI_ESTATE, "fwi_eikonal: no model set");
    (void)hipSetDevice(ctx->cfg.device);
    return DISPATCH_CALL(ctx, eikonal, vt, vs, nodes, init_dist, ref, max_sweeps, launches_out);
}

int fwi_eikonal_adjoint(fwi_ctx *ctx, int32_t t_slot, int32_t rhs_slot, int32_t lam_slot, int32_t scratch_slot,
                        int32_t max_sweeps, int32_t *launches_out) {
    if (!ctx) return FWI_EINVAL;
    VEC_OR_FAIL(ctx, vt, t_slot);
    VEC_OR_FAIL(ctx, vb, rhs_slot);
    VEC_OR_FAIL(ctx, vl, lam_slot);
    VEC_OR_FAIL(ctx, vs, scratch_slot);
    if (vt == vb || vt == vl || vt == vs || vb == vl || vb == vs || vl == vs)
        return ctx->fail(FWI_EINVAL, "fwi_eikonal_adjoint: t, rhs, lam and scratch must be four different slots "
                         "(got %d, %d, %d, %d)", (int)t_slot, (int)rhs_slot, (int)lam_slot, (int)scratch_slot);
    if (!ctx->have_model) return ctx->fail(FWI_ESTATE, "fwi_eikonal_adjoint: no model set");
    (void)hipSetDevice(ctx->cfg.device);
    return DISPATCH_CALL(ctx, adjoint, vt, vb, vl, vs, max_sweeps, launches_out);
}

int fwi_eikonal_gradient(fwi_ctx *ctx, int32_t wrt, int32_t t_slot, int32_t lam_slot, int32_t out_slot, double beta,
                         int32_t n_init, const int32_t *init_idx, const double *init_dist, const int32_t *ref_idx) {
    if (!ctx) return FWI_EINVAL;
    VEC_OR_FAIL(ctx, vt, t_slot);
    VEC_OR_FAIL(ctx, vl, lam_slot);
    VEC_OR_FAIL(ctx, vo, out_slot);
    if (wrt != FWI_WRT_VELOCITY && wrt != FWI_WRT_SLOWNESS2)
        return ctx->fail(FWI_EINVAL, "fwi_eikonal_gradient: unknown parametrisation %d", (int)wrt);
    if (vo == vt || vo == vl)
        return ctx->fail(FWI_EINVAL, "fwi_eikonal_gradient: out (slot %d) must not alias %s", (int)out_slot,
                         vo == vt ? "t" : "lam");
    if (!std::isfinite(beta)) return ctx->fail(FWI_EINVAL, "fwi_eikonal_gradient: beta = %g must be finite", beta);
    std::vector<int64_t> nodes;
    int64_t ref = 0;
    int rc = init_list(ctx, "fwi_eikonal_gradient", n_init, init_idx, init_dist, ref_idx, nodes, &ref);
    if (rc) return rc;
    if (!ctx->have_model) return ctx->fail(FWI_ESTATE, "fwi_eikonal_gradient: no model set");
    (void)hipSetDevice(ctx->cfg.device);
    return DISPATCH_CALL(ctx, gradient, wrt, vt, vl, vo, beta, nodes, init_dist, ref);
}

int fwi_eikonal_tangent(fwi_ctx *ctx, int32_t wrt, int32_t t_slot, int32_t dm_slot, int32_t out_slot,
                        int32_t scratch_slot, int32_t n_init, const int32_t *init_idx, const double *init_dist,
                        const int32_t *ref_idx, int32_t max_sweeps, int32_t *launches_out) {
    if (!ctx) return FWI_EINVAL;
    VEC_OR_FAIL(ctx, vt, t_slot);
    VEC_OR_FAIL(ctx, vd, dm_slot);
    VEC_OR_FAIL(ctx, vo, out_slot);
    VEC_OR_FAIL(ctx, vs, scratch_slot);
    if (wrt != FWI_WRT_VELOCITY && wrt != FWI_WRT_SLOWNESS2)
        return ctx->fail(FWI_EINVAL, "fwi_eikonal_tangent: unknown parametrisation wrt = %d", (int)wrt);
    if (vt == vd || vt == vo || vt == vs || vd == vo || vd == vs || vo == vs)
        return ctx->fail(FWI_EINVAL, "fwi_eikonal_tangent: t_slot, dm_slot, out_slot and scratch_slot must be four "
                         "different slots (got %d, %d, %d, %d)", (int)t_slot, (int)dm_slot, (int)out_slot, (int)scratch_slot);
    std::vector<int64_t> nodes;
    int64_t ref = 0;
    int rc = init_list(ctx, "fwi_eikonal_tangent", n_init, init_idx, init_dist, ref_idx, nodes, &ref);
    if (rc) return rc;
    if (!ctx->have_model) return ctx->fail(FWI_ESTATE, "fwi_eikonal_tangent: no model set");
    (void)hipSetDevice(ctx->cfg.device);
    return DISPATCH_CALL(ctx, tangent, wrt, vt, vd, vo, vs, nodes, init_dist, ref, max_sweeps, launches_out);
}

}  // extern "C"
