// C-ABI of the engine, the model-space vectors (include/fwi.h: fwi_vec_*, fwi_dot) and what reads the gradient and
// illumination accumulators into them or into the caller's arrays.  Host side only; no time loop runs here.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "fwi_host.h"
#include "fwi_illum.h"
#include "fwi_reg.h"
#include "fwi_slant.h"
#include "fwi_smooth.h"

namespace {

template <typename T>
struct Impl {
    // H_m = (S / dt^4) acc (the per-step factor of the gradient, S / dt^2, times the 1 / dt^2 of q ~ dt^2 d2u/dt2),
    // H_c = H_m (2 / c^3)^2, into the compact device array `dev`
    static int illumination_vec(fwi_ctx *ctx, int32_t wrt, void *dev) {
        const double dt2 = ctx->cfg.dt * ctx->cfg.dt;
        HIPCHK(ctx, launch_illum_finalize<T>(ctx->gd, (const T *)ctx->h_acc, (const T *)ctx->c_dev, (T *)dev,
                                             (double)ctx->istride / (dt2 * dt2), wrt == FWI_WRT_VELOCITY, ctx->stream));
        return FWI_OK;
    }

    static int illumination(fwi_ctx *ctx, int32_t wrt, T *out) {
        int rc = illumination_vec(ctx, wrt, ctx->g_out);
        if (rc || (rc = download_compact<T>(ctx, out, ctx->g_out))) return rc;
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        return FWI_OK;
    }

    static int gradient_vec(fwi_ctx *ctx, int32_t wrt, void *dev) {
        const double scale = -(double)ctx->istride / (ctx->cfg.dt * ctx->cfg.dt);  // istride: quadrature weight
        HIPCHK(ctx, launch_finalize_gradient<T>(ctx->gd, (const T *)ctx->g_acc, (const T *)ctx->c_dev, (T *)dev, scale,
                                                wrt == FWI_WRT_VELOCITY, ctx->stream));
        return FWI_OK;
    }

    static int vec_dot(fwi_ctx *ctx, const void *x, const void *y, double *out) {
        double *part;
        int rc = sum_partials(ctx, &part);
        if (rc) return rc;
        HIPCHK(ctx, launch_dot<T>((const T *)x, (const T *)y, ctx->gd.npts, part, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(out, part + sum_blocks(ctx->gd.npts), sizeof(double), hipMemcpyDeviceToHost,
                                   ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        return FWI_OK;
    }

    static int vec_absmax(fwi_ctx *ctx, const void *x, double *out) {
        HIPCHK(ctx, hipMemsetAsync(ctx->red, 0, sizeof(double), ctx->stream));
        HIPCHK(ctx, launch_absmax<T>((const T *)x, ctx->gd.npts, ctx->red, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(out, ctx->red, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        return FWI_OK;
    }

    static int vec_axpby(fwi_ctx *ctx, void *y, double a, const void *x, double b) {
        HIPCHK(ctx, launch_axpby<T>((T *)y, a, (const T *)x, b, ctx->gd.npts, ctx->stream));
        return FWI_OK;
    }

    static int vec_clip(fwi_ctx *ctx, void *x, double lo, double hi) {
        HIPCHK(ctx, launch_clip<T>(ctx->gd, (T *)x, lo, hi, ctx->stream));
        return FWI_OK;
    }

    static int gradient(fwi_ctx *ctx, int32_t wrt, T *out) {
        const GridDesc &g = ctx->gd;
        const double scale = -(double)ctx->istride / (ctx->cfg.dt * ctx->cfg.dt);  // istride: quadrature weight
        HIPCHK(ctx, launch_finalize_gradient<T>(g, (const T *)ctx->g_acc, (const T *)ctx->c_dev,
                                                (T *)ctx->g_out, scale, wrt == FWI_WRT_VELOCITY, ctx->stream));
        int rc = download_compact<T>(ctx, out, ctx->g_out);
        if (rc) return rc;
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        return FWI_OK;
    }

    static int dot(fwi_ctx *ctx, const T *a, const T *b, int64_t n, double *out) {
        double *part;
        int rc = sum_partials(ctx, &part);
        if (rc) return rc;
        void *da = nullptr, *db = nullptr;
        HIPCHK(ctx, hipMalloc(&da, (size_t)n * sizeof(T)));
        hipError_t e = hipMalloc(&db, (size_t)n * sizeof(T));
        if (e != hipSuccess) {
            (void)hipFree(da);
            return ctx->fail(FWI_ENOMEM, "hipMalloc: %s", hipGetErrorString(e));
        }
        do {
            if ((e = hipMemcpyAsync(da, a, (size_t)n * sizeof(T), hipMemcpyHostToDevice, ctx->stream))) break;
            if ((e = hipMemcpyAsync(db, b, (size_t)n * sizeof(T), hipMemcpyHostToDevice, ctx->stream))) break;
            if ((e = launch_dot<T>((const T *)da, (const T *)db, n, part, ctx->stream))) break;
            if ((e = hipMemcpyAsync(out, part + sum_blocks(n), sizeof(double), hipMemcpyDeviceToHost, ctx->stream))) break;
            e = hipStreamSynchronize(ctx->stream);
        } while (0);
        if (e != hipSuccess) rc = ctx->fail(FWI_EHIP, "fwi_dot: %s", hipGetErrorString(e));
        (void)hipFree(da);
        (void)hipFree(db);
        return rc;
    }
};

}  // namespace

template <typename T>
static int vec_smooth_passes(fwi_ctx *ctx, void *vy, const int *axis, const int *R, const double (*w)[SMOOTH_RMAX + 1],
                             int npass) {
    // ping-pong between the vector and the context's spare one; an odd number of passes ends in the spare: copied back
    T *cur = (T *)vy, *other = (T *)ctx->smooth_tmp;
    for (int p = 0; p < npass; ++p) {
        T wt[SMOOTH_RMAX + 1];
        for (int k = 0; k <= R[p]; ++k) wt[k] = (T)w[p][k];
        HIPCHK(ctx, launch_smooth_axis<T>(ctx->gd, other, cur, axis[p], R[p], wt, ctx->stream));
        std::swap(cur, other);
    }
    if (cur != (T *)vy)
        HIPCHK(ctx, hipMemcpyAsync(vy, cur, (size_t)ctx->gd.npts * sizeof(T), hipMemcpyDeviceToDevice, ctx->stream));
    return FWI_OK;
}

template <typename T>
static int vec_regularizer(fwi_ctx *ctx, int32_t kind, const void *x, const void *x0, const void *v, void *out,
                           double alpha, double beta, const double w[3], double eps, double *value_out) {
    const int64_t nb = reg_blocks<T>(ctx->gd);
    if (int rc = dev_first_use(ctx, &ctx->reg_part, (size_t)(nb + 1) * sizeof(double), "reg_part")) return rc;
    double *part = (double *)ctx->reg_part;
    HIPCHK(ctx, launch_regularizer<T>(ctx->gd, kind, (T *)out, (const T *)x, (const T *)x0, (const T *)v, alpha, beta, w,
                                      eps, part, ctx->stream));
    if (value_out) {
        HIPCHK(ctx, hipMemcpyAsync(value_out, part + nb, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    return FWI_OK;
}

extern "C" {

int fwi_gradient(fwi_ctx *ctx, int32_t wrt, void *g_out) {
    if (!ctx) return FWI_EINVAL;
    if (!g_out) return ctx->fail(FWI_EINVAL, "fwi_gradient: null output");
    if (wrt != FWI_WRT_VELOCITY && wrt != FWI_WRT_SLOWNESS2)
        return ctx->fail(FWI_EINVAL, "fwi_gradient: unknown parametrisation %d", wrt);
    if (!ctx->have_model) return ctx->fail(FWI_ESTATE, "fwi_gradient: no model set");
    (void)hipSetDevice(ctx->cfg.device);
    return DISPATCH(ctx, Impl<float>::gradient(ctx, wrt, (float *)g_out),
                    Impl<double>::gradient(ctx, wrt, (double *)g_out));
}

int fwi_gradient_reset(fwi_ctx *ctx) {
    if (!ctx) return FWI_EINVAL;
    (void)hipSetDevice(ctx->cfg.device);
    HIPCHK(ctx, hipMemsetAsync(ctx->g_acc, 0, (size_t)ctx->gd.npts * ctx->esize, ctx->stream));
    if (ctx->h_acc) HIPCHK(ctx, hipMemsetAsync(ctx->h_acc, 0, (size_t)ctx->gd.npts * ctx->esize, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return FWI_OK;
}

int fwi_gradient_add(fwi_ctx *dst, fwi_ctx *src) {
    if (!dst || !src) return FWI_EINVAL;
    if (dst == src) return dst->fail(FWI_EINVAL, "fwi_gradient_add: dst and src are the same context");
    if (dst->cfg.device != src->cfg.device || dst->cfg.dtype != src->cfg.dtype || dst->gd.npts != src->gd.npts ||
        dst->gd.nx != src->gd.nx || dst->gd.nz != src->gd.nz)
        return dst->fail(FWI_EINVAL, "fwi_gradient_add: contexts differ in device, dtype or shape");
    if (!dst->h_acc != !src->h_acc)
        return dst->fail(FWI_EINVAL, "fwi_gradient_add: illumination is enabled in one context only");
    (void)hipSetDevice(dst->cfg.device);
    HIPCHK(dst, hipStreamSynchronize(src->stream));  // src's adjoint sweeps are complete
    int rc = DISPATCH(dst, Impl<float>::vec_axpby(dst, dst->g_acc, 1.0, src->g_acc, 1.0),
                      Impl<double>::vec_axpby(dst, dst->g_acc, 1.0, src->g_acc, 1.0));
    if (rc) return rc;
    if (dst->h_acc && (rc = DISPATCH(dst, Impl<float>::vec_axpby(dst, dst->h_acc, 1.0, src->h_acc, 1.0),
                                     Impl<double>::vec_axpby(dst, dst->h_acc, 1.0, src->h_acc, 1.0))))
        return rc;
    HIPCHK(dst, hipStreamSynchronize(dst->stream));
    return FWI_OK;
}

int fwi_dot(fwi_ctx *ctx, const void *a, const void *b, int64_t n, double *out) {
    if (!ctx) return FWI_EINVAL;
    if (!a || !b || !out || n < 0) return ctx->fail(FWI_EINVAL, "fwi_dot: bad argument");
    if (n == 0) {
        *out = 0.0;
        return FWI_OK;
    }
    (void)hipSetDevice(ctx->cfg.device);
    return DISPATCH(ctx, Impl<float>::dot(ctx, (const float *)a, (const float *)b, n, out),
                    Impl<double>::dot(ctx, (const double *)a, (const double *)b, n, out));
}

int fwi_vec_create(fwi_ctx *ctx, int32_t count) {
    if (!ctx) return FWI_EINVAL;
    if (count < 0 || count > 256) return ctx->fail(FWI_EINVAL, "fwi_vec_create: count must be in [0, 256]");
    (void)hipSetDevice(ctx->cfg.device);
    for (void *&v : ctx->vecs) (void)ctx->mem.release(&v);
    ctx->vecs.assign(count, nullptr);
    const size_t bytes = (size_t)ctx->gd.npts * ctx->esize;
    for (int i = 0; i < count; ++i) {
        if (int rc = dev_acquire(ctx, &ctx->vecs[i], bytes, "vecs", i)) return rc;
        HIPCHK(ctx, hipMemsetAsync(ctx->vecs[i], 0, bytes, ctx->stream));
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return FWI_OK;
}

int fwi_vec_upload(fwi_ctx *ctx, int32_t slot, const void *host) {
    if (!ctx) return FWI_EINVAL;
    VEC_OR_FAIL(ctx, v, slot);
    if (!host) return ctx->fail(FWI_EINVAL, "fwi_vec_upload: null buffer");
    (void)hipSetDevice(ctx->cfg.device);
    int rc = DISPATCH(ctx, upload_compact<float>(ctx, v, host), upload_compact<double>(ctx, v, host));
    if (rc) return rc;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return FWI_OK;
}

int fwi_vec_download(fwi_ctx *ctx, int32_t slot, void *host) {
    if (!ctx) return FWI_EINVAL;
    VEC_OR_FAIL(ctx, v, slot);
    if (!host) return ctx->fail(FWI_EINVAL, "fwi_vec_download: null buffer");
    (void)hipSetDevice(ctx->cfg.device);
    int rc = DISPATCH(ctx, download_compact<float>(ctx, host, v), download_compact<double>(ctx, host, v));
    if (rc) return rc;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return FWI_OK;
}

int fwi_vec_copy(fwi_ctx *ctx, int32_t dst, int32_t src) {
    if (!ctx) return FWI_EINVAL;
    VEC_OR_FAIL(ctx, d, dst);
    VEC_OR_FAIL(ctx, s, src);
    (void)hipSetDevice(ctx->cfg.device);
    if (d != s)
        HIPCHK(ctx, hipMemcpyAsync(d, s, (size_t)ctx->gd.npts * ctx->esize, hipMemcpyDeviceToDevice, ctx->stream));
    return FWI_OK;
}

int fwi_vec_axpby(fwi_ctx *ctx, int32_t y, double a, int32_t x, double b) {
    if (!ctx) return FWI_EINVAL;
    VEC_OR_FAIL(ctx, vy, y);
    VEC_OR_FAIL(ctx, vx, x);
    (void)hipSetDevice(ctx->cfg.device);
    return DISPATCH(ctx, Impl<float>::vec_axpby(ctx, vy, a, vx, b), Impl<double>::vec_axpby(ctx, vy, a, vx, b));
}

int fwi_vec_dot(fwi_ctx *ctx, int32_t x, int32_t y, double *out) {
    if (!ctx) return FWI_EINVAL;
    VEC_OR_FAIL(ctx, vx, x);
    VEC_OR_FAIL(ctx, vy, y);
    if (!out) return ctx->fail(FWI_EINVAL, "fwi_vec_dot: null output");
    (void)hipSetDevice(ctx->cfg.device);
    return DISPATCH(ctx, Impl<float>::vec_dot(ctx, vx, vy, out), Impl<double>::vec_dot(ctx, vx, vy, out));
}

int fwi_vec_absmax(fwi_ctx *ctx, int32_t x, double *out) {
    if (!ctx) return FWI_EINVAL;
    VEC_OR_FAIL(ctx, vx, x);
    if (!out) return ctx->fail(FWI_EINVAL, "fwi_vec_absmax: null output");
    (void)hipSetDevice(ctx->cfg.device);
    return DISPATCH(ctx, Impl<float>::vec_absmax(ctx, vx, out), Impl<double>::vec_absmax(ctx, vx, out));
}

int fwi_vec_clip(fwi_ctx *ctx, int32_t x, double lo, double hi) {
    if (!ctx) return FWI_EINVAL;
    VEC_OR_FAIL(ctx, vx, x);
    if (!(lo <= hi)) return ctx->fail(FWI_EINVAL, "fwi_vec_clip: lo > hi");
    (void)hipSetDevice(ctx->cfg.device);
    return DISPATCH(ctx, Impl<float>::vec_clip(ctx, vx, lo, hi), Impl<double>::vec_clip(ctx, vx, lo, hi));
}

int fwi_gradient_vec(fwi_ctx *ctx, int32_t wrt, int32_t slot) {
    if (!ctx) return FWI_EINVAL;
    VEC_OR_FAIL(ctx, v, slot);
    if (wrt != FWI_WRT_VELOCITY && wrt != FWI_WRT_SLOWNESS2)
        return ctx->fail(FWI_EINVAL, "fwi_gradient_vec: unknown parametrisation %d", wrt);
    if (!ctx->have_model) return ctx->fail(FWI_ESTATE, "fwi_gradient_vec: no model set");
    (void)hipSetDevice(ctx->cfg.device);
    return DISPATCH(ctx, Impl<float>::gradient_vec(ctx, wrt, v), Impl<double>::gradient_vec(ctx, wrt, v));
}

#define ILLUM_READABLE(ctx, who, wrt)                                                                              \
    do {                                                                                                           \
        if ((wrt) != FWI_WRT_VELOCITY && (wrt) != FWI_WRT_SLOWNESS2)                                               \
            return (ctx)->fail(FWI_EINVAL, "%s: unknown parametrisation %d", who, (int)(wrt));                     \
        if (!(ctx)->h_acc) return (ctx)->fail(FWI_ESTATE, "%s: illumination is disabled (fwi_set_illumination)", who); \
        if (!(ctx)->have_model) return (ctx)->fail(FWI_ESTATE, "%s: no model set", who);                          \
    } while (0)

int fwi_illumination(fwi_ctx *ctx, int32_t wrt, void *out) {
    if (!ctx) return FWI_EINVAL;
    if (!out) return ctx->fail(FWI_EINVAL, "fwi_illumination: null output");
    ILLUM_READABLE(ctx, "fwi_illumination", wrt);
    (void)hipSetDevice(ctx->cfg.device);
    return DISPATCH(ctx, Impl<float>::illumination(ctx, wrt, (float *)out),
                    Impl<double>::illumination(ctx, wrt, (double *)out));
}

int fwi_illumination_vec(fwi_ctx *ctx, int32_t wrt, int32_t slot) {
    if (!ctx) return FWI_EINVAL;
    VEC_OR_FAIL(ctx, v, slot);
    ILLUM_READABLE(ctx, "fwi_illumination_vec", wrt);
    (void)hipSetDevice(ctx->cfg.device);
    return DISPATCH(ctx, Impl<float>::illumination_vec(ctx, wrt, v), Impl<double>::illumination_vec(ctx, wrt, v));
}

int fwi_vec_mul(fwi_ctx *ctx, int32_t y, int32_t x) {
    if (!ctx) return FWI_EINVAL;
    VEC_OR_FAIL(ctx, vy, y);
    VEC_OR_FAIL(ctx, vx, x);
    (void)hipSetDevice(ctx->cfg.device);
    HIPCHK(ctx, DISPATCH(ctx, launch_vec_mul<float>(ctx->gd, (float *)vy, (const float *)vx, ctx->stream),
                         launch_vec_mul<double>(ctx->gd, (double *)vy, (const double *)vx, ctx->stream)));
    return FWI_OK;
}

int fwi_vec_recip(fwi_ctx *ctx, int32_t y, double a, double b) {
    if (!ctx) return FWI_EINVAL;
    VEC_OR_FAIL(ctx, vy, y);
    (void)hipSetDevice(ctx->cfg.device);
    HIPCHK(ctx, DISPATCH(ctx, launch_vec_recip<float>(ctx->gd, (float *)vy, a, b, ctx->stream),
                         launch_vec_recip<double>(ctx->gd, (double *)vy, a, b, ctx->stream)));
    return FWI_OK;
}

int fwi_vec_smooth(fwi_ctx *ctx, int32_t y, const double *sigma) {
    if (!ctx) return FWI_EINVAL;
    VEC_OR_FAIL(ctx, vy, y);
    if (!sigma) return ctx->fail(FWI_EINVAL, "fwi_vec_smooth: null sigma");
    const GridDesc &g = ctx->gd;
    const int nd = g.ndim;
    int axis[3], R[3], npass = 0;
    double w[3][SMOOTH_RMAX + 1];
    // applied in the order x, y, z; sigma is in grid order (z, [y,] x)
    for (int d = nd - 1; d >= 0; --d) {
        const double sg = sigma[d];
        const int ax = (nd == 2 && d == 1) ? 2 : d;  // internal axis: 0 = z, 1 = y, 2 = x
        const int n = ax == 0 ? g.nz : ax == 1 ? g.ny : g.nx;
        if (!std::isfinite(sg) || sg < 0.0)
            return ctx->fail(FWI_EINVAL, "fwi_vec_smooth: sigma[%d] = %g must be finite and >= 0", d, sg);
        if (3.0 * sg + 0.5 >= (double)(SMOOTH_RMAX + 1))
            return ctx->fail(FWI_EINVAL, "fwi_vec_smooth: sigma[%d] = %g gives a radius above %d (apply the operator twice)",
                             d, sg, SMOOTH_RMAX);
        const int r = smooth_radius(sg);
        if (r > n)
            return ctx->fail(FWI_EINVAL, "fwi_vec_smooth: sigma[%d] = %g gives radius %d, the axis has %d cells "
                             "(one reflection only)", d, sg, r, n);
        if (r == 0) continue;  // the identity on this axis: no launch
        axis[npass] = ax;
        R[npass] = r;
        smooth_weights(sg, r, w[npass]);
        ++npass;
    }
    if (npass == 0) return FWI_OK;
    (void)hipSetDevice(ctx->cfg.device);
    if (int rc = dev_first_use(ctx, &ctx->smooth_tmp, (size_t)g.npts * ctx->esize, "smooth_tmp")) return rc;
    return DISPATCH(ctx, vec_smooth_passes<float>(ctx, vy, axis, R, w, npass),
                    vec_smooth_passes<double>(ctx, vy, axis, R, w, npass));
}

int fwi_vec_shift_sum(fwi_ctx *ctx, int32_t dst, int32_t nsrc, const int32_t *src_slots, const double *shifts,
                      const double *weights, double beta) {
    if (!ctx) return FWI_EINVAL;
    void *vd = vec_slot(ctx, dst);
    if (!vd) return ctx->fail(FWI_EINVAL, "fwi_vec_shift_sum: dst: vector slot %d does not exist", (int)dst);
    if (nsrc < 1 || nsrc > FWI_SHIFT_SUM_MAX)
        return ctx->fail(FWI_EINVAL, "fwi_vec_shift_sum: nsrc = %d must be in [1, %d]", (int)nsrc, FWI_SHIFT_SUM_MAX);
    if (!src_slots) return ctx->fail(FWI_EINVAL, "fwi_vec_shift_sum: null src_slots");
    if (!shifts) return ctx->fail(FWI_EINVAL, "fwi_vec_shift_sum: null shifts");
    if (!std::isfinite(beta)) return ctx->fail(FWI_EINVAL, "fwi_vec_shift_sum: beta = %g must be finite", beta);
    static_assert(FWI_SHIFT_SUM_MAX == SLANT_MAX, "include/fwi.h and fwi_slant.h disagree");
    const GridDesc &g = ctx->gd;
    SlantTable t = {};
    int kept = 0;
    for (int i = 0; i < nsrc; ++i) {
        const void *vs = vec_slot(ctx, src_slots[i]);
        const double s = shifts[i], w = weights ? weights[i] : 1.0;
        if (!vs)
            return ctx->fail(FWI_EINVAL, "fwi_vec_shift_sum: src_slots[%d]: vector slot %d does not exist", i,
                             (int)src_slots[i]);
        if (vs == vd)
            return ctx->fail(FWI_EINVAL, "fwi_vec_shift_sum: src_slots[%d] is dst (slot %d)", i, (int)dst);
        if (!std::isfinite(s)) return ctx->fail(FWI_EINVAL, "fwi_vec_shift_sum: shifts[%d] = %g must be finite", i, s);
        if (!std::isfinite(w)) return ctx->fail(FWI_EINVAL, "fwi_vec_shift_sum: weights[%d] = %g must be finite", i, w);
        if (std::fabs(s) >= (double)g.nz + 1.0) continue;  // wholly outside the grid: tested before n is formed
        const double n = std::floor(s), f = s - n;
        t.src[kept] = vs;
        t.n[kept] = (int64_t)n;
        t.c0[kept] = w * (1.0 - f);
        t.c1[kept] = w * f;
        ++kept;
    }
    (void)hipSetDevice(ctx->cfg.device);
    HIPCHK(ctx, DISPATCH(ctx, launch_slant_sum<float>(g, (float *)vd, t, kept, beta, ctx->stream),
                         launch_slant_sum<double>(g, (double *)vd, t, kept, beta, ctx->stream)));
    return FWI_OK;
}

int fwi_vec_regularizer(fwi_ctx *ctx, int32_t kind, int32_t x, int32_t x0, int32_t v, int32_t out, double alpha,
                        double beta, const double *weight, double eps, double *value_out) {
    if (!ctx) return FWI_EINVAL;
    if (kind != FWI_REG_TIKHONOV && kind != FWI_REG_TV)
        return ctx->fail(FWI_EINVAL, "fwi_vec_regularizer: unknown kind %d", (int)kind);
    void *vx = vec_slot(ctx, x), *vx0 = nullptr, *vv = nullptr, *vout = nullptr;
    if (!vx) return ctx->fail(FWI_EINVAL, "fwi_vec_regularizer: x: vector slot %d does not exist", (int)x);
    if (x0 != -1 && !(vx0 = vec_slot(ctx, x0)))
        return ctx->fail(FWI_EINVAL, "fwi_vec_regularizer: x0: vector slot %d does not exist", (int)x0);
    if (v != -1 && !(vv = vec_slot(ctx, v)))
        return ctx->fail(FWI_EINVAL, "fwi_vec_regularizer: v: vector slot %d does not exist", (int)v);
    if (out != -1 && !(vout = vec_slot(ctx, out)))
        return ctx->fail(FWI_EINVAL, "fwi_vec_regularizer: out: vector slot %d does not exist", (int)out);
    if (vout && (vout == vx || vout == vx0 || vout == vv))
        return ctx->fail(FWI_EINVAL, "fwi_vec_regularizer: out (slot %d) must not alias %s", (int)out,
                         vout == vx ? "x" : vout == vx0 ? "x0" : "v");
    if (!vout && !value_out)
        return ctx->fail(FWI_EINVAL, "fwi_vec_regularizer: out == -1 and value_out == NULL: nothing to do");
    if (!weight) return ctx->fail(FWI_EINVAL, "fwi_vec_regularizer: null weight");
    const int nd = ctx->gd.ndim;
    for (int d = 0; d < nd; ++d)
        if (!std::isfinite(weight[d]) || weight[d] < 0.0)
            return ctx->fail(FWI_EINVAL, "fwi_vec_regularizer: weight[%d] = %g must be finite and >= 0", d, weight[d]);
    if (kind == FWI_REG_TV && (!std::isfinite(eps) || eps <= 0.0))
        return ctx->fail(FWI_EINVAL, "fwi_vec_regularizer: eps = %g must be finite and > 0 for total variation", eps);
    if (!std::isfinite(alpha)) return ctx->fail(FWI_EINVAL, "fwi_vec_regularizer: alpha = %g must be finite", alpha);
    if (!std::isfinite(beta)) return ctx->fail(FWI_EINVAL, "fwi_vec_regularizer: beta = %g must be finite", beta);
    const double w[3] = {weight[0], nd == 3 ? weight[1] : 0.0, weight[nd - 1]};  // z, y, x
    if (kind != FWI_REG_TV) eps = 0.0;
    (void)hipSetDevice(ctx->cfg.device);
    return DISPATCH(ctx, vec_regularizer<float>(ctx, kind, vx, vx0, vv, vout, alpha, beta, w, eps, value_out),
                    vec_regularizer<double>(ctx, kind, vx, vx0, vv, vout, alpha, beta, w, eps, value_out));
}

}  // extern "C"
