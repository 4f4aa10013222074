// C-ABI of the engine, the images formed from the resident Fourier coefficients after the sweeps (include/fwi.h:
// fwi_fourier_image, fwi_fourier_{gradient,illumination,offset_image,lag_image,split_image}[_vec], the spectra), and
// the argument checks every call on the Fourier store shares.  Host side only; no time loop runs here.
#include <algorithm>
#include <cmath>
#include <cstdio>

#include "fwi_host.h"
#include "fwi_fimage.h"
#include "fwi_feximage.h"
#include "fwi_fsplit.h"
#include "fwi_illum.h"

namespace fwi {

// The weights a_k w_k of one image / illumination pass on the device (w_k as fourier_table's synthesis weights, for
// the N samples of the last forward); `fw` = nullptr: a_k = 1.  With `tau` (a time-lag image) the table holds 2 F
// entries instead, C_k = a_k w_k cos phi_k at k and D_k = a_k w_k sin phi_k at F + k, phi_k = 2 pi f_k tau formed in
// fp64 from the fractional part of f_k tau as fourier_table forms its phases (tau = 0: C_k = a_k w_k, D_k = 0).
// `unit`: a_k w_k = 1, the bare phases (cos phi_k, sin phi_k) of an extended Born source (fwi_fbornx.h).
// `taps` (a split image, fwi_fsplit.h): the `ntaps` <= FWI_SPLIT_RMAX taps follow at FWI_FOURIER_FMAX.
template <typename T>
int fourier_weights(fwi_ctx *ctx, const double *fw, const double *tau, bool unit, const double *taps, int ntaps) {
    const int S = ctx->istride, N = (ctx->nt + S - 1) / S, F = (int)ctx->four_freqs.size();
    const double sdt = (double)S * ctx->cfg.dt;
    if (int rc = dev_first_use(ctx, &ctx->four_w, 2 * FWI_FOURIER_FMAX * sizeof(double), "four_w")) return rc;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // the upload of the pass before may still read the host copy
    std::vector<double> &a = ctx->four_w_host;
    a.assign(tau ? 2 * F : F, 0.0);
    for (int k = 0; k < F; ++k) {
        const double f = ctx->four_freqs[k];
        const bool edge = f == 0.0 || std::fabs(2.0 * f * sdt - 1.0) <= FOURIER_NYQUIST_RTOL;
        a[k] = unit ? 1.0 : (fw ? fw[k] : 1.0) * ((edge ? 1.0 : 2.0) / N);
        if (tau) {
            const double x = f * *tau, th = 2.0 * M_PI * (x - std::floor(x));
            a[F + k] = a[k] * std::sin(th);
            a[k] = a[k] * std::cos(th);
        }
    }
    if (taps) {
        a.resize(FWI_FOURIER_FMAX, 0.0);
        a.insert(a.end(), taps, taps + ntaps);
    }
    HIPCHK(ctx, hipMemcpyAsync(ctx->four_w, a.data(), a.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    return FWI_OK;
}

template int fourier_weights<float>(fwi_ctx *, const double *, const double *, bool, const double *, int);
template int fourier_weights<double>(fwi_ctx *, const double *, const double *, bool, const double *, int);

// What the entry points of spectral imaging begin with: a Fourier context that holds the Q_k of a forward(save) and, with
// `need_m`, the M_k of an fwi_adjoint_spectral that followed it.
int fourier_callable(fwi_ctx *ctx, const char *who, bool need_m) {
    if (ctx->four_freqs.empty())
        return ctx->fail(FWI_ESTATE, "%s: the Fourier store is off (fwi_set_fourier_store)", who);
    if (!ctx->have_forward || !ctx->have_q || !ctx->four_acc)
        return ctx->fail(FWI_ESTATE, "%s: needs fwi_forward(save=1) on this context first", who);
    if (need_m && (!ctx->have_m || !ctx->four_adj))
        return ctx->fail(FWI_ESTATE, "%s: needs an fwi_adjoint_spectral after the latest fwi_forward(save=1)", who);
    return FWI_OK;
}

// the F weights of the caller (nullptr: ones): finite, and with `nonneg` >= 0
int fourier_weight_args(fwi_ctx *ctx, const char *who, const double *fw, bool nonneg) {
    if (!fw) return FWI_OK;
    for (int k = 0; k < (int)ctx->four_freqs.size(); ++k) {
        if (!std::isfinite(fw[k])) return ctx->fail(FWI_EINVAL, "%s: freq_weights[%d] is not finite", who, k);
        if (nonneg && fw[k] < 0.0) return ctx->fail(FWI_EINVAL, "%s: freq_weights[%d]=%g is negative", who, k, fw[k]);
    }
    return FWI_OK;
}

// The axis of the GridDesc (0 = z, 1 = y, 2 = x) of the caller's `axis` in grid order z, [y,] x, in *ax; refused outside it.
int fourier_axis(fwi_ctx *ctx, const char *who, int32_t axis, int *ax) {
    if (axis < 0 || axis >= ctx->gd.ndim)
        return ctx->fail(FWI_EINVAL, "%s: axis=%d outside [0, %d)", who, (int)axis, ctx->gd.ndim);
    *ax = axis == ctx->gd.ndim - 1 ? 2 : ctx->gd.ndim == 3 ? axis : 0;
    return FWI_OK;
}

// A time lag `tau` (l < 0), or taus[l]: that it is finite, or with `phase` that it leaves a finite phase at every
// frequency of the store.  Two calls, because the entry points check other arguments in between.
int fourier_tau_ok(fwi_ctx *ctx, const char *who, double tau, int l, bool phase) {
    char name[32] = "tau";
    if (l >= 0) snprintf(name, sizeof name, "taus[%d]", l);
    if (!phase) return std::isfinite(tau) ? FWI_OK : ctx->fail(FWI_EINVAL, "%s: %s is not finite", who, name);
    for (double f : ctx->four_freqs)
        if (!std::isfinite(f * tau))
            return ctx->fail(FWI_EINVAL, "%s: %s=%g s leaves no finite phase at %g Hz", who, name, tau, f);
    return FWI_OK;
}

}  // namespace fwi

namespace {

template <typename T>
struct Impl {
    // dst = beta dst + sum_k a_k w_k Re(Q_k conj M_k) (`illum`: |Q_k|^2) in the units of g_acc
    static int fourier_sum(fwi_ctx *ctx, const double *fw, bool illum, void *dst, int beta) {
        int rc = fourier_weights<T>(ctx, fw);
        if (rc) return rc;
        const int F = (int)ctx->four_freqs.size();
        if (illum)
            HIPCHK(ctx, launch_fimage_illuminate<T>((T *)dst, (const T *)ctx->four_acc, (const double *)ctx->four_w,
                                                    ctx->gd.npts, F, beta, ctx->stream));
        else
            HIPCHK(ctx, launch_fimage_image<T>((T *)dst, (const T *)ctx->four_acc, (const T *)ctx->four_adj,
                                               (const double *)ctx->four_w, ctx->gd.npts, F, beta, ctx->stream));
        return FWI_OK;
    }

    static int fourier_image(fwi_ctx *ctx, const double *fw) {
        int rc = fourier_sum(ctx, fw, false, ctx->g_acc, 1);
        if (rc) return rc;
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        return FWI_OK;
    }

    // The tail of every image on the Fourier store: the sum over k that stands in the compact device array `dev` is scaled
    // there into the gradient (`illum`: the illumination) in the parametrisation `wrt`; `dev` is ctx->g_out and goes on to
    // the host array `out`, or a vector slot (out = nullptr).
    static int fourier_tail(fwi_ctx *ctx, int32_t wrt, bool illum, void *dev, T *out) {
        const double dt2 = ctx->cfg.dt * ctx->cfg.dt, S = (double)ctx->istride;
        if (illum)
            HIPCHK(ctx, launch_illum_finalize<T>(ctx->gd, (const T *)dev, (const T *)ctx->c_dev, (T *)dev, S / (dt2 * dt2),
                                                 wrt == FWI_WRT_VELOCITY, ctx->stream));
        else
            HIPCHK(ctx, launch_finalize_gradient<T>(ctx->gd, (const T *)dev, (const T *)ctx->c_dev, (T *)dev, -S / dt2,
                                                    wrt == FWI_WRT_VELOCITY, ctx->stream));
        if (out)
            if (int rc = download_compact<T>(ctx, out, dev)) return rc;
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        return FWI_OK;
    }

    // the gradient (`illum`: the illumination) of that sum alone into `dev`
    static int fourier_finalize(fwi_ctx *ctx, int32_t wrt, const double *fw, bool illum, void *dev, T *out) {
        int rc = fourier_sum(ctx, fw, illum, dev, 0);
        return rc ? rc : fourier_tail(ctx, wrt, illum, dev, out);
    }

    // One lag of an extended image (fwi_feximage.h) into `dev`, through the sum and fourier_tail(wrt = FWI_WRT_SLOWNESS2): the offset image of `h` cells along `axis` (0 = z, 1 = y, 2 = x of the
    // GridDesc), or with `tau` the time-lag image.  Q_k, M_k and the gradient accumulator are read at most.
    static int fourier_extended(fwi_ctx *ctx, int axis, int64_t h, const double *tau, const double *fw, void *dev, T *out) {
        int rc = fourier_weights<T>(ctx, fw, tau);
        if (rc) return rc;
        const int F = (int)ctx->four_freqs.size();
        const T *q = (const T *)ctx->four_acc, *m = (const T *)ctx->four_adj;
        if (tau)
            HIPCHK(ctx, launch_feximage_lag<T>((T *)dev, q, m, (const double *)ctx->four_w, ctx->gd.npts, F, ctx->stream));
        else
            HIPCHK(ctx, launch_feximage_offset<T>(ctx->gd, (T *)dev, q, m, (const double *)ctx->four_w, F, axis, h,
                                                  ctx->stream));
        return fourier_tail(ctx, FWI_WRT_SLOWNESS2, false, dev, out);
    }

    // One part of the split image (fwi_fsplit.h) into `dev`, through the sum and fourier_tail: `axis` 0 = z, 1 = y, 2 = x of the GridDesc, `taps` the `ntaps` < n_axis taps that can touch a cell.
    // Q_k, M_k and the gradient accumulator are read at most.
    static int fourier_split(fwi_ctx *ctx, int32_t wrt, int axis, const double *taps, int ntaps, double alpha, double beta,
                             const double *fw, void *dev, T *out) {
        static_assert(FSPLIT_RMAX == FWI_SPLIT_RMAX && FWI_SPLIT_RMAX <= FWI_FOURIER_FMAX, "the taps share four_w");
        int rc = fourier_weights<T>(ctx, fw, nullptr, false, taps, ntaps);
        if (rc) return rc;
        const int F = (int)ctx->four_freqs.size();
        const double *w = (const double *)ctx->four_w;
        HIPCHK(ctx, launch_fsplit<T>(ctx->gd, (T *)dev, (const T *)ctx->four_acc, (const T *)ctx->four_adj, w, F, axis,
                                     w + FWI_FOURIER_FMAX, ntaps, alpha, beta, ctx->stream));
        return fourier_tail(ctx, wrt, false, dev, out);
    }
};

}  // namespace

extern "C" {

int fwi_fourier_spectrum(fwi_ctx *ctx, int32_t k, void *re_out, void *im_out) {
    if (!ctx) return FWI_EINVAL;
    if (ctx->four_freqs.empty())
        return ctx->fail(FWI_ESTATE, "fwi_fourier_spectrum: the Fourier store is off (fwi_set_fourier_store)");
    if (k < 0 || k >= (int)ctx->four_freqs.size())
        return ctx->fail(FWI_EINVAL, "fwi_fourier_spectrum: frequency index %d outside [0, %d)", (int)k,
                         (int)ctx->four_freqs.size());
    if (!re_out || !im_out) return ctx->fail(FWI_EINVAL, "fwi_fourier_spectrum: null output");
    if (!ctx->have_q || !ctx->four_acc)
        return ctx->fail(FWI_ESTATE, "fwi_fourier_spectrum: needs fwi_forward(save=1) on this context first");
    (void)hipSetDevice(ctx->cfg.device);
    const char *re = (const char *)ctx->four_acc + (size_t)2 * k * ctx->gd.npts * ctx->esize;
    const char *im = re + (size_t)ctx->gd.npts * ctx->esize;
    for (int c = 0; c < 2; ++c) {  // (one staging array: the first copy leaves it before the second repack)
        if (int rc = DISPATCH(ctx, download_compact<float>(ctx, c ? im_out : re_out, c ? im : re),
                              download_compact<double>(ctx, c ? im_out : re_out, c ? im : re)))
            return rc;
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    return FWI_OK;
}

static int wrt_and_model(fwi_ctx *ctx, const char *who, int32_t wrt) {
    if (wrt != FWI_WRT_VELOCITY && wrt != FWI_WRT_SLOWNESS2)
        return ctx->fail(FWI_EINVAL, "%s: unknown parametrisation %d", who, (int)wrt);
    if (!ctx->have_model) return ctx->fail(FWI_ESTATE, "%s: no model set", who);
    return FWI_OK;
}

int fwi_fourier_image(fwi_ctx *ctx, const double *freq_weights) {
    if (!ctx) return FWI_EINVAL;
    if (int rc = fourier_callable(ctx, "fwi_fourier_image", true)) return rc;
    if (int rc = fourier_weight_args(ctx, "fwi_fourier_image", freq_weights, false)) return rc;
    (void)hipSetDevice(ctx->cfg.device);
    return DISPATCH_CALL(ctx, fourier_image, freq_weights);
}

// `illum`: fwi_fourier_illumination[_vec], else fwi_fourier_gradient[_vec]; `out`: the host array, nullptr for `dev`
static int fourier_finalize(fwi_ctx *ctx, const char *who, bool illum, int32_t wrt, const double *fw, void *dev,
                            void *out) {
    if (int rc = fourier_callable(ctx, who, !illum)) return rc;
    if (int rc = fourier_weight_args(ctx, who, fw, illum)) return rc;
    if (int rc = wrt_and_model(ctx, who, wrt)) return rc;
    (void)hipSetDevice(ctx->cfg.device);
    return DISPATCH(ctx, Impl<float>::fourier_finalize(ctx, wrt, fw, illum, dev, (float *)out),
                    Impl<double>::fourier_finalize(ctx, wrt, fw, illum, dev, (double *)out));
}

int fwi_fourier_gradient(fwi_ctx *ctx, int32_t wrt, const double *freq_weights, void *out) {
    if (!ctx) return FWI_EINVAL;
    if (!out) return ctx->fail(FWI_EINVAL, "fwi_fourier_gradient: null output");
    return fourier_finalize(ctx, "fwi_fourier_gradient", false, wrt, freq_weights, ctx->g_out, out);
}

int fwi_fourier_gradient_vec(fwi_ctx *ctx, int32_t wrt, const double *freq_weights, int32_t slot) {
    if (!ctx) return FWI_EINVAL;
    VEC_OR_FAIL(ctx, v, slot);
    return fourier_finalize(ctx, "fwi_fourier_gradient_vec", false, wrt, freq_weights, v, nullptr);
}

int fwi_fourier_illumination(fwi_ctx *ctx, int32_t wrt, const double *freq_weights, void *out) {
    if (!ctx) return FWI_EINVAL;
    if (!out) return ctx->fail(FWI_EINVAL, "fwi_fourier_illumination: null output");
    return fourier_finalize(ctx, "fwi_fourier_illumination", true, wrt, freq_weights, ctx->g_out, out);
}

int fwi_fourier_illumination_vec(fwi_ctx *ctx, int32_t wrt, const double *freq_weights, int32_t slot) {
    if (!ctx) return FWI_EINVAL;
    VEC_OR_FAIL(ctx, v, slot);
    return fourier_finalize(ctx, "fwi_fourier_illumination_vec", true, wrt, freq_weights, v, nullptr);
}

// `tau`: fwi_fourier_lag_image[_vec], else fwi_fourier_offset_image[_vec] of `h` cells along `axis` of the grid order;
// `out`: the host array, nullptr for `dev`
static int fourier_extended(fwi_ctx *ctx, const char *who, int32_t axis, int32_t h, const double *tau, const double *fw,
                            void *dev, void *out) {
    if (int rc = fourier_callable(ctx, who, true)) return rc;
    int ax = 0;
    if (int rc = tau ? fourier_tau_ok(ctx, who, *tau, -1, false) : fourier_axis(ctx, who, axis, &ax)) return rc;
    if (int rc = fourier_weight_args(ctx, who, fw, false)) return rc;
    if (tau)
        if (int rc = fourier_tau_ok(ctx, who, *tau, -1, true)) return rc;
    (void)hipSetDevice(ctx->cfg.device);
    return DISPATCH(ctx, Impl<float>::fourier_extended(ctx, ax, h, tau, fw, dev, (float *)out),
                    Impl<double>::fourier_extended(ctx, ax, h, tau, fw, dev, (double *)out));
}

int fwi_fourier_offset_image(fwi_ctx *ctx, int32_t axis, int32_t h, const double *freq_weights, void *out) {
    if (!ctx) return FWI_EINVAL;
    if (!out) return ctx->fail(FWI_EINVAL, "fwi_fourier_offset_image: null output");
    return fourier_extended(ctx, "fwi_fourier_offset_image", axis, h, nullptr, freq_weights, ctx->g_out, out);
}

int fwi_fourier_offset_image_vec(fwi_ctx *ctx, int32_t axis, int32_t h, const double *freq_weights, int32_t slot) {
    if (!ctx) return FWI_EINVAL;
    VEC_OR_FAIL(ctx, v, slot);
    return fourier_extended(ctx, "fwi_fourier_offset_image_vec", axis, h, nullptr, freq_weights, v, nullptr);
}

int fwi_fourier_lag_image(fwi_ctx *ctx, double tau, const double *freq_weights, void *out) {
    if (!ctx) return FWI_EINVAL;
    if (!out) return ctx->fail(FWI_EINVAL, "fwi_fourier_lag_image: null output");
    return fourier_extended(ctx, "fwi_fourier_lag_image", 0, 0, &tau, freq_weights, ctx->g_out, out);
}

int fwi_fourier_lag_image_vec(fwi_ctx *ctx, double tau, const double *freq_weights, int32_t slot) {
    if (!ctx) return FWI_EINVAL;
    VEC_OR_FAIL(ctx, v, slot);
    return fourier_extended(ctx, "fwi_fourier_lag_image_vec", 0, 0, &tau, freq_weights, v, nullptr);
}

// fwi_fourier_split_image[_vec]; `out`: the host array, nullptr for `dev`
static int fourier_split(fwi_ctx *ctx, const char *who, int32_t wrt, int32_t part, int32_t axis, int32_t ntaps,
                         const double *taps, const double *fw, void *dev, void *out) {
    if (int rc = fourier_callable(ctx, who, true)) return rc;
    if (part != FWI_SPLIT_SAME && part != FWI_SPLIT_OPPOSITE && part != FWI_SPLIT_HILBERT)
        return ctx->fail(FWI_EINVAL, "%s: unknown part %d", who, (int)part);
    int ax = 0;
    if (int rc = fourier_axis(ctx, who, axis, &ax)) return rc;
    if (ntaps < 1 || ntaps > FWI_SPLIT_RMAX)
        return ctx->fail(FWI_EINVAL, "%s: ntaps=%d outside [1, %d]", who, (int)ntaps, FWI_SPLIT_RMAX);
    if (!taps) return ctx->fail(FWI_EINVAL, "%s: null taps", who);
    for (int r = 0; r < ntaps; ++r)
        if (!std::isfinite(taps[r])) return ctx->fail(FWI_EINVAL, "%s: taps[%d] is not finite", who, r);
    if (int rc = fourier_weight_args(ctx, who, fw, false)) return rc;
    if (int rc = wrt_and_model(ctx, who, wrt)) return rc;
    (void)hipSetDevice(ctx->cfg.device);
    const int n = ax == 0 ? ctx->gd.nz : ax == 1 ? ctx->gd.ny : ctx->gd.nx;
    int R = std::min<int>(ntaps, n - 1);  // a tap at r >= n touches no cell, a trailing zero tap is skipped
    while (R > 0 && taps[R - 1] == 0.0) --R;
    const double alpha = part == FWI_SPLIT_HILBERT ? 0.0 : 0.5;
    const double beta = part == FWI_SPLIT_HILBERT ? 1.0 : part == FWI_SPLIT_SAME ? 0.5 : -0.5;
    return DISPATCH(ctx, Impl<float>::fourier_split(ctx, wrt, ax, taps, R, alpha, beta, fw, dev, (float *)out),
                    Impl<double>::fourier_split(ctx, wrt, ax, taps, R, alpha, beta, fw, dev, (double *)out));
}

int fwi_fourier_split_image(fwi_ctx *ctx, int32_t wrt, int32_t part, int32_t axis, int32_t ntaps, const double *taps,
                            const double *freq_weights, void *out) {
    if (!ctx) return FWI_EINVAL;
    if (!out) return ctx->fail(FWI_EINVAL, "fwi_fourier_split_image: null output");
    return fourier_split(ctx, "fwi_fourier_split_image", wrt, part, axis, ntaps, taps, freq_weights, ctx->g_out, out);
}

int fwi_fourier_split_image_vec(fwi_ctx *ctx, int32_t wrt, int32_t part, int32_t axis, int32_t ntaps, const double *taps,
                                const double *freq_weights, int32_t slot) {
    if (!ctx) return FWI_EINVAL;
    VEC_OR_FAIL(ctx, v, slot);
    return fourier_split(ctx, "fwi_fourier_split_image_vec", wrt, part, axis, ntaps, taps, freq_weights, v, nullptr);
}

int fwi_fourier_adjoint_spectrum(fwi_ctx *ctx, int32_t k, void *re_out, void *im_out) {
    if (!ctx) return FWI_EINVAL;
    if (int rc = fourier_callable(ctx, "fwi_fourier_adjoint_spectrum", true)) return rc;
    if (k < 0 || k >= (int)ctx->four_freqs.size())
        return ctx->fail(FWI_EINVAL, "fwi_fourier_adjoint_spectrum: frequency index %d outside [0, %d)", (int)k,
                         (int)ctx->four_freqs.size());
    if (!re_out || !im_out) return ctx->fail(FWI_EINVAL, "fwi_fourier_adjoint_spectrum: null output");
    (void)hipSetDevice(ctx->cfg.device);
    const char *re = (const char *)ctx->four_adj + (size_t)2 * k * ctx->gd.npts * ctx->esize;
    const char *im = re + (size_t)ctx->gd.npts * ctx->esize;
    for (int c = 0; c < 2; ++c) {  // (one staging array: the first copy leaves it before the second repack)
        if (int rc = DISPATCH(ctx, download_compact<float>(ctx, c ? im_out : re_out, c ? im : re),
                              download_compact<double>(ctx, c ? im_out : re_out, c ? im : re)))
            return rc;
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    return FWI_OK;
}

}  // extern "C"
