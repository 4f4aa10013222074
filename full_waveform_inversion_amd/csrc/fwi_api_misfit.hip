// C-ABI of the engine, the data misfits (include/fwi.h: fwi_misfit_*, fwi_match_solve, fwi_residual_*): the
// synthetics of the last forward against the data, the adjoint source left on the device.  Host side, no time loop.
#include <algorithm>
#include <cmath>
#include <vector>

#include "fwi_host.h"
#include "fwi_data.h"
#include "fwi_gather_tile.h"
#include "fwi_match.h"
#include "fwi_match_solve.h"
#include "fwi_envelope.h"
#include "fwi_corr.h"
#include "fwi_ttime.h"
#include "fwi_ot.h"
#include "fwi_spec.h"
#include "fwi_awi.h"
#include "fwi_robust.h"

namespace {

template <typename T>
struct Impl {
    // weights (nt, ntr) and taps b_0 .. b_R of the caller -> the device; the buffers of the two filter passes.  R_out:
    // the half-width that meets samples (taps beyond nt - 1 are not uploaded)
    static int data_prepare(fwi_ctx *ctx, const T *weights, const double *taps, int R, int nt, int ntr, const T **w_dev,
                            const double **taps_dev, int *R_out) {
        const size_t n = (size_t)nt * ntr;
        int rc;
        if ((rc = ensure(ctx, ctx->data_tmp, n * sizeof(T)))) return rc;
        if ((rc = ensure(ctx, ctx->data_part, (size_t)(gather_blocks(nt, ntr) + 1) * sizeof(double))))
            return rc;
        *w_dev = nullptr;
        if (weights) {
            if ((rc = ensure(ctx, ctx->data_w, n * sizeof(T)))) return rc;
            if ((rc = upload_series(ctx, ctx->data_w.p, weights, n * sizeof(T)))) return rc;
            *w_dev = (const T *)ctx->data_w.p;
        }
        *taps_dev = nullptr;
        *R_out = 0;
        if (taps) {
            *R_out = std::min(R, nt - 1);
            const size_t bytes = (size_t)(*R_out + 1) * sizeof(double);
            if ((rc = ensure(ctx, ctx->data_taps, bytes))) return rc;
            // the taps are the caller's pageable memory: the copy is complete before anything that can fail and return
            // follows it (at most 32 KB, in the stream's order behind the uploads above)
            HIPCHK(ctx, hipMemcpyAsync(ctx->data_taps.p, taps, bytes, hipMemcpyHostToDevice, ctx->stream));
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
            *taps_dev = (const double *)ctx->data_taps.p;
        }
        return FWI_OK;
    }

    // What the data misfits share around their own launches: where the gathers lie, the upload of d_obs, the filter B
    // before and after, the scatter onto the nodes, the read-back of the sum of squares and the state of the device
    // residual.  Off-grid receivers: everything per POINT (against the gathered synthetics kept by the forward); the
    // residual is then scattered onto the nodes, where the adjoint sweep injects it.
    struct Misfit {
        fwi_ctx *ctx;
        int nt = 0, ntr = 0;
        size_t n = 0;
        bool data = false;          // there are receivers and samples: otherwise nothing is launched
        T *resid = nullptr;         // d_obs after begin(), the residual after finish(): ctx->amp, or ctx->pts_a per point
        const T *syn = nullptr;     // the synthetics of the last forward: ctx->series, or ctx->pts_d per point
        const T *w = nullptr;       // data_prepare's: the weights, the taps of B, the half-width that meets samples
        const double *b = nullptr;
        int Re = 0;
        double *part = nullptr;     // gather_blocks + 1 doubles: the block sums of a gather kernel and their total,
        const double *sum = nullptr;  // ... which is what finish() reads back

        explicit Misfit(fwi_ctx *c) : ctx(c) {}

        // Whatever residual the device held goes with the upload of d_obs: none is left until finish() has succeeded.
        int begin(const T *d_obs) {
            const fwi_ctx::SpreadSet &sp = ctx->rec_sp;
            nt = ctx->nt, ntr = sp.npts ? sp.npts : ctx->nrec;
            n = (size_t)nt * ntr;
            data = n && ctx->nrec;
            ctx->have_dev_residual = false;
            ctx->resid_pts_in = fwi_ctx::RESID_PTS_NONE;
            if (!data) return FWI_OK;
            resid = (T *)ctx->amp.p, syn = (const T *)ctx->series.p;
            if (sp.npts) {
                if (int rc = ensure(ctx, ctx->pts_a, n * sizeof(T))) return rc;
                resid = (T *)ctx->pts_a.p, syn = (const T *)ctx->pts_d.p;
            }
            return upload_series(ctx, resid, d_obs, n * sizeof(T));
        }

        // ... and the weights, the taps and the buffers of the filter passes
        int begin(const T *d_obs, const T *weights, const double *taps, int R) {
            int rc = begin(d_obs);
            if (rc || !data || (rc = data_prepare(ctx, weights, taps, R, nt, ntr, &w, &b, &Re))) return rc;
            part = (double *)ctx->data_part.p;
            sum = part + gather_blocks(nt, ntr);
            return FWI_OK;
        }

        int filter(T *out, const T *in) {
            HIPCHK(ctx, launch_fir_time<T>(out, in, nullptr, nullptr, nullptr, b, Re, nt, ntr, nullptr, false, ctx->stream));
            return FWI_OK;
        }

        // s1, d1: the synthetics and the data; with taps s' = B d_syn and d' = B d_obs, each rounded to T once
        int prefilter(const T **s1, const T **d1) {
            *s1 = syn, *d1 = resid;
            if (!b) return FWI_OK;
            int rc;
            if ((rc = ensure(ctx, ctx->data_s, n * sizeof(T))) ||
                (rc = ensure(ctx, ctx->data_d, n * sizeof(T))) ||
                (rc = filter((T *)ctx->data_s.p, syn)) || (rc = filter((T *)ctx->data_d.p, resid)))
                return rc;
            *s1 = (const T *)ctx->data_s.p, *d1 = (const T *)ctx->data_d.p;
            return FWI_OK;
        }

        // where a misfit that prefilters writes its adjoint source once s' and d' are used up: without taps it is the
        // residual; with taps it takes the place of s', and finish() has B write r over the uploaded d_obs
        T *adjoint_source() const { return b ? (T *)ctx->data_s.p : resid; }

        // *tw := the caller's ntr weights per trace on the device (ctx->data_tw), or nullptr where there are none (all 1)
        int trace_weights(const double *host, const double **tw) {
            *tw = nullptr;
            if (!host) return FWI_OK;
            const size_t bytes = (size_t)ntr * sizeof(double);
            if (int rc = ensure(ctx, ctx->data_tw, bytes)) return rc;
            // (the caller's pageable memory: the copy is complete before anything that can fail and return follows it)
            HIPCHK(ctx, hipMemcpyAsync(ctx->data_tw.p, host, bytes, hipMemcpyHostToDevice, ctx->stream));
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
            *tw = (const double *)ctx->data_tw.p;
            return FWI_OK;
        }

        // resid := B src (src == resid: it is there already), onto the nodes, *ss := the sum of squares
        int finish(const T *src, double *ss) {
            const fwi_ctx::SpreadSet &sp = ctx->rec_sp;
            if (data) {
                if (src != resid)
                    if (int rc = filter(resid, src)) return rc;
                if (sp.npts)
                    HIPCHK(ctx, launch_scatter_series<T>((const T *)resid, (T *)ctx->amp.p, (const int *)sp.owner,
                                                         (const T *)sp.weight, nt, sp.npts, ctx->nrec, ctx->stream));
                HIPCHK(ctx, hipMemcpyAsync(ss, sum, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
                HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
            }
            ctx->have_dev_residual = true;
            ctx->resid_pts_in = (data && sp.npts) ? fwi_ctx::RESID_PTS_A : fwi_ctx::RESID_PTS_NONE;
            return FWI_OK;
        }

        // after finish(): up to two arrays of ntr numbers per trace to the caller (a null destination: not asked for),
        // under one synchronise; without receivers or samples no trace counts and they are zeros
        template <typename A, typename B = double>
        int per_trace(A *out_a, const A *dev_a, B *out_b = nullptr, const B *dev_b = nullptr) {
            if (!data) {
                if (out_a) std::fill(out_a, out_a + ntr, A(0));
                if (out_b) std::fill(out_b, out_b + ntr, B(0));
                return FWI_OK;
            }
            if (out_a) HIPCHK(ctx, hipMemcpyAsync(out_a, dev_a, (size_t)ntr * sizeof(A), hipMemcpyDeviceToHost, ctx->stream));
            if (out_b) HIPCHK(ctx, hipMemcpyAsync(out_b, dev_b, (size_t)ntr * sizeof(B), hipMemcpyDeviceToHost, ctx->stream));
            if (out_a || out_b) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
            return FWI_OK;
        }
    };

    // d_obs -> the residual buffer, then residual := d_syn - d_obs and J = 1/2 sum residual^2, all on the device
    static int misfit_l2(fwi_ctx *ctx, const T *d_obs, double *J_out) {
        Misfit m(ctx);
        double ss = 0.0;
        int rc = m.begin(d_obs);
        if (rc) return rc;
        if (m.data) {
            if ((rc = sum_partials(ctx, &m.part))) return rc;
            m.sum = m.part + sum_blocks((int64_t)m.n);
            HIPCHK(ctx, launch_residual_l2<T>(m.syn, m.resid, (int64_t)m.n, m.part, ctx->stream));
        }
        if ((rc = m.finish(m.resid, &ss))) return rc;
        *J_out = 0.5 * ss;
        return FWI_OK;
    }

    // e = M . B (d_syn - d_obs), J = 1/2 sum e^2, r = B (M . e) where the adjoint sweep reads its amplitudes
    static int misfit_weighted(fwi_ctx *ctx, const T *d_obs, const T *weights, const double *taps, int R, double *J_out) {
        Misfit m(ctx);
        double ss = 0.0;
        int rc = m.begin(d_obs, weights, taps, R);
        if (rc) return rc;
        if (m.data) {
            // neither taps nor weights: e is the plain residual and the call is fwi_misfit_l2 with a fixed-order sum, so
            // J is summed as there, from the residual as stored; otherwise from the unrounded e
            const bool plain = !m.w && !m.b;
            T *e = (T *)ctx->data_tmp.p;
            HIPCHK(ctx, launch_fir_time<T>(e, m.syn, m.resid, nullptr, m.w, m.b, m.Re, m.nt, m.ntr, m.part, plain,
                                           ctx->stream));
            HIPCHK(ctx, launch_fir_time<T>(m.resid, e, nullptr, m.w, nullptr, m.b, m.Re, m.nt, m.ntr, nullptr, false,
                                           ctx->stream));
        }
        if ((rc = m.finish(m.resid, &ss))) return rc;
        *J_out = 0.5 * ss;
        return FWI_OK;
    }

    // s' = B d_syn, d' = B d_obs, e = M . (C_f s' - d'), J = 1/2 sum e^2 + mu/2 |f|^2, r = B C_f^T (M . e) where the
    // adjoint sweep reads its amplitudes; f given, or the minimiser (G + mu I)^-1 b of J
    static int misfit_matched(fwi_ctx *ctx, const T *d_obs, const T *weights, const double *taps, int R, int L, double mu,
                              const double *f_in, double *f_out, double *normal_out, double *J_out) {
        const int K = 2 * L + 1;
        std::vector<double> f(K, 0.0), nrm((size_t)K * K + K, 0.0);
        if (f_in) std::copy(f_in, f_in + K, f.begin());
        Misfit m(ctx);
        const T *s1 = nullptr, *d1 = nullptr;
        int rc = m.begin(d_obs, weights, taps, R);
        if (rc) return rc;
        if (m.data) {
            if ((rc = ensure(ctx, ctx->match_f, (size_t)K * sizeof(double)))) return rc;
            if ((rc = m.prefilter(&s1, &d1))) return rc;
            if (!f_in || normal_out) {
                if ((rc = ensure(ctx, ctx->match_part,
                                 (size_t)match_normal_partials(m.nt, m.ntr, L) * sizeof(double))))
                    return rc;
                if ((rc = ensure(ctx, ctx->match_norm, nrm.size() * sizeof(double)))) return rc;
                HIPCHK(ctx, launch_match_normal<T>((double *)ctx->match_norm.p, (double *)ctx->match_part.p, s1, d1, m.w, L,
                                                   m.nt, m.ntr, ctx->stream));
                HIPCHK(ctx, hipMemcpyAsync(nrm.data(), ctx->match_norm.p, nrm.size() * sizeof(double),
                                           hipMemcpyDeviceToHost, ctx->stream));
                HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
            }
        }
        if (!f_in && match_solve(nrm.data(), nrm.data() + (size_t)K * K, K, mu, f.data()))
            return ctx->fail(FWI_EINVAL, "fwi_misfit_matched: the normal matrix G + mu I (L=%d, mu=%g) is not positive "
                                         "definite: raise mu", L, mu);
        double ss = 0.0;
        T *ct = nullptr;
        if (m.data) {
            // (the filter is this call's pageable memory: the copy is complete before anything that can return follows)
            HIPCHK(ctx, hipMemcpyAsync(ctx->match_f.p, f.data(), (size_t)K * sizeof(double), hipMemcpyHostToDevice,
                                       ctx->stream));
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
            const double *fd = (const double *)ctx->match_f.p;
            T *e = (T *)ctx->data_tmp.p;
            HIPCHK(ctx, launch_match_apply<T>(e, s1, d1, nullptr, m.w, fd, L, false, m.nt, m.ntr, m.part, ctx->stream));
            ct = m.adjoint_source();  // C_f^T (M . e)
            HIPCHK(ctx, launch_match_apply<T>(ct, e, nullptr, m.w, nullptr, fd, L, true, m.nt, m.ntr, nullptr, ctx->stream));
        }
        if ((rc = m.finish(ct, &ss))) return rc;
        double ff = 0.0;
        for (int k = 0; k < K; ++k) ff += f[k] * f[k];
        *J_out = 0.5 * ss + 0.5 * mu * ff;
        if (f_out) std::copy(f.begin(), f.end(), f_out);
        if (normal_out) std::copy(nrm.begin(), nrm.end(), normal_out);
        return FWI_OK;
    }

    // s' = B d_syn, d' = B d_obs, e = M . (E(s')^p - E(d')^p), J = 1/2 sum e^2, r = B (g1 - H g2) where the adjoint sweep
    // reads its amplitudes (fwi_envelope.h)
    static int misfit_envelope(fwi_ctx *ctx, const T *d_obs, const T *weights, const double *taps, int R,
                               const double *hilbert, int Q, int power, double eps, double *J_out) {
        Misfit m(ctx);
        double ss = 0.0;
        T *q = nullptr;
        int rc = m.begin(d_obs, weights, taps, R);
        if (rc) return rc;
        if (m.data) {
            if ((rc = ensure(ctx, ctx->env_g2, m.n * sizeof(T)))) return rc;
            // the taps that meet samples; are the even ones all zero (a Hilbert transformer's are)?
            const int Qe = std::max(std::min(Q, m.nt - 1), 1);
            bool odd_only = true;
            for (int k = 2; k <= Qe; k += 2) odd_only = odd_only && hilbert[k - 1] == 0.0;
            if ((rc = ensure(ctx, ctx->env_h, (size_t)Qe * sizeof(double)))) return rc;
            // (the caller's pageable memory: the copy is complete before anything that can fail and return follows it)
            HIPCHK(ctx, hipMemcpyAsync(ctx->env_h.p, hilbert, (size_t)Qe * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
            const double *hd = (const double *)ctx->env_h.p;
            const T *s1, *d1;
            if ((rc = m.prefilter(&s1, &d1))) return rc;
            T *g1 = (T *)ctx->data_tmp.p, *g2 = (T *)ctx->env_g2.p;
            HIPCHK(ctx, launch_env_forward<T>(g1, g2, s1, d1, m.w, hd, Qe, odd_only, power, eps, m.nt, m.ntr, m.part,
                                              ctx->stream));
            q = m.adjoint_source();  // g1 - H g2
            HIPCHK(ctx, launch_env_adjoint<T>(q, g1, g2, hd, Qe, odd_only, m.nt, m.ntr, ctx->stream));
        }
        if ((rc = m.finish(q, &ss))) return rc;
        *J_out = 0.5 * ss;
        return FWI_OK;
    }

    // s' = B d_syn, d' = B d_obs, rho_j the normalised zero-lag correlation of the weighted traces M s', M d' with the
    // floor eps, J = sum_j w_j (1 - rho_j), r = B g where the adjoint sweep reads its amplitudes (fwi_corr.h)
    static int misfit_correlation(fwi_ctx *ctx, const T *d_obs, const T *weights, const double *taps, int R,
                                  const double *trace_weights, double eps, double *J_out, double *rho_out) {
        Misfit m(ctx);
        double J = 0.0;
        T *g = nullptr;
        int rc = m.begin(d_obs, weights, taps, R);
        if (rc) return rc;
        if (m.data) {
            const size_t np = corr_partials(m.nt, m.ntr);
            if ((rc = ensure(ctx, ctx->corr_part, np * sizeof(double))) ||
                (rc = ensure(ctx, ctx->corr_coef, (size_t)3 * m.ntr * sizeof(double))))
                return rc;
            const double *tw;
            if ((rc = m.trace_weights(trace_weights, &tw))) return rc;
            double *part = (double *)ctx->corr_part.p, *coef = (double *)ctx->corr_coef.p;
            m.sum = part + (np - 1);  // the total of the terms w_j (1 - rho_j): J itself
            const T *s1, *d1;
            if ((rc = m.prefilter(&s1, &d1))) return rc;
            HIPCHK(ctx, launch_corr_sums<T>(part, s1, d1, m.w, m.nt, m.ntr, ctx->stream));
            HIPCHK(ctx, launch_corr_coeffs(coef, part, tw, eps, m.nt, m.ntr, ctx->stream));
            g = m.adjoint_source();  // in place of s' (with taps) or of d_obs (without): elementwise
            HIPCHK(ctx, launch_corr_source<T>(g, s1, d1, m.w, coef, m.nt, m.ntr, ctx->stream));
        }
        if ((rc = m.finish(g, &J))) return rc;
        // without receivers or samples rho_out stays as the caller handed it in, as it always has (the two misfits below
        // zero their per-trace outputs then): hence only with data
        if (m.data && (rc = m.per_trace(rho_out, (const double *)ctx->corr_coef.p + 2 * (size_t)m.ntr))) return rc;
        *J_out = J;
        return FWI_OK;
    }

    // s' = B d_syn, d' = B d_obs, c_j(k) the correlation of the weighted traces M s', M d' over the lags |k| <= Ke, tau_j
    // the delay at its refined maximum, J = 1/2 sum_j w_j tau_j^2, r = B g where the adjoint sweep reads its amplitudes
    // (fwi_ttime.h)
    static int misfit_traveltime(fwi_ctx *ctx, const T *d_obs, const T *weights, const double *taps, int R,
                                 const double *trace_weights, int K, double *J_out, double *tau_out, int32_t *lag_out) {
        Misfit m(ctx);
        double J = 0.0;
        T *g = nullptr;
        int rc = m.begin(d_obs, weights, taps, R);
        if (rc) return rc;
        if (m.data) {
            const size_t np = tt_partials(m.nt, m.ntr, K);
            if ((rc = ensure(ctx, ctx->tt_part, np * sizeof(double))) ||
                (rc = ensure(ctx, ctx->tt_coef, (size_t)4 * m.ntr * sizeof(double))) ||
                (rc = ensure(ctx, ctx->tt_lag, (size_t)m.ntr * sizeof(int32_t))))
                return rc;
            const double *tw;
            if ((rc = m.trace_weights(trace_weights, &tw))) return rc;
            double *part = (double *)ctx->tt_part.p, *coef = (double *)ctx->tt_coef.p;
            int32_t *lag = (int32_t *)ctx->tt_lag.p;
            m.sum = part + (np - 1);  // the total of the terms 1/2 w_j tau_j^2: J itself
            const T *s1, *d1;
            if ((rc = m.prefilter(&s1, &d1))) return rc;
            HIPCHK(ctx, launch_tt_xcorr<T>(part, s1, d1, m.w, K, m.nt, m.ntr, ctx->stream));
            HIPCHK(ctx, launch_tt_pick(coef, lag, part, tw, ctx->cfg.dt, K, m.nt, m.ntr, ctx->stream));
            // g reads d' at shifted rows, and without taps adjoint_source() IS d': g goes to the spare gather buffer, and
            // finish() filters (with taps) or copies (without) it into place
            g = (T *)ctx->data_tmp.p;
            HIPCHK(ctx, launch_tt_source<T>(g, d1, m.w, coef, lag, m.nt, m.ntr, ctx->stream));
        }
        if ((rc = m.finish(g, &J)) ||
            (rc = m.per_trace(tau_out, (const double *)ctx->tt_coef.p, lag_out, (const int32_t *)ctx->tt_lag.p)))
            return rc;
        *J_out = J;
        return FWI_OK;
    }

    // s' = B d_syn, d' = B d_obs, W_j the squared 2-Wasserstein distance between the weighted traces M s', M d' made
    // positive and normalised to densities along time, J = 1/2 sum_j w_j W_j, r = B g where the adjoint sweep reads its
    // amplitudes (fwi_ot.h)
    static int misfit_transport(fwi_ctx *ctx, const T *d_obs, const T *weights, const double *taps, int R,
                                const double *trace_weights, int transform, double param, double *J_out, double *w2_out,
                                int32_t *counts_out) {
        Misfit m(ctx);
        double J = 0.0;
        T *g = nullptr;
        const double *w2 = nullptr;  // the distances W_j within the work array
        int rc = m.begin(d_obs, weights, taps, R);
        if (rc) return rc;
        if (m.data) {
            if ((rc = ensure(ctx, ctx->ot_work, ot_work_doubles(m.nt, m.ntr) * sizeof(double))) ||
                (rc = ensure(ctx, ctx->ot_counts, (size_t)m.ntr * sizeof(int32_t))))
                return rc;
            const double *tw;
            if ((rc = m.trace_weights(trace_weights, &tw))) return rc;
            double *work = (double *)ctx->ot_work.p;
            m.sum = work + ot_total_at(m.nt, m.ntr);  // the total of the terms 1/2 w_j W_j: J itself
            w2 = work + ot_w2_at(m.nt, m.ntr);
            const T *s1, *d1;
            if ((rc = m.prefilter(&s1, &d1))) return rc;
            g = m.adjoint_source();  // in place of s' (with taps) or of d_obs (without): elementwise, written last
            HIPCHK(ctx, launch_ot_misfit<T>(work, (int32_t *)ctx->ot_counts.p, g, s1, d1, m.w, tw, transform, param,
                                            ctx->cfg.dt, m.nt, m.ntr, ctx->stream));
        }
        if ((rc = m.finish(g, &J)) || (rc = m.per_trace(w2_out, w2, counts_out, (const int32_t *)ctx->ot_counts.p))) return rc;
        *J_out = J;
        return FWI_OK;
    }

    // s' = B d_syn, d' = B d_obs, w_j the Wiener filter with w_j * (M d') ~= M s' per trace (normal equations G_j w_j = c_j
    // from the lag correlations, solved by Cholesky on the device), W_j its second moment about zero lag over its energy,
    // J = 1/2 sum_j w_j W_j, r = B g where the adjoint sweep reads its amplitudes (fwi_awi.h)
    static int misfit_adaptive(fwi_ctx *ctx, const T *d_obs, const T *weights, const double *taps, int R,
                               const double *trace_weights, int L, double lam, double *J_out, double *w2_out,
                               int32_t *counts_out, double *filters_out) {
        Misfit m(ctx);
        double J = 0.0;
        T *g = nullptr;
        const double *w2 = nullptr, *filters = nullptr;  // W_j and the filters within the work array
        int rc = m.begin(d_obs, weights, taps, R);
        if (rc) return rc;
        const size_t nfilt = (size_t)m.ntr * (2 * L + 1);
        if (m.data) {
            if ((rc = ensure(ctx, ctx->awi_part, awi_partials(m.nt, m.ntr, L) * sizeof(double))) ||
                (rc = ensure(ctx, ctx->awi_work, awi_work_doubles(m.ntr, L) * sizeof(double))) ||
                (rc = ensure(ctx, ctx->awi_counts, (size_t)m.ntr * sizeof(int32_t))))
                return rc;
            const double *tw;
            if ((rc = m.trace_weights(trace_weights, &tw))) return rc;
            double *part = (double *)ctx->awi_part.p, *work = (double *)ctx->awi_work.p;
            int32_t *counts = (int32_t *)ctx->awi_counts.p;
            m.sum = work + awi_total_at(m.ntr, L);  // the total of the terms 1/2 w_j W_j: J itself
            w2 = work + awi_w2_at(m.ntr, L), filters = work + awi_w_at(m.ntr, L);
            const T *s1, *d1;
            if ((rc = m.prefilter(&s1, &d1))) return rc;
            // the events around the three phases (fwi_misfit_adaptive_ms): recorded, never waited for here
            ctx->have_awi_ms = false;
            for (hipEvent_t &ev : ctx->awi_ev)
                if (!ev) HIPCHK(ctx, hipEventCreate(&ev));
            HIPCHK(ctx, hipEventRecord(ctx->awi_ev[0], ctx->stream));
            HIPCHK(ctx, launch_awi_correlations<T>(part, s1, d1, m.w, L, m.nt, m.ntr, ctx->stream));
            HIPCHK(ctx, hipEventRecord(ctx->awi_ev[1], ctx->stream));
            HIPCHK(ctx, launch_awi_solve(work, counts, part, tw, ctx->cfg.dt, lam, L, m.nt, m.ntr, ctx->stream));
            HIPCHK(ctx, hipEventRecord(ctx->awi_ev[2], ctx->stream));
            // g reads d' at shifted rows, and without taps adjoint_source() IS d': g goes to the spare gather buffer, and
            // finish() filters (with taps) or copies (without) it into place
            g = (T *)ctx->data_tmp.p;
            HIPCHK(ctx, launch_awi_source<T>(g, d1, m.w, work, counts, L, m.nt, m.ntr, ctx->stream));
            HIPCHK(ctx, hipEventRecord(ctx->awi_ev[3], ctx->stream));
            ctx->have_awi_ms = true;
        }
        if ((rc = m.finish(g, &J)) || (rc = m.per_trace(w2_out, w2, counts_out, (const int32_t *)ctx->awi_counts.p)))
            return rc;
        if (filters_out) {  // (ntr, 2 L + 1); without receivers or samples no trace counts: zeros
            if (!m.data) {
                std::fill(filters_out, filters_out + nfilt, 0.0);
            } else {
                HIPCHK(ctx, hipMemcpyAsync(filters_out, filters, nfilt * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
                HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
            }
        }
        *J_out = J;
        return FWI_OK;
    }

    // The twiddles of fwi_misfit_spectral, formed in fp64 as fourier_table forms the store's (from the fractional part of
    // f_k n dt) and kept on the context: block k, row n = (cos theta_kn, sin theta_kn), the rows from nt on zero
    // (spec_table_rows).  Rebuilt only when nt or the frequencies change.
    static int spectral_table(fwi_ctx *ctx, int nt, int F, const double *freqs) {
        if (ctx->spec_table.p && ctx->spec_table_nt == nt && ctx->spec_table_freqs.size() == (size_t)F &&
            std::equal(freqs, freqs + F, ctx->spec_table_freqs.begin()))
            return FWI_OK;
        const int rows = spec_table_rows(nt);
        ctx->spec_table_nt = 0;  // no table until the new one is complete
        if (int rc = ensure(ctx, ctx->spec_table, spec_table_doubles(nt, F) * sizeof(double)))
            return rc;
        std::vector<double> &t = ctx->spec_table_host;
        t.assign(spec_table_doubles(nt, F), 0.0);
        for (int k = 0; k < F; ++k)
            for (int n = 0; n < nt; ++n) {
                const double x = freqs[k] * ctx->cfg.dt * n, th = 2.0 * M_PI * (x - std::floor(x));
                t[((size_t)k * rows + n) * 2] = std::cos(th);
                t[((size_t)k * rows + n) * 2 + 1] = std::sin(th);
            }
        HIPCHK(ctx, hipMemcpyAsync(ctx->spec_table.p, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        ctx->spec_table_nt = nt;
        ctx->spec_table_freqs.assign(freqs, freqs + F);
        return FWI_OK;
    }

    // s' = B d_syn, d' = B d_obs, S_kj and O_kj the Fourier coefficients of the weighted traces M s', M d' at the F
    // frequencies, J the sum over the pairs (k, j) of the terms of `kind`, r = B g where the adjoint sweep reads its
    // amplitudes (fwi_spec.h)
    static int misfit_spectral(fwi_ctx *ctx, const T *d_obs, const T *weights, const double *taps, int R, int F,
                               const double *freqs, int kind, double eps, const double *freq_weights,
                               const double *trace_weights, double *J_out, double *phase_out, double *logamp_out,
                               uint8_t *counts_out) {
        Misfit m(ctx);
        double J = 0.0;
        T *g = nullptr;
        int rc = m.begin(d_obs, weights, taps, R);
        if (rc) return rc;
        const size_t npair = (size_t)F * m.ntr;
        if (m.data) {
            if ((rc = ensure(ctx, ctx->spec_part, spec_partials(m.nt, m.ntr, F) * sizeof(double))) ||
                (rc = ensure(ctx, ctx->spec_coef, spec_coef_doubles(m.ntr, F) * sizeof(double))) ||
                (rc = ensure(ctx, ctx->spec_counts, npair)) ||
                (rc = spectral_table(ctx, m.nt, F, freqs)))
                return rc;
            const double *tw, *fw = nullptr;
            if ((rc = m.trace_weights(trace_weights, &tw))) return rc;
            if (freq_weights) {
                if ((rc = ensure(ctx, ctx->spec_fw, (size_t)F * sizeof(double)))) return rc;
                // (the caller's pageable memory: the copy is complete before anything that can fail and return follows it)
                HIPCHK(ctx, hipMemcpyAsync(ctx->spec_fw.p, freq_weights, (size_t)F * sizeof(double), hipMemcpyHostToDevice,
                                           ctx->stream));
                HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
                fw = (const double *)ctx->spec_fw.p;
            }
            double *part = (double *)ctx->spec_part.p, *coef = (double *)ctx->spec_coef.p;
            const double *table = (const double *)ctx->spec_table.p;
            m.sum = coef + spec_total_at(m.ntr, F);  // the total of the terms of J: J itself
            const T *s1, *d1;
            if ((rc = m.prefilter(&s1, &d1))) return rc;
            HIPCHK(ctx, launch_spec_analysis<T>(part, s1, d1, m.w, table, F, m.nt, m.ntr, ctx->stream));
            HIPCHK(ctx, launch_spec_coeffs(coef, (uint8_t *)ctx->spec_counts.p, part, fw, tw, kind, eps, F, m.nt, m.ntr,
                                           ctx->stream));
            g = m.adjoint_source();  // in place of s' (with taps) or of d_obs (without): both are used up
            HIPCHK(ctx, launch_spec_source<T>(g, m.w, coef, table, F, m.nt, m.ntr, ctx->stream));
        }
        if ((rc = m.finish(g, &J))) return rc;
        // the three (F, ntr) outputs under one synchronise; without receivers or samples no pair counts: zeros
        if (!m.data) {
            if (phase_out) std::fill(phase_out, phase_out + npair, 0.0);
            if (logamp_out) std::fill(logamp_out, logamp_out + npair, 0.0);
            if (counts_out) std::fill(counts_out, counts_out + npair, (uint8_t)0);
        } else if (phase_out || logamp_out || counts_out) {
            const double *coef = (const double *)ctx->spec_coef.p;
            if (phase_out)
                HIPCHK(ctx, hipMemcpyAsync(phase_out, coef + spec_phase_at(m.ntr, F), npair * sizeof(double),
                                           hipMemcpyDeviceToHost, ctx->stream));
            if (logamp_out)
                HIPCHK(ctx, hipMemcpyAsync(logamp_out, coef + spec_logamp_at(m.ntr, F), npair * sizeof(double),
                                           hipMemcpyDeviceToHost, ctx->stream));
            if (counts_out)
                HIPCHK(ctx, hipMemcpyAsync(counts_out, ctx->spec_counts.p, npair, hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        }
        *J_out = J;
        return FWI_OK;
    }

    // device residual := B M^2 B residual: per node, or per off-grid point and scattered onto the nodes again
    static int residual_weight(fwi_ctx *ctx, const T *weights, const double *taps, int R) {
        const fwi_ctx::SpreadSet &sp = ctx->rec_sp;
        const int nt = ctx->nt, ntr = sp.npts ? sp.npts : ctx->nrec;
        if (!ctx->nrec || !nt || !ntr) return FWI_OK;
        void *resid = ctx->amp.p;
        if (sp.npts) {
            if (ctx->resid_pts_in == fwi_ctx::RESID_PTS_NONE)
                return ctx->fail(FWI_ESTATE, "fwi_residual_weight: the residual's per-point series were not kept "
                                             "(off-grid receivers): weight it on the host");
            resid = ctx->resid_pts_in == fwi_ctx::RESID_PTS_A ? ctx->pts_a.p : ctx->pts_d.p;
        }
        int rc, Re;
        const T *w;
        const double *b;
        if ((rc = data_prepare(ctx, weights, taps, R, nt, ntr, &w, &b, &Re))) return rc;
        HIPCHK(ctx, launch_fir_time<T>((T *)ctx->data_tmp.p, (const T *)resid, nullptr, nullptr, w, b, Re, nt, ntr, nullptr,
                                       false, ctx->stream));
        HIPCHK(ctx, launch_fir_time<T>((T *)resid, (const T *)ctx->data_tmp.p, nullptr, w, nullptr, b, Re, nt, ntr, nullptr,
                                       false, ctx->stream));
        if (sp.npts)
            HIPCHK(ctx, launch_scatter_series<T>((const T *)resid, (T *)ctx->amp.p, (const int *)sp.owner,
                                                 (const T *)sp.weight, nt, sp.npts, ctx->nrec, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        return FWI_OK;
    }

    // e = M . B (d_syn - d_obs) as fwi_misfit_weighted's, J = sum_j tw_j sum_n rho(e; a_j), g = tw_j psi e in place of e,
    // r = B (M . g) where the adjoint sweep reads its amplitudes (fwi_robust.h).  keep: W = tw_j M^2 psi stays in
    // ctx->robust_w for fwi_residual_weight_robust; whatever W was held goes with the call.
    static int misfit_robust(fwi_ctx *ctx, const T *d_obs, const T *weights, const double *taps, int R, int kind,
                             const double *thresh, const double *trace_weights, int keep, double *jtrace_out,
                             int32_t *nout_out, double *J_out) {
        Misfit m(ctx);
        double J = 0.0;
        ctx->have_irls = false;
        int rc = m.begin(d_obs, weights, taps, R);
        if (rc) return rc;
        const size_t tiles_ntr = (size_t)robust_tiles(m.nt) * m.ntr;
        if (m.data) {
            if ((rc = ensure(ctx, ctx->robust_part, robust_partials(m.nt, m.ntr) * sizeof(double))) ||
                (rc = ensure(ctx, ctx->robust_cnt, robust_counts(m.nt, m.ntr) * sizeof(int32_t))) ||
                (rc = ensure(ctx, ctx->robust_thresh, (size_t)m.ntr * sizeof(double))) ||
                (keep && (rc = ensure(ctx, ctx->robust_w, m.n * sizeof(T)))))
                return rc;
            const double *tw;
            if ((rc = m.trace_weights(trace_weights, &tw))) return rc;
            // (the caller's pageable memory: the copy is complete before anything that can fail and return follows it)
            HIPCHK(ctx, hipMemcpyAsync(ctx->robust_thresh.p, thresh, (size_t)m.ntr * sizeof(double), hipMemcpyHostToDevice,
                                       ctx->stream));
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
            T *e = (T *)ctx->data_tmp.p;
            HIPCHK(ctx, launch_fir_time<T>(e, m.syn, m.resid, nullptr, m.w, m.b, m.Re, m.nt, m.ntr, nullptr, false,
                                           ctx->stream));
            // the block sums and their total go where fwi_misfit_weighted's go: m.sum is J itself
            HIPCHK(ctx, launch_robust_source<T>(e, keep ? (T *)ctx->robust_w.p : nullptr, e, m.w,
                                                (const double *)ctx->robust_thresh.p, tw, kind,
                                                (double *)ctx->robust_part.p, (int32_t *)ctx->robust_cnt.p, m.part, m.nt,
                                                m.ntr, ctx->stream));
            HIPCHK(ctx, launch_robust_terms((double *)ctx->robust_part.p, (int32_t *)ctx->robust_cnt.p, tw, m.nt, m.ntr,
                                            ctx->stream));
            HIPCHK(ctx, launch_fir_time<T>(m.resid, e, nullptr, m.w, nullptr, m.b, m.Re, m.nt, m.ntr, nullptr, false,
                                           ctx->stream));
        }
        if ((rc = m.finish(m.resid, &J)) ||
            (rc = m.per_trace(jtrace_out, (const double *)ctx->robust_part.p + tiles_ntr, nout_out,
                              (const int32_t *)ctx->robust_cnt.p + tiles_ntr)))
            return rc;
        ctx->have_irls = keep != 0;
        *J_out = J;
        return FWI_OK;
    }

    // the lower median of |e|, e as above, per trace or of the whole gather; no residual is left on the device
    static int residual_median(fwi_ctx *ctx, const T *d_obs, const T *weights, const double *taps, int R, int segment,
                               double *med_out, int64_t *count_out) {
        Misfit m(ctx);
        int rc = m.begin(d_obs, weights, taps, R);
        if (rc) return rc;
        const size_t nseg = segment ? 1 : (size_t)m.ntr;
        if (!m.data) {
            std::fill(med_out, med_out + nseg, 0.0);
            std::fill(count_out, count_out + nseg, (int64_t)0);
            return FWI_OK;
        }
        if ((rc = ensure(ctx, ctx->robust_med, nseg * (sizeof(double) + sizeof(int64_t)) + median_all_work()))) return rc;
        double *med = (double *)ctx->robust_med.p;
        int64_t *count = (int64_t *)(med + nseg);
        T *e = (T *)ctx->data_tmp.p;
        HIPCHK(ctx, launch_fir_time<T>(e, m.syn, m.resid, nullptr, m.w, m.b, m.Re, m.nt, m.ntr, nullptr, false, ctx->stream));
        if (segment)
            HIPCHK(ctx, launch_median_all<T>(med, count, count + nseg, e, m.w, (int64_t)m.n, ctx->stream));
        else
            HIPCHK(ctx, launch_median_traces<T>(med, count, e, m.w, m.nt, m.ntr, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(med_out, med, nseg * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(count_out, count, nseg * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        return FWI_OK;
    }

    // where the residual on the device lies: per node, or per off-grid point (nullptr: those series were not kept)
    static void *device_residual(fwi_ctx *ctx) {
        if (!ctx->rec_sp.npts) return ctx->amp.p;
        if (ctx->resid_pts_in == fwi_ctx::RESID_PTS_NONE) return nullptr;
        return ctx->resid_pts_in == fwi_ctx::RESID_PTS_A ? ctx->pts_a.p : ctx->pts_d.p;
    }

    // device residual := B (W . (B residual)), W the kept IRLS weight: per node, or per off-grid point and scattered
    static int residual_weight_robust(fwi_ctx *ctx, const double *taps, int R) {
        const fwi_ctx::SpreadSet &sp = ctx->rec_sp;
        const int nt = ctx->nt, ntr = sp.npts ? sp.npts : ctx->nrec;
        if (!ctx->nrec || !nt || !ntr) return FWI_OK;
        void *resid = device_residual(ctx);
        if (!resid)
            return ctx->fail(FWI_ESTATE, "fwi_residual_weight_robust: the residual's per-point series were not kept "
                                         "(off-grid receivers): weight it on the host");
        int rc, Re;
        const T *w;
        const double *b;
        if ((rc = data_prepare(ctx, nullptr, taps, R, nt, ntr, &w, &b, &Re))) return rc;
        HIPCHK(ctx, launch_fir_time<T>((T *)ctx->data_tmp.p, (const T *)resid, nullptr, nullptr, (const T *)ctx->robust_w.p,
                                       b, Re, nt, ntr, nullptr, false, ctx->stream));
        HIPCHK(ctx, launch_fir_time<T>((T *)resid, (const T *)ctx->data_tmp.p, nullptr, nullptr, nullptr, b, Re, nt, ntr,
                                       nullptr, false, ctx->stream));
        if (sp.npts)
            HIPCHK(ctx, launch_scatter_series<T>((const T *)resid, (T *)ctx->amp.p, (const int *)sp.owner,
                                                 (const T *)sp.weight, nt, sp.npts, ctx->nrec, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        return FWI_OK;
    }
};

}  // namespace

// An array of the caller's in the context's dtype, as DISPATCH_CALL hands it to Impl<T>: const float * or const double *
struct typed {
    const void *p;
    explicit typed(const void *q) : p(q) {}
    template <typename T> operator const T *() const { return (const T *)p; }
};

extern "C" {

// The checks every data misfit begins with: a forward run to compare, and the arguments all of them take (`out`: J_out,
// or nullptr where another mandatory pointer is null).
static int misfit_callable(fwi_ctx *ctx, const char *who, const void *d_obs, const void *out) {
    if (!ctx) return FWI_EINVAL;
    if (!ctx->have_forward) return ctx->fail(FWI_ESTATE, "%s: no forward run whose data to compare", who);
    if (!out || (ctx->nrec && !d_obs)) return ctx->fail(FWI_EINVAL, "%s: null argument", who);
    return FWI_OK;
}

// ... and the one they end with, after their own parameters: the synthetics are still there (`also`: what else, besides
// an fwi_adjoint, the entry point names as having overwritten them).  Selects the device.
static int misfit_synthetics(fwi_ctx *ctx, const char *who, const char *also) {
    if (!ctx->have_syn)
        return ctx->fail(FWI_ESTATE, "%s: the synthetics of the last forward are gone (an fwi_adjoint %shas run since): "
                                     "call it between fwi_forward and fwi_adjoint", who, also);
    (void)hipSetDevice(ctx->cfg.device);
    return FWI_OK;
}

int fwi_misfit_l2(fwi_ctx *ctx, const void *d_obs, double *J_out) {
    if (int rc = misfit_callable(ctx, "fwi_misfit_l2", d_obs, J_out)) return rc;
    if (int rc = misfit_synthetics(ctx, "fwi_misfit_l2", "")) return rc;
    return DISPATCH_CALL(ctx, misfit_l2, typed(d_obs), J_out);
}

static int data_args(fwi_ctx *ctx, const char *who, const double *taps, int32_t R) {
    if (R < 0 || R > FIR_RMAX) return ctx->fail(FWI_EINVAL, "%s: R=%d outside [0, %d]", who, (int)R, FIR_RMAX);
    if (R > 0 && !taps) return ctx->fail(FWI_EINVAL, "%s: null taps with R=%d", who, (int)R);
    return FWI_OK;
}

// the weights per trace, one per node receiver or per off-grid point (nullptr: none)
static int trace_weight_args(fwi_ctx *ctx, const char *who, const double *trace_weights) {
    if (!trace_weights || !ctx->nrec) return FWI_OK;
    const int ntr = ctx->rec_sp.npts ? ctx->rec_sp.npts : ctx->nrec;
    for (int j = 0; j < ntr; ++j)
        if (!(trace_weights[j] >= 0.0) || !std::isfinite(trace_weights[j]))
            return ctx->fail(FWI_EINVAL, "%s: trace_weights[%d]=%g must be finite and >= 0", who, j, trace_weights[j]);
    return FWI_OK;
}

// a scalar parameter `name` that must be finite and >= 0 (`positive`: > 0)
static int nonneg_finite(fwi_ctx *ctx, const char *who, const char *name, double v, bool positive = false) {
    if (std::isfinite(v) && (positive ? v > 0.0 : v >= 0.0)) return FWI_OK;
    return ctx->fail(FWI_EINVAL, "%s: %s=%g must be finite and %s 0", who, name, v, positive ? ">" : ">=");
}

int fwi_misfit_weighted(fwi_ctx *ctx, const void *d_obs, const void *weights, const double *taps, int32_t R,
                        double *J_out) {
    if (int rc = misfit_callable(ctx, "fwi_misfit_weighted", d_obs, J_out)) return rc;
    if (int rc = data_args(ctx, "fwi_misfit_weighted", taps, R)) return rc;
    if (int rc = misfit_synthetics(ctx, "fwi_misfit_weighted", "or fwi_born ")) return rc;
    return DISPATCH_CALL(ctx, misfit_weighted, typed(d_obs), typed(weights), taps, R, J_out);
}

int fwi_misfit_matched(fwi_ctx *ctx, const void *d_obs, const void *weights, const double *taps, int32_t R, int32_t L,
                       double mu, const double *f_in, double *f_out, double *normal_out, double *J_out) {
    if (int rc = misfit_callable(ctx, "fwi_misfit_matched", d_obs, J_out)) return rc;
    if (int rc = data_args(ctx, "fwi_misfit_matched", taps, R)) return rc;
    if (L < 0 || L > FWI_MATCH_LMAX)
        return ctx->fail(FWI_EINVAL, "fwi_misfit_matched: L=%d outside [0, %d]", (int)L, FWI_MATCH_LMAX);
    if (int rc = nonneg_finite(ctx, "fwi_misfit_matched", "mu", mu)) return rc;
    if (f_in)
        for (int k = 0; k < 2 * L + 1; ++k)
            if (!std::isfinite(f_in[k])) return ctx->fail(FWI_EINVAL, "fwi_misfit_matched: f_in[%d] is not finite", k);
    if (int rc = misfit_synthetics(ctx, "fwi_misfit_matched", "or fwi_born ")) return rc;
    return DISPATCH_CALL(ctx, misfit_matched, typed(d_obs), typed(weights), taps, R, L, mu, f_in, f_out, normal_out, J_out);
}

int fwi_misfit_envelope(fwi_ctx *ctx, const void *d_obs, const void *weights, const double *taps, int32_t R,
                        const double *hilbert, int32_t Q, int32_t power, double eps, double *J_out) {
    if (int rc = misfit_callable(ctx, "fwi_misfit_envelope", d_obs, hilbert ? J_out : nullptr)) return rc;
    if (int rc = data_args(ctx, "fwi_misfit_envelope", taps, R)) return rc;
    if (Q < 1 || Q > FIR_RMAX) return ctx->fail(FWI_EINVAL, "fwi_misfit_envelope: Q=%d outside [1, %d]", (int)Q, FIR_RMAX);
    for (int k = 0; k < Q; ++k)
        if (!std::isfinite(hilbert[k])) return ctx->fail(FWI_EINVAL, "fwi_misfit_envelope: hilbert[%d] is not finite", k);
    if (power != 1 && power != 2) return ctx->fail(FWI_EINVAL, "fwi_misfit_envelope: power=%d is neither 1 nor 2", (int)power);
    if (int rc = nonneg_finite(ctx, "fwi_misfit_envelope", "eps", eps)) return rc;
    if (power == 1 && eps == 0.0)
        return ctx->fail(FWI_EINVAL, "fwi_misfit_envelope: power 1 needs eps > 0 (the envelope is not differentiable at 0)");
    if (int rc = misfit_synthetics(ctx, "fwi_misfit_envelope", "or fwi_born ")) return rc;
    return DISPATCH_CALL(ctx, misfit_envelope, typed(d_obs), typed(weights), taps, R, hilbert, Q, power, eps, J_out);
}

int fwi_misfit_correlation(fwi_ctx *ctx, const void *d_obs, const void *weights, const double *taps, int32_t R,
                           const double *trace_weights, double eps, double *J_out, double *rho_out) {
    if (int rc = misfit_callable(ctx, "fwi_misfit_correlation", d_obs, J_out)) return rc;
    if (int rc = data_args(ctx, "fwi_misfit_correlation", taps, R)) return rc;
    if (int rc = nonneg_finite(ctx, "fwi_misfit_correlation", "eps", eps)) return rc;
    if (int rc = trace_weight_args(ctx, "fwi_misfit_correlation", trace_weights)) return rc;
    if (int rc = misfit_synthetics(ctx, "fwi_misfit_correlation", "or fwi_born ")) return rc;
    return DISPATCH_CALL(ctx, misfit_correlation, typed(d_obs), typed(weights), taps, R, trace_weights, eps, J_out, rho_out);
}

int fwi_misfit_traveltime(fwi_ctx *ctx, const void *d_obs, const void *weights, const double *taps, int32_t R,
                          const double *trace_weights, int32_t max_lag, double *J_out, double *tau_out, int32_t *lag_out) {
    if (int rc = misfit_callable(ctx, "fwi_misfit_traveltime", d_obs, J_out)) return rc;
    if (int rc = data_args(ctx, "fwi_misfit_traveltime", taps, R)) return rc;
    if (max_lag < 1 || max_lag > FWI_TT_KMAX)
        return ctx->fail(FWI_EINVAL, "fwi_misfit_traveltime: max_lag=%d outside [1, %d]", (int)max_lag, FWI_TT_KMAX);
    if (int rc = trace_weight_args(ctx, "fwi_misfit_traveltime", trace_weights)) return rc;
    if (int rc = misfit_synthetics(ctx, "fwi_misfit_traveltime", "or fwi_born ")) return rc;
    return DISPATCH_CALL(ctx, misfit_traveltime, typed(d_obs), typed(weights), taps, R, trace_weights, max_lag, J_out,
                         tau_out, lag_out);
}

int fwi_misfit_transport(fwi_ctx *ctx, const void *d_obs, const void *weights, const double *taps, int32_t R,
                         const double *trace_weights, int32_t transform, double param, double *J_out, double *w2_out,
                         int32_t *counts_out) {
    if (int rc = misfit_callable(ctx, "fwi_misfit_transport", d_obs, J_out)) return rc;
    if (int rc = data_args(ctx, "fwi_misfit_transport", taps, R)) return rc;
    if (transform != FWI_OT_LINEAR && transform != FWI_OT_SOFTPLUS)
        return ctx->fail(FWI_EINVAL, "fwi_misfit_transport: transform=%d is neither FWI_OT_LINEAR nor FWI_OT_SOFTPLUS",
                         (int)transform);
    if (int rc = nonneg_finite(ctx, "fwi_misfit_transport", "param", param, true)) return rc;
    if (int rc = trace_weight_args(ctx, "fwi_misfit_transport", trace_weights)) return rc;
    if (int rc = misfit_synthetics(ctx, "fwi_misfit_transport", "or fwi_born ")) return rc;
    return DISPATCH_CALL(ctx, misfit_transport, typed(d_obs), typed(weights), taps, R, trace_weights, transform, param,
                         J_out, w2_out, counts_out);
}

int fwi_misfit_spectral(fwi_ctx *ctx, const void *d_obs, const void *weights, const double *taps, int32_t R,
                        int32_t nfreq, const double *freqs_hz, int32_t kind, double eps, const double *freq_weights,
                        const double *trace_weights, double *J_out, double *phase_out, double *logamp_out,
                        uint8_t *counts_out) {
    const char *who = "fwi_misfit_spectral";
    if (int rc = misfit_callable(ctx, who, d_obs, J_out)) return rc;
    if (int rc = data_args(ctx, who, taps, R)) return rc;
    if (nfreq < 1 || nfreq > FWI_FOURIER_FMAX)
        return ctx->fail(FWI_EINVAL, "%s: nfreq=%d outside [1, %d]", who, (int)nfreq, FWI_FOURIER_FMAX);
    if (!freqs_hz) return ctx->fail(FWI_EINVAL, "%s: null frequencies", who);
    if (kind != FWI_SPEC_L2 && kind != FWI_SPEC_PHASE && kind != FWI_SPEC_LOGAMP && kind != FWI_SPEC_LOG)
        return ctx->fail(FWI_EINVAL, "%s: kind=%d is none of FWI_SPEC_L2, FWI_SPEC_PHASE, FWI_SPEC_LOGAMP, FWI_SPEC_LOG", who,
                         (int)kind);
    const bool phase = kind == FWI_SPEC_PHASE || kind == FWI_SPEC_LOG;
    const double nyq = 1.0 / (2.0 * ctx->cfg.dt);
    for (int k = 0; k < nfreq; ++k) {
        const double f = freqs_hz[k];
        if (!std::isfinite(f)) return ctx->fail(FWI_EINVAL, "%s: frequency %d is not finite", who, k);
        if (f < 0.0) return ctx->fail(FWI_EINVAL, "%s: frequency %d is negative (%g Hz)", who, k, f);
        if (f > nyq * (1.0 + FOURIER_NYQUIST_RTOL))
            return ctx->fail(FWI_EINVAL, "%s: frequency %d (%g Hz) is above the Nyquist frequency %g Hz (dt %g s)", who, k, f,
                             nyq, ctx->cfg.dt);
        if (phase && (f == 0.0 || std::fabs(2.0 * f * ctx->cfg.dt - 1.0) <= FOURIER_NYQUIST_RTOL))
            return ctx->fail(FWI_EINVAL, "%s: frequency %d (%g Hz) is 0 or the Nyquist frequency, where the spectrum is real "
                                         "and has no phase to compare (kinds PHASE and LOG)", who, k, f);
        for (int m = 0; m < k; ++m)
            if (freqs_hz[m] == f) return ctx->fail(FWI_EINVAL, "%s: frequencies %d and %d are equal (%g Hz)", who, m, k, f);
    }
    if (int rc = nonneg_finite(ctx, who, "eps", eps)) return rc;
    if (freq_weights)
        for (int k = 0; k < nfreq; ++k)
            if (!(freq_weights[k] >= 0.0) || !std::isfinite(freq_weights[k]))
                return ctx->fail(FWI_EINVAL, "%s: freq_weights[%d]=%g must be finite and >= 0", who, k, freq_weights[k]);
    if (int rc = trace_weight_args(ctx, who, trace_weights)) return rc;
    if (int rc = misfit_synthetics(ctx, who, "or fwi_born ")) return rc;
    return DISPATCH_CALL(ctx, misfit_spectral, typed(d_obs), typed(weights), taps, R, nfreq, freqs_hz, kind, eps,
                         freq_weights, trace_weights, J_out, phase_out, logamp_out, counts_out);
}

int fwi_misfit_adaptive(fwi_ctx *ctx, const void *d_obs, const void *weights, const double *taps, int32_t R,
                        const double *trace_weights, int32_t L, double lam, double *J_out, double *w2_out,
                        int32_t *counts_out, double *filters_out) {
    if (int rc = misfit_callable(ctx, "fwi_misfit_adaptive", d_obs, J_out)) return rc;
    if (int rc = data_args(ctx, "fwi_misfit_adaptive", taps, R)) return rc;
    static_assert(FWI_AWI_LMAX == AWI_LMAX, "include/fwi.h and fwi_awi.h disagree");
    if (L < 1 || L > FWI_AWI_LMAX)
        return ctx->fail(FWI_EINVAL, "fwi_misfit_adaptive: L=%d outside [1, %d]", (int)L, FWI_AWI_LMAX);
    if (int rc = nonneg_finite(ctx, "fwi_misfit_adaptive", "lam", lam, true)) return rc;
    if (int rc = trace_weight_args(ctx, "fwi_misfit_adaptive", trace_weights)) return rc;
    if (int rc = misfit_synthetics(ctx, "fwi_misfit_adaptive", "or fwi_born ")) return rc;
    return DISPATCH_CALL(ctx, misfit_adaptive, typed(d_obs), typed(weights), taps, R, trace_weights, L, lam, J_out, w2_out,
                         counts_out, filters_out);
}

int fwi_misfit_adaptive_ms(fwi_ctx *ctx, double *ms_out) {
    if (!ctx) return FWI_EINVAL;
    if (!ms_out) return ctx->fail(FWI_EINVAL, "fwi_misfit_adaptive_ms: null argument");
    if (!ctx->have_awi_ms)
        return ctx->fail(FWI_ESTATE, "fwi_misfit_adaptive_ms: no fwi_misfit_adaptive call with receivers has launched its "
                                     "kernels");
    (void)hipSetDevice(ctx->cfg.device);
    HIPCHK(ctx, hipEventSynchronize(ctx->awi_ev[3]));
    for (int i = 0; i < 3; ++i) {
        float ms = 0.f;
        HIPCHK(ctx, hipEventElapsedTime(&ms, ctx->awi_ev[i], ctx->awi_ev[i + 1]));
        ms_out[i] = (double)ms;
    }
    return FWI_OK;
}

int fwi_match_solve(const double *G, const double *b, int32_t K, double mu, double *f_out) {
    return match_solve(G, b, K, mu, f_out) ? FWI_EINVAL : FWI_OK;
}

int fwi_residual_weight(fwi_ctx *ctx, const void *weights, const double *taps, int32_t R) {
    if (!ctx) return FWI_EINVAL;
    if (int rc = data_args(ctx, "fwi_residual_weight", taps, R)) return rc;
    if (!ctx->have_dev_residual)
        return ctx->fail(FWI_ESTATE, "fwi_residual_weight: no residual on the device (fwi_born, fwi_misfit_l2 or "
                                     "fwi_misfit_weighted leave one; fwi_adjoint uses it up)");
    (void)hipSetDevice(ctx->cfg.device);
    return DISPATCH_CALL(ctx, residual_weight, typed(weights), taps, R);
}

int fwi_misfit_robust(fwi_ctx *ctx, const void *d_obs, const void *weights, const double *taps, int32_t R, int32_t kind,
                      const double *thresh, const double *trace_weights, int32_t keep_irls, double *J_trace_out,
                      int32_t *nout_out, double *J_out) {
    const char *who = "fwi_misfit_robust";
    if (int rc = misfit_callable(ctx, who, d_obs, J_out)) return rc;
    if (int rc = data_args(ctx, who, taps, R)) return rc;
    static_assert(FWI_ROBUST_HUBER == ROBUST_HUBER && FWI_ROBUST_HYBRID == ROBUST_HYBRID &&
                  FWI_ROBUST_CAUCHY == ROBUST_CAUCHY, "include/fwi.h and fwi_robust.h disagree");
    if (kind != FWI_ROBUST_HUBER && kind != FWI_ROBUST_HYBRID && kind != FWI_ROBUST_CAUCHY)
        return ctx->fail(FWI_EINVAL, "%s: kind=%d is none of FWI_ROBUST_HUBER, FWI_ROBUST_HYBRID, FWI_ROBUST_CAUCHY", who,
                         (int)kind);
    if (ctx->nrec) {
        if (!thresh) return ctx->fail(FWI_EINVAL, "%s: null thresholds", who);
        const int ntr = ctx->rec_sp.npts ? ctx->rec_sp.npts : ctx->nrec;
        for (int j = 0; j < ntr; ++j) {
            if (!(thresh[j] > 0.0)) return ctx->fail(FWI_EINVAL, "%s: thresh[%d]=%g must be > 0", who, j, thresh[j]);
            if (std::isinf(thresh[j]) && kind != FWI_ROBUST_HUBER)
                return ctx->fail(FWI_EINVAL, "%s: thresh[%d] is infinite, which only FWI_ROBUST_HUBER takes", who, j);
        }
    }
    if (int rc = trace_weight_args(ctx, who, trace_weights)) return rc;
    if (int rc = misfit_synthetics(ctx, who, "or fwi_born ")) return rc;
    return DISPATCH_CALL(ctx, misfit_robust, typed(d_obs), typed(weights), taps, R, kind, thresh, trace_weights, keep_irls,
                         J_trace_out, nout_out, J_out);
}

int fwi_residual_median(fwi_ctx *ctx, const void *d_obs, const void *weights, const double *taps, int32_t R,
                        int32_t segment, double *med_out, int64_t *count_out) {
    const char *who = "fwi_residual_median";
    if (int rc = misfit_callable(ctx, who, d_obs, count_out ? (const void *)med_out : nullptr)) return rc;
    if (int rc = data_args(ctx, who, taps, R)) return rc;
    if (segment != 0 && segment != 1)
        return ctx->fail(FWI_EINVAL, "%s: segment=%d is neither 0 (per trace) nor 1 (the whole gather)", who, (int)segment);
    if (int rc = misfit_synthetics(ctx, who, "or fwi_born ")) return rc;
    return DISPATCH_CALL(ctx, residual_median, typed(d_obs), typed(weights), taps, R, segment, med_out, count_out);
}

int fwi_residual_weight_robust(fwi_ctx *ctx, const double *taps, int32_t R) {
    if (!ctx) return FWI_EINVAL;
    if (int rc = data_args(ctx, "fwi_residual_weight_robust", taps, R)) return rc;
    if (!ctx->have_irls)
        return ctx->fail(FWI_ESTATE, "fwi_residual_weight_robust: no IRLS weight is held (fwi_misfit_robust with keep_irls "
                                     "leaves one; the next forward drops it)");
    if (!ctx->have_dev_residual)
        return ctx->fail(FWI_ESTATE, "fwi_residual_weight_robust: no residual on the device (fwi_born or a misfit call "
                                     "leaves one; fwi_adjoint uses it up)");
    (void)hipSetDevice(ctx->cfg.device);
    return DISPATCH_CALL(ctx, residual_weight_robust, taps, R);
}

}  // extern "C"
