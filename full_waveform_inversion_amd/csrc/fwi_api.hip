// C-ABI of the engine (include/fwi.h): context, device memory, time loops.  Host-side runtime only; the arithmetic is in
// fwi_kernels.hip.  The calls that run no time loop have their own units over the same context (fwi_host.h):
// fwi_api_misfit.hip, fwi_api_fourier.hip, fwi_api_vec.hip and fwi_api_comm.hip (the RCCL exchange).
//
// No reference counterpart (the reference has neither a native layer nor this
// path); the entry points are the ones BASELINE.json's
// north_star names.  The time loop mirrors oracle/fwi_oracle.py::_propagate
// one-to-one so the parity tests can compare every intermediate.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <type_traits>

#include "fwi_host.h"
#include "fwi_points.h"
#include "fwi_born.h"
#include "fwi_fourier.h"
#include "fwi_fimage.h"
#include "fwi_fbornx.h"
#include "fwi_illum.h"

namespace {

thread_local std::string g_create_error;

const double COEF2[] = {-2.0, 1.0};
const double COEF4[] = {-5.0 / 2.0, 4.0 / 3.0, -1.0 / 12.0};
const double COEF8[] = {-205.0 / 72.0, 8.0 / 5.0, -1.0 / 5.0, 8.0 / 315.0, -1.0 / 560.0};
// centred first-difference weights d_1 .. d_r (CPML)
const double DCOEF2[] = {1.0 / 2.0};
const double DCOEF4[] = {2.0 / 3.0, -1.0 / 12.0};
const double DCOEF8[] = {4.0 / 5.0, -1.0 / 5.0, 4.0 / 105.0, -1.0 / 280.0};
static_assert(FWI_FOURIER_BMAX == FOURIER_BMAX, "batch limit of the ABI and of the kernels");

void profile(std::vector<double> &p, int n, int npml, double sigma_max, double dt) {
    p.assign(n, 0.0);
    if (npml <= 0) return;
    for (int i = 0; i < n; ++i) {
        double dist = std::max(0.0, std::max((double)npml - i, (double)i - (n - 1 - npml)));
        p[i] = 0.5 * dt * sigma_max * (dist / npml) * (dist / npml);
    }
}

template <typename T>
int upload_vec(fwi_ctx *ctx, void *dst, const std::vector<double> &v) {
    std::vector<T> t(v.begin(), v.end());
    HIPCHK(ctx, hipMemcpyAsync(dst, t.data(), t.size() * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return FWI_OK;
}

// Time series cross the PCIe boundary through a persistent pinned staging buffer: the caller's
// NumPy arrays are pageable and usually freshly mapped, and the driver's pageable path cost up to
// tens of ms per 2 MB copy (measured in the 2-D shot loop).
int stage_reserve(fwi_ctx *ctx, size_t bytes) {
    if (ctx->cap_pin >= bytes && ctx->pin) return FWI_OK;
    if (ctx->pin) {
        // an H2D copy out of the buffer may still be queued on the stream (forward: the wavelet upload)
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        HIPCHK(ctx, hipHostFree(ctx->pin));
    }
    ctx->pin = nullptr;
    HIPCHK(ctx, hipHostMalloc(&ctx->pin, bytes ? bytes : 16, hipHostMallocDefault));
    ctx->cap_pin = bytes;
    return FWI_OK;
}

}  // namespace

namespace fwi {

int upload_series(fwi_ctx *ctx, void *dst, const void *src, size_t bytes) {
    if (!bytes) return FWI_OK;
    int rc = stage_reserve(ctx, bytes);
    if (rc) return rc;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // the staging buffer may still be in flight
    memcpy(ctx->pin, src, bytes);
    HIPCHK(ctx, hipMemcpyAsync(dst, ctx->pin, bytes, hipMemcpyHostToDevice, ctx->stream));
    return FWI_OK;
}

int ensure(fwi_ctx *ctx, Buf &b, size_t bytes) {
    if (b.cap >= bytes && b.p) return FWI_OK;
    int rc;
    if ((rc = dev_release(ctx, &b.p, b.member)) || (rc = dev_acquire(ctx, &b.p, bytes ? bytes : 16, b.member, b.index)))
        return rc;
    b.cap = bytes;
    return FWI_OK;
}

// the block partials (and their total) of the fixed-order sums (launch_dot, launch_residual_l2): allocated on first use
int sum_partials(fwi_ctx *ctx, double **part) {
    const int rc = dev_first_use(ctx, &ctx->sum_part, (size_t)(SUM_MAX_BLOCKS + 1) * sizeof(double), "sum_part");
    *part = (double *)ctx->sum_part;
    return rc;
}

// Host arrays are model-shaped (row stride nx); compact device arrays have row stride cx (nx
// rounded up to 4, pad columns zero).  Equal for nx % 4 == 0: one plain copy.  Otherwise the
// contiguous array goes through a device staging buffer and a repack kernel.
template <typename T>
int upload_compact(fwi_ctx *ctx, void *dst, const void *host) {
    const GridDesc &g = ctx->gd;
    if (g.cx == g.nx) {
        HIPCHK(ctx, hipMemcpyAsync(dst, host, (size_t)g.npts * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
        return FWI_OK;
    }
    const size_t nlog = (size_t)g.nz * g.ny * g.nx;
    if (int rc = dev_first_use(ctx, &ctx->logical, nlog * sizeof(T), "logical")) return rc;
    HIPCHK(ctx, hipMemcpyAsync(ctx->logical, host, nlog * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, launch_repack<T>(g, (T *)dst, (const T *)ctx->logical, 1, ctx->stream));
    return FWI_OK;
}

template <typename T>
int download_compact(fwi_ctx *ctx, void *host, const void *src) {
    const GridDesc &g = ctx->gd;
    if (g.cx == g.nx) {
        HIPCHK(ctx, hipMemcpyAsync(host, src, (size_t)g.npts * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
        return FWI_OK;
    }
    const size_t nlog = (size_t)g.nz * g.ny * g.nx;
    if (int rc = dev_first_use(ctx, &ctx->logical, nlog * sizeof(T), "logical")) return rc;
    HIPCHK(ctx, launch_repack<T>(g, (T *)ctx->logical, (const T *)src, 0, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(host, ctx->logical, nlog * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
    return FWI_OK;
}

template int upload_compact<float>(fwi_ctx *, void *, const void *);
template int upload_compact<double>(fwi_ctx *, void *, const void *);
template int download_compact<float>(fwi_ctx *, void *, const void *);
template int download_compact<double>(fwi_ctx *, void *, const void *);

}  // namespace fwi

namespace {

// device -> caller; synchronises the stream
int download_series(fwi_ctx *ctx, void *dst, const void *src, size_t bytes) {
    if (bytes) {
        int rc = stage_reserve(ctx, bytes);
        if (rc) return rc;
        HIPCHK(ctx, hipMemcpyAsync(ctx->pin, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (bytes) memcpy(dst, ctx->pin, bytes);
    return FWI_OK;
}

// ensure for a group of plain pointers of `bytes` each that share one capacity: `member`[index0], [index0 + 1], ...
int ensure_all(fwi_ctx *ctx, const char *member, int index0, std::initializer_list<void **> group, size_t *cap,
               size_t bytes) {
    if (*cap >= bytes && std::all_of(group.begin(), group.end(), [](void **p) { return *p != nullptr; })) return FWI_OK;
    int rc;
    for (void **p : group)
        if ((rc = dev_release(ctx, p, member)) || (rc = dev_acquire(ctx, p, bytes ? bytes : 16, member, index0++)))
            return rc;
    *cap = bytes;
    return FWI_OK;
}

// All-or-nothing device allocation: every entry of `want` with bytes (entries of none are skipped), `zero` ones cleared on
// the context's stream, provided their sum fits into the free memory.  FWI_ENOMEM without a message where it does not fit
// or an allocation fails: whatever was allocated is freed again, every pointer is null, and the caller reports *total
// against *free_bytes in its own words.
struct Want {
    void **p;
    const char *member;
    size_t bytes;
    bool zero;
    int index = 0;
};
int alloc_all(fwi_ctx *ctx, std::initializer_list<Want> want, size_t *total, size_t *free_bytes) {
    size_t device_bytes = 0;
    *total = 0;
    for (const Want &w : want) *total += w.bytes;
    HIPCHK(ctx, hipMemGetInfo(free_bytes, &device_bytes));
    int e = hipSuccess;
    if (*total <= *free_bytes)
        for (const Want &w : want) {
            if (!w.bytes) continue;
            if ((e = ctx->mem.acquire(w.p, w.bytes, w.member, w.index)) != hipSuccess) break;
            if (w.zero && (e = hipMemsetAsync(*w.p, 0, w.bytes, ctx->stream)) != hipSuccess) break;
        }
    if (*total <= *free_bytes && e == hipSuccess) return FWI_OK;
    (void)hipGetLastError();
    for (const Want &w : want) (void)ctx->mem.release(w.p);
    return FWI_ENOMEM;
}

// The time loop of one sweep, either submitted launch by launch or captured into a hipGraph and launched once
// (fwi_config.launch_mode).  begin() stands where the loop's first launch is about to be formed, end() behind its
// last one; between them only kernel launches and device-to-device copies on ctx->stream may happen (true of
// run_steps / run_fused / run_pairs, the checkpoint copies and the record / imaging tails).  A TimeLoop that goes out
// of scope inside a capture (an error return) ends the capture and drops the partial graph.
struct TimeLoop {
    fwi_ctx *ctx;
    bool capturing = false;
    std::chrono::steady_clock::time_point t0;
    explicit TimeLoop(fwi_ctx *c) : ctx(c) {}
    int begin() {
        t0 = std::chrono::steady_clock::now();
        ctx->host_graph_ms = 0.0;
        if (ctx->graph_exec) {  // the previous sweep's graph: finished by now or not, the stream orders us behind it
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
            (void)hipGraphExecDestroy(ctx->graph_exec);
            ctx->graph_exec = nullptr;
        }
        if (ctx->graph) {
            (void)hipGraphDestroy(ctx->graph);
            ctx->graph = nullptr;
        }
        if (ctx->graph_mode) {
            HIPCHK(ctx, hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
            capturing = true;
        } else {
            HIPCHK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
        }
        return FWI_OK;
    }
    int end() {
        if (capturing) {
            capturing = false;
            HIPCHK(ctx, hipStreamEndCapture(ctx->stream, &ctx->graph));
            HIPCHK(ctx, hipGraphInstantiate(&ctx->graph_exec, ctx->graph, nullptr, nullptr, 0));
            ctx->host_graph_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            HIPCHK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
            HIPCHK(ctx, hipGraphLaunch(ctx->graph_exec, ctx->stream));
        }
        HIPCHK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
        ctx->host_submit_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        ctx->have_loop_time = true;
        return FWI_OK;
    }
    ~TimeLoop() {
        if (capturing) {
            hipGraph_t g = nullptr;
            (void)hipStreamEndCapture(ctx->stream, &g);
            if (g) (void)hipGraphDestroy(g);
            (void)hipGetLastError();
        }
    }
};

// v in a table's order: out[k] = v[col[k]]
template <typename V>
std::vector<V> permuted(const std::vector<V> &v, const std::vector<int> &col) {
    std::vector<V> out(col.size());
    for (size_t k = 0; k < col.size(); ++k) out[k] = v[col[k]];
    return out;
}

template <typename T>
struct Impl {
    // State of one field pair being stepped: which buffer holds the newest field, and the step
    // whose sampling is still owed (it rides on the next launch).
    struct Sweep {
        void *f[2];
        int cur = 0;
        int prev_n = -1;
        void *v = nullptr;  // increment form: the v field of this sweep
        bool pml_fw = false;  // CPML: this sweep is the checkpointed forward recomputation (its own memory variables)
        const void *born_w = nullptr;  // fused Born sweep: w (compact); the step kernel adds w q_in(n) inside q
    };

    static StepArgs<T> base_args(fwi_ctx *ctx, int cur) {
        StepArgs<T> a;
        a.u_cur = (const T *)ctx->u[cur];
        a.u_prev = (T *)ctx->u[cur ^ 1];
        a.v = nullptr;
        a.C = (const T *)ctx->C;
        a.dz = (const T *)ctx->dz;
        a.dy = (const T *)ctx->dy;
        a.dx = (const T *)ctx->dx;
        a.q_out = nullptr;
        a.q_in = nullptr;
        a.q_in2 = nullptr;
        a.q_bf16 = ctx->qbf16 ? 1 : 0;
        a.g = (T *)ctx->g_acc;
        // Star weights NORMALISED by a_1 (the factor a_1 / h^2 lives in the padded C, see finish_model): in fp32 the
        // rounded a_k / h^2 are a systematic perturbation of the operator -- a phase error growing with omega T that
        // was the largest term of the fp32 seismogram error (2-D layered 256^2 x 1000 steps in emulation: 3.4e-6 ->
        // 1.8e-6 standard form, 2.9e-6 -> 7.7e-7 increment form).  Normalised, a_1 -> 1 and a_2 -> -1/8 (O(8)) or
        // -1/16 (O(4)) are exact and the inexact a_3, a_4 weigh 0.016 and 0.0011: their rounding no longer matters.
        const double *co = ctx->cfg.order == 2 ? COEF2 : ctx->cfg.order == 4 ? COEF4 : COEF8;
        for (int k = 0; k < 5; ++k) a.ck[k] = T(0);
        for (int k = 1; k <= ctx->gd.r; ++k) a.ck[k] = (T)(co[k] / co[1]);
        a.damp = ctx->cfg.npml > 0 && !ctx->cpml;
        a.npml = ctx->cfg.npml;
        a.dz_scale = a.damp ? (T)(0.5 * ctx->cfg.dt * ctx->cfg.sigma_max /
                                  ((double)ctx->cfg.npml * ctx->cfg.npml)) : T(0);
        a.pml_tz = a.pml_ty = nullptr;
        a.xp_mode = 0;
        a.xp_partial = 0;
        a.xp_psi = a.xp_zeta = nullptr;
        a.xp_a = a.xp_b = nullptr;
        for (int k = 0; k < 5; ++k) a.xp_dk[k] = a.xp_dk1[k] = T(0);
        a.inj_start = nullptr;
        a.inj_pidx = a.inj_cidx = nullptr;
        a.inj_cu = a.inj_cq = a.inj_amp = nullptr;
        a.inj_col = nullptr;
        a.inj_run = nullptr;
        a.rec_pidx = nullptr;
        a.rec_out = nullptr;
        a.rec_scale = T(0);
        a.nrec = 0;
        return a;
    }

    // caller's per-point (or per-node) series -> the per-node device array `dst` (nt x nnodes)
    static int upload_amplitudes(fwi_ctx *ctx, void *dst, const void *host, int nt, int nnodes,
                                 const fwi_ctx::SpreadSet &sp) {
        if (sp.npts == 0) return upload_series(ctx, dst, host, (size_t)nt * nnodes * sizeof(T));
        int rc = ensure(ctx, ctx->pts_a, (size_t)nt * sp.npts * sizeof(T));
        if (rc) return rc;
        if ((rc = upload_series(ctx, ctx->pts_a.p, host, (size_t)nt * sp.npts * sizeof(T)))) return rc;
        HIPCHK(ctx, launch_scatter_series<T>((const T *)ctx->pts_a.p, (T *)dst, (const int *)sp.owner, (const T *)sp.weight,
                                             nt, sp.npts, nnodes, ctx->stream));
        return FWI_OK;
    }

    // the per-node device series `src` (nt x nnodes) -> the caller, per node or gathered per point; `keep` (or
    // nullptr) receives the device copy of what was handed out
    static int download_samples(fwi_ctx *ctx, void *host, const void *src, int nt, int nnodes,
                                const fwi_ctx::SpreadSet &sp, Buf *keep) {
        if (sp.npts == 0) return download_series(ctx, host, src, host ? (size_t)nt * nnodes * sizeof(T) : 0);
        Buf &buf = keep ? *keep : ctx->pts_a;
        int rc = ensure(ctx, buf, (size_t)nt * sp.npts * sizeof(T));
        if (rc) return rc;
        HIPCHK(ctx, launch_gather_series<T>((const T *)src, (T *)buf.p, (const int *)sp.pt_start, (const T *)sp.weight, nt,
                                            sp.npts, nnodes, ctx->stream));
        return download_series(ctx, host, buf.p, host ? (size_t)nt * sp.npts * sizeof(T) : 0);
    }

    static PmlArgs<T> pml_args(fwi_ctx *ctx, const Sweep &sw, T *q_out) {
        PmlArgs<T> p;
        p.u_cur = (const T *)sw.f[sw.cur];
        p.u_next = (T *)sw.f[sw.cur ^ 1];
        p.v = (T *)sw.v;
        p.C = (const T *)ctx->C;
        p.q_out = q_out;
        for (int d = 0; d < 3; ++d) {
            p.psi[d] = (T *)(sw.pml_fw ? ctx->pml_psi_fw[d] : ctx->pml_psi[d]);
            p.zeta[d] = (T *)(sw.pml_fw ? ctx->pml_zeta_fw[d] : ctx->pml_zeta[d]);
            p.a[d] = (const T *)ctx->pml_a[d];
            p.b[d] = (const T *)ctx->pml_b[d];
        }
        const double *co = ctx->cfg.order == 2 ? COEF2 : ctx->cfg.order == 4 ? COEF4 : COEF8;
        const double *dc = ctx->cfg.order == 2 ? DCOEF2 : ctx->cfg.order == 4 ? DCOEF4 : DCOEF8;
        // The padded C carries a_1 / h^2 (base_args), so the border term is formed times s = h^2 / a_1: the second
        // differences take the normalised weights, the first differences that act on the FIELD (inside the psi / pt
        // recursions) take dk1 = s d_k / h, those that act on a memory variable the plain d_k / h.  The memory
        // variables are thereby carried times s, which nothing outside these kernels sees.
        const double h = ctx->cfg.h;
        for (int k = 0; k < 5; ++k) p.ck[k] = p.dk[k] = p.dk1[k] = T(0);
        for (int k = 0; k <= ctx->gd.r; ++k) p.ck[k] = (T)(co[k] / co[1]);
        for (int k = 1; k <= ctx->gd.r; ++k) {
            p.dk[k] = (T)(dc[k - 1] / h);
            p.dk1[k] = (T)(dc[k - 1] * h / co[1]);
        }
        p.npml = ctx->cfg.npml;
        p.tz = (T *)ctx->pml_tz;
        p.ty = (T *)ctx->pml_ty;
        return p;
    }

    // the memory variables <-> snapshot `seg` (forward set when `fw`, else the main set: the plain forward sweep)
    static int pml_snapshot(fwi_ctx *ctx, int seg, bool fw, bool restore) {
        char *base = (char *)ctx->pml_snap + (size_t)seg * ctx->pml_snap_stride;
        size_t off = 0;
        for (int d = 0; d < 3; ++d) {
            if (!ctx->pml_psi[d]) continue;
            for (void *arr : {fw ? ctx->pml_psi_fw[d] : ctx->pml_psi[d], fw ? ctx->pml_zeta_fw[d] : ctx->pml_zeta[d]}) {
                if (restore)
                    HIPCHK(ctx, hipMemcpyAsync(arr, base + off, ctx->pml_bytes[d], hipMemcpyDeviceToDevice, ctx->stream));
                else
                    HIPCHK(ctx, hipMemcpyAsync(base + off, arr, ctx->pml_bytes[d], hipMemcpyDeviceToDevice, ctx->stream));
                off += ctx->pml_bytes[d];
            }
        }
        return FWI_OK;
    }

    static int pml_zero(fwi_ctx *ctx) {
        for (int d = 0; d < 3; ++d)
            if (ctx->pml_psi[d]) {
                HIPCHK(ctx, hipMemsetAsync(ctx->pml_psi[d], 0, ctx->pml_bytes[d], ctx->stream));
                HIPCHK(ctx, hipMemsetAsync(ctx->pml_zeta[d], 0, ctx->pml_bytes[d], ctx->stream));
            }
        return FWI_OK;
    }

    static int set_model(fwi_ctx *ctx, const T *c) {
        // compact H2D copy, then validation + padded C = dt^2 c^2 on the device (the halo of C
        // was zeroed at creation and is never written)
        int rc = upload_compact<T>(ctx, ctx->c_dev, c);
        if (rc) return rc;
        return finish_model(ctx);
    }

    static int set_model_vec(fwi_ctx *ctx, const void *dev) {
        HIPCHK(ctx, hipMemcpyAsync(ctx->c_dev, dev, (size_t)ctx->gd.npts * sizeof(T), hipMemcpyDeviceToDevice,
                                   ctx->stream));
        return finish_model(ctx);
    }

    static int finish_model(fwi_ctx *ctx) {
        const GridDesc &g = ctx->gd;
        hipStream_t s = ctx->stream;
        int *bad = (int *)(ctx->red + 4);
        HIPCHK(ctx, hipMemsetAsync(bad, 0, sizeof(int), s));
        // padded C = dt^2 c^2 a_1 / h^2: the kernels' star weights are normalised by a_1 (base_args)
        const double *co = ctx->cfg.order == 2 ? COEF2 : ctx->cfg.order == 4 ? COEF4 : COEF8;
        HIPCHK(ctx, launch_build_model<T>(g, (const T *)ctx->c_dev, (T *)ctx->C,
                                          ctx->cfg.dt * ctx->cfg.dt * co[1] / (ctx->cfg.h * ctx->cfg.h), bad, s));
        int nbad = 0;
        HIPCHK(ctx, hipMemcpyAsync(&nbad, bad, sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
        ctx->have_forward = false;
        if (nbad) {
            ctx->have_model = false;
            return ctx->fail(FWI_EINVAL, "velocity must be finite and > 0 (%d bad entries)", nbad);
        }
        ctx->have_model = true;
        return FWI_OK;
    }

    // coefficient of an injected amplitude in u (A*C*scale) and in q (C*scale)
    static void point_coefs(fwi_ctx *ctx, const int32_t *idx, int n, double scale, const std::vector<T> &cpt,
                            std::vector<T> &cu, std::vector<T> &cq) {
        const GridDesc &g = ctx->gd;
        const double dt2 = ctx->cfg.dt * ctx->cfg.dt;
        cu.resize(n);
        cq.resize(n);
        for (int i = 0; i < n; ++i) {
            const int32_t *t = idx + (size_t)i * g.ndim;
            const int z = t[0], y = (g.ndim == 3) ? t[1] : 0, x = t[g.ndim - 1];
            const double cv = (double)cpt[i];
            const double d = ctx->pz[z] + ((g.ndim == 3) ? ctx->py[y] : 0.0) + ctx->px[x];
            const double Cv = dt2 * cv * cv;  // dt^2 c^2 itself (the padded C of the kernels carries a_1 / h^2 as well)
            cq[i] = (T)(Cv * scale);
            cu[i] = (T)(Cv * scale / (1.0 + d));
        }
    }

    static int upload_set(fwi_ctx *ctx, fwi_ctx::PointSet &ps, int32_t n, const int32_t *idx,
                          double scale) {
        FlatPoints flat;
        const int outside = flatten(ctx->gd, idx, n, &flat);
        if (outside >= 0) return ctx->fail(FWI_EINVAL, "grid index %d outside the grid", outside);
        int rcode;
        const size_t need = (size_t)n * 8 + 16;
        if ((rcode = ensure_all(ctx, ps.member, 0, {&ps.pidx, &ps.cidx, &ps.cu, &ps.cq, &ps.s_pidx, &ps.s_cidx, &ps.s_cu,
                                                    &ps.s_cq, &ps.s_col, &ps.s_run}, &ps.cap, need)))
            return rcode;
        auto up = [&](void *d, const void *h, size_t b) {
            return b ? hipMemcpyAsync(d, h, b, hipMemcpyHostToDevice, ctx->stream) : hipSuccess;
        };
        HIPCHK(ctx, up(ps.pidx, flat.pidx.data(), (size_t)n * 8));
        HIPCHK(ctx, up(ps.cidx, flat.cidx.data(), (size_t)n * 8));
        // velocities at the points: gathered from the device copy of the model
        std::vector<T> cpt(n), cu, cq;
        if (n) {
            HIPCHK(ctx, launch_record<T>((const T *)ctx->c_dev, (const int64_t *)ps.cidx, (T *)ps.cu, T(1), n,
                                         ctx->stream));
            HIPCHK(ctx, hipMemcpyAsync(cpt.data(), ps.cu, (size_t)n * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        }
        point_coefs(ctx, idx, n, scale, cpt, cu, cq);
        HIPCHK(ctx, up(ps.cu, cu.data(), (size_t)n * sizeof(T)));
        HIPCHK(ctx, up(ps.cq, cq.data(), (size_t)n * sizeof(T)));

        // the tables (fwi_points.h) and the coefficients in each table's order; all of it lives until the last copy is done
        StepTable st;
        Fused2dTables ft;
        Pair3dTable pt;
        step_table(*ctx, idx, n, flat, &st);
        const std::vector<T> scu = permuted(cu, st.col), scq = permuted(cq, st.col);
        std::vector<int64_t> fcidx;
        std::vector<T> fcu, fcq;
        if (ctx->fused2d) {
            fused2d_tables(*ctx, idx, n, &ft);
            fcidx = permuted(flat.cidx, ft.col);
            fcu = permuted(cu, ft.col);
            fcq = permuted(cq, ft.col);
        }
        if (ctx->pair3d) {  // (fp32 contexts only, plan_context)
            pair3d_table(*ctx, idx, n, &pt);
            for (Pair3dInj &e : pt.ent) e.cu = (float)cu[e.col];
        }

        const size_t sb = st.start.size() * sizeof(int);
        if ((rcode = ensure(ctx, ps.s_start, sb))) return rcode;
        HIPCHK(ctx, up(ps.s_start.p, st.start.data(), sb));
        HIPCHK(ctx, up(ps.s_pidx, st.pidx.data(), (size_t)n * 8));
        HIPCHK(ctx, up(ps.s_cidx, st.cidx.data(), (size_t)n * 8));
        HIPCHK(ctx, up(ps.s_cu, scu.data(), (size_t)n * sizeof(T)));
        HIPCHK(ctx, up(ps.s_cq, scq.data(), (size_t)n * sizeof(T)));
        HIPCHK(ctx, up(ps.s_col, st.col.data(), (size_t)n * sizeof(int)));
        HIPCHK(ctx, up(ps.s_run, st.run.data(), (size_t)n * sizeof(int)));
        if (ctx->fused2d) {
            const size_t ne = ft.col.size(), nr = ft.rcol.size();
            const size_t fneed = ne * 8 + 16, sneed = ft.start.size() * sizeof(int);
            if ((rcode = ensure_all(ctx, ps.member, 11, {&ps.fi_lz, &ps.fi_lx, &ps.fi_col, &ps.fi_int, &ps.fi_cidx, &ps.fi_cu,
                                                         &ps.fi_cq, &ps.fi_run, &ps.fr_lz, &ps.fr_lx, &ps.fr_col},
                                    &ps.fcap, fneed)) ||
                (rcode = ensure_all(ctx, ps.member, 22, {&ps.fi_start, &ps.fr_start}, &ps.fcap_start, sneed)))
                return rcode;
            HIPCHK(ctx, up(ps.fi_start, ft.start.data(), sneed));
            HIPCHK(ctx, up(ps.fr_start, ft.rstart.data(), sneed));
            HIPCHK(ctx, up(ps.fi_lz, ft.lz.data(), ne * sizeof(int)));
            HIPCHK(ctx, up(ps.fi_lx, ft.lx.data(), ne * sizeof(int)));
            HIPCHK(ctx, up(ps.fi_col, ft.col.data(), ne * sizeof(int)));
            HIPCHK(ctx, up(ps.fi_int, ft.interior.data(), ne));
            HIPCHK(ctx, up(ps.fi_cidx, fcidx.data(), ne * 8));
            HIPCHK(ctx, up(ps.fi_cu, fcu.data(), ne * sizeof(T)));
            HIPCHK(ctx, up(ps.fi_cq, fcq.data(), ne * sizeof(T)));
            HIPCHK(ctx, up(ps.fi_run, ft.run.data(), ne * sizeof(int)));
            HIPCHK(ctx, up(ps.fr_lz, ft.rlz.data(), nr * sizeof(int)));
            HIPCHK(ctx, up(ps.fr_lx, ft.rlx.data(), nr * sizeof(int)));
            HIPCHK(ctx, up(ps.fr_col, ft.rcol.data(), nr * sizeof(int)));
        }
        if (ctx->pair3d) {  // (fp32 contexts only, plan_context)
            const size_t pb = pt.start.size() * sizeof(int), eb = pt.ent.size() * sizeof(Pair3dInj);
            if ((rcode = ensure(ctx, ps.pr_start, pb)) || (rcode = ensure(ctx, ps.pr_ent, eb + 16))) return rcode;
            HIPCHK(ctx, up(ps.pr_start.p, pt.start.data(), pb));
            HIPCHK(ctx, up(ps.pr_ent.p, pt.ent.data(), eb));
        }
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // host vectors go out of scope
        ps.n = n;
        return FWI_OK;
    }

    // 3-D temporal blocking: `count` (even) forward steps from n0, two per pass, ping-ponging between the buffer
    // pair in `sw` and `spare`.  Both new fields are sampled by the next pass; the last pair by the caller's
    // flush_record (newest field) and one explicit record here (the older one).
    static int run_pairs(fwi_ctx *ctx, Sweep &sw, void **spare, int n0, int count, const fwi_ctx::PointSet &inj,
                         const T *amp, const fwi_ctx::PointSet *out, T *series, T out_scale) {
        if constexpr (std::is_same<T, float>::value) {
            const GridDesc &g = ctx->gd;
            const StepArgs<T> b = base_args(ctx, 0);
            for (int done = 0; done < count; done += 2) {
                const int n = n0 + done;
                Pair3dArgs a{};
                a.u_cur = (const float *)sw.f[sw.cur];
                a.u_prev = (const float *)sw.f[sw.cur ^ 1];
                a.C = (const float *)ctx->C;
                a.out2 = (float *)spare[0];
                a.out1 = (float *)spare[1];
                a.dy = (const float *)ctx->dy;
                a.dx = (const float *)ctx->dx;
                for (int k = 0; k < 5; ++k) a.ck[k] = b.ck[k];
                a.damp = b.damp;
                a.npml = b.npml;
                a.dz_scale = b.dz_scale;
                if (inj.n > 0) {
                    a.inj_start = (const int *)inj.pr_start.p;
                    a.inj = (const Pair3dInj *)inj.pr_ent.p;
                    a.inj_amp0 = amp + (size_t)n * inj.n;
                    a.inj_amp1 = amp + (size_t)(n + 1) * inj.n;
                }
                if (out && out->n > 0 && done > 0) {  // the previous pass' fields: steps n - 2 and n - 1
                    a.rec_pidx = (const int64_t *)out->pidx;
                    a.rec_out0 = series + (size_t)(n - 2) * out->n;
                    a.rec_out1 = series + (size_t)(n - 1) * out->n;
                    a.rec_scale = out_scale;
                    a.nrec = out->n;
                }
                HIPCHK(ctx, launch_pair3d(g, a, ctx->pair_zc, ctx->pair_tw, ctx->stream));
                void *oc = sw.f[sw.cur], *op = sw.f[sw.cur ^ 1];
                sw.f[0] = spare[0];  // u^{n+2}
                sw.f[1] = spare[1];  // u^{n+1}
                sw.cur = 0;
                spare[0] = oc;
                spare[1] = op;
            }
            if (out && out->n > 0 && count > 0)
                HIPCHK(ctx, launch_record<T>((const T *)sw.f[1], (const int64_t *)out->pidx,
                                             series + (size_t)(n0 + count - 2) * out->n, out_scale, out->n, ctx->stream));
            sw.prev_n = count > 0 ? n0 + count - 1 : sw.prev_n;
            return FWI_OK;
        } else {
            (void)sw; (void)spare; (void)n0; (void)count; (void)inj; (void)amp; (void)out; (void)series; (void)out_scale;
            return ctx->fail(FWI_ESTATE, "3-D two-step path is fp32 only");
        }
    }

    // 2-D temporal blocking: `count` steps (a multiple of FUSED2D_STEPS) starting at n0 in direction
    // dn, FUSED2D_STEPS per launch, ping-ponging between the buffer pair in `sw` and ctx->fx.
    // Sampling is not lagged here (it happens inside the sub-steps): sw.prev_n stays -1.
    static int run_fused(fwi_ctx *ctx, Sweep &sw, void **spare, int n0, int dn, int count,
                         const fwi_ctx::PointSet &inj, const T *amp, const fwi_ctx::PointSet *out, T *series,
                         T out_scale, int mode, T *q_base) {
        if constexpr (std::is_same<T, float>::value) {
            const GridDesc &g = ctx->gd;
            const StepArgs<T> b = base_args(ctx, 0);
            for (int done = 0; done < count; done += FUSED2D_STEPS) {
                Fused2dArgs a{};
                a.u_cur = (const float *)sw.f[sw.cur];
                a.u_prev = (const float *)(ctx->inc ? sw.v : sw.f[sw.cur ^ 1]);  // increment form: v in / v out
                a.inc = ctx->inc ? 1 : 0;
                a.skipd = ctx->fused_skipd;
                a.ft = ctx->fused_ft;
                a.tile_order = ctx->fused_order;
                a.C = (const float *)ctx->C;
                a.out_cur = (float *)spare[0];
                a.out_prev = (float *)spare[1];
                a.dz = (const float *)ctx->dz;
                a.dx = (const float *)ctx->dx;
                for (int k = 0; k < 5; ++k) a.ck[k] = b.ck[k];
                a.damp = b.damp;
                a.mode = mode;
                a.q_base = (float *)q_base;
                a.istride = ctx->istride;
                a.g = (float *)ctx->g_acc;
                a.n0 = n0 + done * dn;
                a.dn = dn;
                if (inj.n > 0) {
                    a.inj_start = (const int *)inj.fi_start;
                    a.inj_lz = (const int *)inj.fi_lz;
                    a.inj_lx = (const int *)inj.fi_lx;
                    a.inj_col = (const int *)inj.fi_col;
                    a.inj_interior = (const unsigned char *)inj.fi_int;
                    a.inj_run = (const int *)inj.fi_run;
                    a.inj_cidx = (const int64_t *)inj.fi_cidx;
                    a.inj_cu = (const float *)inj.fi_cu;
                    a.inj_cq = (const float *)inj.fi_cq;
                    a.inj_amp = (const float *)amp;
                    a.ninj = inj.n;
                }
                if (out && out->n > 0) {
                    a.rec_start = (const int *)out->fr_start;
                    a.rec_lz = (const int *)out->fr_lz;
                    a.rec_lx = (const int *)out->fr_lx;
                    a.rec_col = (const int *)out->fr_col;
                    a.rec_out = (float *)series;
                    a.rec_scale = out_scale;
                    a.nrec = out->n;
                }
                if (ctx->cpml) {  // the border recursion inside the launch (fwi_fused2d_pml.hip)
                    const PmlArgs<T> p = pml_args(ctx, sw, nullptr);
                    a.pml_npml = p.npml;
                    a.pml_rev = dn < 0;
                    for (int d = 0; d < 2; ++d) {  // z -> 0, x -> 1
                        a.pml_psi[d] = (float *)p.psi[d ? 2 : 0];
                        a.pml_zeta[d] = (float *)p.zeta[d ? 2 : 0];
                        a.pml_psi_out[d] = (float *)ctx->pml_spare_psi[d ? 2 : 0];
                        a.pml_zeta_out[d] = (float *)ctx->pml_spare_zeta[d ? 2 : 0];
                        a.pml_a[d] = (const float *)p.a[d ? 2 : 0];
                        a.pml_b[d] = (const float *)p.b[d ? 2 : 0];
                    }
                    for (int k = 0; k < 5; ++k) {
                        a.pml_dk[k] = (float)p.dk[k];
                        a.pml_dk1[k] = (float)p.dk1[k];
                    }
                    HIPCHK(ctx, launch_fused2d_cpml(g, a, ctx->stream));
                    for (int d : {0, 2}) {  // the written set becomes the current one of this sweep
                        std::swap(sw.pml_fw ? ctx->pml_psi_fw[d] : ctx->pml_psi[d], ctx->pml_spare_psi[d]);
                        std::swap(sw.pml_fw ? ctx->pml_zeta_fw[d] : ctx->pml_zeta[d], ctx->pml_spare_zeta[d]);
                    }
                } else {
                    HIPCHK(ctx, launch_fused2d(g, a, ctx->stream));
                }
                if (ctx->inc) {
                    // (u, v) written into the spare pair; the old u and v buffers become the next launch's output.
                    // The second u buffer of the sweep (the single-step kernels' output) is not involved.
                    void *ou = sw.f[sw.cur], *ov = sw.v;
                    sw.f[sw.cur] = spare[0];
                    sw.v = spare[1];
                    spare[0] = ou;
                    spare[1] = ov;
                    continue;
                }
                // the freshly written pair becomes current; the old pair is the next launch's output
                void *oc = sw.f[sw.cur], *op = sw.f[sw.cur ^ 1];
                sw.f[0] = spare[0];
                sw.f[1] = spare[1];
                sw.cur = 0;
                spare[0] = oc;
                spare[1] = op;
            }
            sw.prev_n = -1;
            return FWI_OK;
        } else {
            (void)sw; (void)spare; (void)n0; (void)dn; (void)count; (void)inj; (void)amp; (void)out; (void)series;
            (void)out_scale; (void)mode; (void)q_base;
            return ctx->fail(FWI_ESTATE, "fused 2-D path is fp32 only");
        }
    }

    // (never on a sweep that writes or reads the Fourier store, fwi_ctx::four_sweep: its transforms sit between single steps)
    static bool use_fused(const fwi_ctx *ctx, int nt) {
        return ctx->fused2d && !ctx->four_sweep && nt % FUSED2D_STEPS == 0 &&
               (ctx->ckpt == 0 || ctx->ckpt % FUSED2D_STEPS == 0);
    }

    // Steps taken by the fused kernel when nt is not a multiple of FUSED2D_STEPS (store-all mode only): the
    // first nt - nt % FUSED2D_STEPS; the remaining 1-3 steps go one per launch.  0 = not applicable.
    static int mixed_fused_steps(const fwi_ctx *ctx, int nt) {
        if (!ctx->fused2d || ctx->four_sweep || ctx->ckpt != 0 || nt % FUSED2D_STEPS == 0) return 0;
        return nt - nt % FUSED2D_STEPS;
    }

    static int upload_points(fwi_ctx *ctx, int32_t nsrc, const int32_t *src_idx, int32_t nrec,
                             const int32_t *rec_idx) {
        int rc = upload_set(ctx, ctx->src, nsrc, src_idx, 1.0 / std::pow(ctx->cfg.h, ctx->gd.ndim));
        if (rc) return rc;
        return upload_set(ctx, ctx->rec, nrec, rec_idx, 1.0);
    }

    // Steps n = n0, n0 + dn, ... (count steps) of the shared time loop (oracle:
    // Propagator._propagate): inject `amp` rows at point set `inj`, sample the new field at point
    // set `out` (nullptr = none) into `series`; q_out(n) / q_in(n) give the per-step imaging-term
    // pointers (nullptr = off).  Injection and sampling are fused into the step launch: one launch
    // per time step; the sampling of step n rides on the next launch, which reads that field anyway.
    template <class QOut, class QIn>
    static int run_steps(fwi_ctx *ctx, Sweep &sw, int n0, int dn, int count, const fwi_ctx::PointSet &inj,
                         const T *amp, const fwi_ctx::PointSet *out, T *series, T out_scale, QOut q_out,
                         QIn q_in) {
        const GridDesc &g = ctx->gd;
        for (int it = 0, n = n0; it < count; ++it, n += dn) {
            StepArgs<T> a = base_args(ctx, 0);
            a.u_cur = (const T *)sw.f[sw.cur];
            a.u_prev = (T *)sw.f[sw.cur ^ 1];
            a.v = (T *)sw.v;
            a.q_out = q_out(n);
            q_in(n, a.q_in, a.q_in2);
            if (inj.n > 0) {
                a.inj_start = (const int *)inj.s_start.p;
                a.inj_pidx = (const int64_t *)inj.s_pidx;
                a.inj_cidx = (const int64_t *)inj.s_cidx;
                a.inj_cu = (const T *)inj.s_cu;
                a.inj_cq = (const T *)inj.s_cq;
                a.inj_col = (const int *)inj.s_col;
                a.inj_run = (const int *)inj.s_run;
                a.inj_amp = amp + (size_t)n * inj.n;
            }
            if (out && sw.prev_n >= 0 && out->n > 0) {
                a.rec_pidx = (const int64_t *)out->pidx;
                a.rec_out = series + (size_t)sw.prev_n * out->n;
                a.rec_scale = out_scale;
                a.nrec = out->n;
            }
            if (ctx->cpml) {  // memory variables of the border advance with the newest field ...
                const PmlArgs<T> p = pml_args(ctx, sw, a.q_out);
                int axes = 7;
                if (ctx->xpml) {  // ... the x border's inside the step kernel itself (step3d_stream, XP)
                    axes = 3;
                    a.xp_mode = dn < 0 ? 2 : 1;
                    a.xp_partial = ctx->cfg.npml % 4 != 0;
                    a.xp_psi = p.psi[2];
                    a.xp_zeta = p.zeta[2];
                    a.xp_a = p.a[2];
                    a.xp_b = p.b[2];
                    for (int k = 0; k < 5; ++k) {
                        a.xp_dk[k] = p.dk[k];
                        a.xp_dk1[k] = p.dk1[k];
                    }
                }
                // z / y borders: ONE line launch for both BEFORE the step (all three phases of the recursion; fwi_pml.hip,
                // pml_line_t) hands their term to the step kernel, which adds it inside q; the slab phases around the step
                // kernel take whatever is left (the x border of contexts whose lanes cannot carry it, grids without lines)
                const int lines = axes & ctx->pml_lines;
                axes &= ~lines;
                if (lines) {
                    HIPCHK(ctx, launch_pml_lines<T>(g, p, dn < 0, ctx->stream, lines));
                    a.pml_tz = p.tz;
                    a.pml_ty = p.ty;
                }
                if (axes) {
                    HIPCHK(ctx, launch_pml<T>(g, p, 1, dn < 0, ctx->stream, axes));
                    HIPCHK(ctx, launch_pml<T>(g, p, 2, dn < 0, ctx->stream, axes));
                }
                HIPCHK(ctx, launch_step<T>(ctx->kernel, g, a, ctx->tune, ctx->stream));
                if (axes) HIPCHK(ctx, launch_pml<T>(g, p, 3, dn < 0, ctx->stream, axes));  // their term joins u' (and q)
            } else if (sw.born_w) {  // (born_fused_supported: 3-D fp32 O(8) stream contexts without the CPML)
                if constexpr (std::is_same<T, float>::value) {
                    a.g = (T *)sw.born_w;  // read only
                    if (a.q_bf16)
                        HIPCHK(ctx, (launch_stream_born_bf16<4>(g, a, ctx->tune, ctx->stream)));
                    else
                        HIPCHK(ctx, (launch_stream_born<T, 4>(g, a, ctx->tune, ctx->stream)));
                } else {
                    return ctx->fail(FWI_ESTATE, "the fused Born path is fp32 only");
                }
            } else {
                HIPCHK(ctx, launch_step<T>(ctx->kernel, g, a, ctx->tune, ctx->stream));
            }
            sw.prev_n = n;
            sw.cur ^= 1;
        }
        return FWI_OK;
    }

    // PLACEMENT SEARCH (3-D CPML contexts past the cache-resident sizes; fwi_create).  The step kernel of such a context
    // streams seven arrays side by side, and how fast it runs depends on where they lie RELATIVE to each other: with every
    // device array of a 256^3 / npml 16 context carved from one slab, moving the 10 MiB `ty` alone by 4 MiB switched the
    // step kernel between 48.7 and 57.9 us (63.5 with everything on 64 MiB boundaries) -- same bytes by the FETCH / WRITE
    // counters, the line launch unmoved -- and with one hipMalloc per array the draw differs per process and per box
    // (72.9 ... 85.8 us per time step, profiles/r04_variance.log, r04_placement_probes.log).  No congruence rule we tried
    // predicts the slow positions, so the context MEASURES: the four small arrays (x border's psi / zeta, tz, ty) are
    // allocated with `place_pad` bytes of slack, and a coordinate search over their offsets (steps of 2 MiB) times a few
    // time steps of the real launch sequence on zeroed fields for each candidate and keeps a position only if it is
    // > 1 % faster twice.  ~30 candidates x ~1.5 ms: some tens of milliseconds per context, bit-identical results (the
    // arithmetic never sees an address).  FWI_PLACEMENT_TUNE=0 is the A/B hook.
    static int tune_placement(fwi_ctx *ctx) {
        const GridDesc &g = ctx->gd;
        const size_t fb = (size_t)g.ptot * sizeof(T), step = (size_t)2 << 20;
        const int ncand = (int)(ctx->place_pad / step) + 1;
        if (ncand < 2 || ctx->nmov == 0) return FWI_OK;
        // everything the trial steps read is zero, so everything they write is: the context is left as created
        for (void *f : {ctx->u[0], ctx->u[1], ctx->C, ctx->vf})
            if (f) HIPCHK(ctx, hipMemsetAsync(f, 0, fb, ctx->stream));
        for (int i = 0; i < ctx->nmov; ++i)  // (the movable arrays: the whole allocation, whichever position wins)
            HIPCHK(ctx, hipMemsetAsync(*ctx->mov_slot[i], 0, ctx->mov_bytes[i] + ctx->place_pad, ctx->stream));
        int rc = pml_zero(ctx);
        if (rc) return rc;
        hipEvent_t e0 = nullptr, e1 = nullptr;  // (every failure from here on leaves through `done`, which destroys them)
        const fwi_ctx::PointSet nobody;
        Sweep sw = main_sweep(ctx);
        int nstep = 0;
        auto timed = [&](int n, float *us) -> int {  // n time steps of the real launch sequence, no sources, no receivers
            sw.v = ctx->vf;  // (a movable array itself in increment form)
            HIPCHK(ctx, hipEventRecord(e0, ctx->stream));
            const int r = run_steps(ctx, sw, nstep, 1, n, nobody, (const T *)nullptr, nullptr, (T *)nullptr, T(0), none, noq);
            if (r) return r;
            nstep += n;
            HIPCHK(ctx, hipEventRecord(e1, ctx->stream));
            HIPCHK(ctx, hipEventSynchronize(e1));
            float ms = 0.f;
            HIPCHK(ctx, hipEventElapsedTime(&ms, e0, e1));
            *us = 1e3f * ms / n;
            return FWI_OK;
        };
        float best = 0.f, t = 0.f, t2 = 0.f;
        int n = 8;
        auto event = [&](hipEvent_t *e) -> int {
            HIPCHK(ctx, hipEventCreate(e));
            return FWI_OK;
        };
        if ((rc = event(&e0)) || (rc = event(&e1))) goto done;
        // warm up (code objects' first use, clocks), then the position the context was created with -- twice, the better
        if ((rc = timed(24, &t)) || (rc = timed(8, &t))) goto done;
        n = std::max(4, std::min(12, (int)(1500.f / std::max(t, 1.f))));  // ~1.5 ms per trial
        if (t > 2500.f) goto done;  // (a search would take seconds on such a grid, whose borders are a small share anyway)
        if ((rc = timed(n, &t)) || (rc = timed(n, &t2))) goto done;
        best = std::min(t, t2);
        ctx->place_us[0] = ctx->place_us[1] = best;
        for (int i = 0; i < ctx->nmov && !rc; ++i) {
            void **const slot = ctx->mov_slot[i];
            char *const base = (char *)*slot - ctx->mov_shift[i];
            size_t keep = ctx->mov_shift[i];
            for (int c = 0; c < ncand && !rc; ++c) {
                const size_t sh = (size_t)c * step;
                if (sh == keep) continue;
                *slot = base + sh;
                if ((rc = timed(n, &t)) || t >= 0.99f * best) continue;
                // a candidate that looks > 1 % faster: once more, then the incumbent again (the clock drifts over a
                // search), and only a candidate that beats both readings is kept
                if ((rc = timed(n, &t2))) continue;
                t = std::max(t, t2);
                *slot = base + keep;
                if ((rc = timed(n, &t2))) continue;
                if (t < 0.99f * t2) {
                    best = t;
                    keep = sh;
                } else {
                    best = t2;
                }
            }
            *slot = base + keep;  // (also on an error: the slot and its recorded shift always agree)
            ctx->mov_shift[i] = keep;
        }
        if (!rc) ctx->place_us[1] = best;
    done:
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        return rc;
    }

    // the last step's field has no following launch to ride on
    static int flush_record(fwi_ctx *ctx, Sweep &sw, const fwi_ctx::PointSet &out, T *series, T out_scale) {
        if (sw.prev_n < 0) return FWI_OK;
        HIPCHK(ctx, launch_record<T>((const T *)sw.f[sw.cur], (const int64_t *)out.pidx,
                                     series + (size_t)sw.prev_n * out.n, out_scale, out.n, ctx->stream));
        return FWI_OK;
    }

    static int zero_fields(fwi_ctx *ctx, void *a, void *b) {
        HIPCHK(ctx, hipMemsetAsync(a, 0, (size_t)ctx->gd.ptot * sizeof(T), ctx->stream));
        HIPCHK(ctx, hipMemsetAsync(b, 0, (size_t)ctx->gd.ptot * sizeof(T), ctx->stream));
        return FWI_OK;
    }

    // What the three sweeps (forward, adjoint, born) share on the host.  Everything here that queues a memset is called
    // before TimeLoop::begin(); save_segment / restore_segment queue device-to-device copies only and run inside the loop.

    static T *none(int) { return nullptr; }                                  // run_steps: no q_out ...
    static void noq(int, const T *&p, const T *&p2) { p = p2 = nullptr; }  // ... and no q_in

    static Sweep main_sweep(fwi_ctx *ctx) {
        Sweep sw;
        sw.f[0] = ctx->u[0];
        sw.f[1] = ctx->u[1];
        sw.v = ctx->vf;
        return sw;
    }

    // the sweep in u[] / vf from zeroed fields and memory variables
    static int start_sweep(fwi_ctx *ctx, Sweep &sw) {
        int rc = zero_fields(ctx, ctx->u[0], ctx->u[1]);
        if (rc) return rc;
        sw = main_sweep(ctx);
        if (ctx->inc) HIPCHK(ctx, hipMemsetAsync(ctx->vf, 0, (size_t)ctx->gd.ptot * sizeof(T), ctx->stream));
        return ctx->cpml ? pml_zero(ctx) : FWI_OK;
    }

    // the checkpointed forward recomputation: its own fields and its own set of memory variables
    static Sweep recompute_sweep(fwi_ctx *ctx) {
        Sweep fw;
        fw.f[0] = ctx->fwd[0];
        fw.f[1] = ctx->fwd[1];
        fw.v = ctx->fwv;
        fw.pml_fw = true;
        return fw;
    }

    // snapshot `seg` of a checkpointed forward: two padded fields, (u^n0, u^{n0-1}) or, increment form, (u^n0, v^n0)
    static T *snapshot(fwi_ctx *ctx, int seg) {
        const GridDesc &g = ctx->gd;
        return (T *)ctx->snap + (size_t)seg * 2 * g.ptot;
    }

    static int save_segment(fwi_ctx *ctx, const Sweep &sw, int seg) {
        const size_t n = (size_t)ctx->gd.ptot;
        T *sn = snapshot(ctx, seg);
        HIPCHK(ctx, hipMemcpyAsync(sn, sw.f[sw.cur], n * sizeof(T), hipMemcpyDeviceToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(sn + n, ctx->inc ? sw.v : sw.f[sw.cur ^ 1], n * sizeof(T), hipMemcpyDeviceToDevice,
                                   ctx->stream));
        return ctx->cpml ? pml_snapshot(ctx, seg, false, false) : FWI_OK;
    }

    // ... and back into the recomputation sweep, which starts over from it
    static int restore_segment(fwi_ctx *ctx, Sweep &fw, int seg) {
        const size_t n = (size_t)ctx->gd.ptot;
        const T *sn = snapshot(ctx, seg);
        fw.cur = 0;
        fw.prev_n = -1;
        HIPCHK(ctx, hipMemcpyAsync(fw.f[0], sn, n * sizeof(T), hipMemcpyDeviceToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(ctx->inc ? fw.v : fw.f[1], sn + n, n * sizeof(T), hipMemcpyDeviceToDevice, ctx->stream));
        return ctx->cpml ? pml_snapshot(ctx, seg, true, true) : FWI_OK;
    }

    // The fused and the two-step launches swap the buffers of a sweep with its spare pair: the context owns whichever
    // the sweep ended with (a no-op after a sweep that swapped nothing).  After the loops, never on an error return.
    static void adopt(fwi_ctx *ctx, const Sweep &sw, void *const *spare) {
        ctx->u[0] = sw.f[0];
        ctx->u[1] = sw.f[1];
        ctx->fx[0] = spare[0];
        ctx->fx[1] = spare[1];
        ctx->vf = sw.v;
    }

    static void adopt_recompute(fwi_ctx *ctx, const Sweep &fw, void *const *fspare) {
        ctx->fwd[0] = fw.f[0];
        ctx->fwd[1] = fw.f[1];
        ctx->fwx[0] = fspare[0];
        ctx->fwx[1] = fspare[1];
        ctx->fwv = fw.v;
    }

    // Where the forward term q^n of step n lives, by the kind of store the context holds
    struct Store {
        char *q;        // q_store
        T *ring;        // Fourier store: the B + 1 ring slots
        size_t slot_bytes;  // of the native store, which may hold bf16
        int64_t npts;
        int S, K, R;
        explicit Store(const fwi_ctx *ctx)
            : q((char *)ctx->q_store), ring((T *)ctx->four_ring), slot_bytes((size_t)ctx->gd.npts * ctx->qes),
              npts(ctx->gd.npts), S(ctx->istride), K(ctx->ckpt), R(ctx->four_batch + 1) {}
        // native store: q^n is kept for n % S == 0, in slot n / S
        void *slot(int n) const { return q + (size_t)(n / S) * slot_bytes; }
        size_t bytes(int nt) const { return ((size_t)nt + S - 1) / S * slot_bytes; }
        // checkpointed: K slots for the steps of the segment that begins at n0 (n may lie below n0: run_fused's q_base
        // is the slot of step 0), then the carry
        T *seg_slot(int n, int n0) const { return (T *)q + (int64_t)(n - n0) * npts; }
        T *carry() const { return (T *)q + (int64_t)K * npts; }
        // Fourier store: sample j = n / S in ring slot j % (B + 1)
        T *ring_slot(int n) const { return ring + (int64_t)((n / S) % R) * npts; }
    };

    // Fourier store: the accumulators, the ring and the device table, all or nothing, by the first forward(save)
    static int fourier_alloc(fwi_ctx *ctx) {
        if (ctx->four_acc) return FWI_OK;
        const size_t F = ctx->four_freqs.size(), vol = (size_t)ctx->gd.npts * sizeof(T);
        const int rows = (ctx->cfg.nt_max + ctx->istride - 1) / ctx->istride + FOURIER_BMAX - 1;
        const size_t acc = 2 * F * vol, ring = (size_t)(ctx->four_batch + 1) * vol;
        size_t total, fr;
        // (zeroed: the pad columns of a ring slot are the step kernels' to write or to leave)
        if (int rc = alloc_all(ctx, {{&ctx->four_acc, "four_acc", acc, true}, {&ctx->four_ring, "four_ring", ring, true},
                                     {&ctx->four_tw, "four_tw", F * rows * 2 * sizeof(double), true}}, &total, &fr))
            return rc != FWI_ENOMEM ? rc : ctx->fail(FWI_ENOMEM,
                             "Fourier forward-term store needs %.1f GiB (%d frequencies, batch %d) but only %.1f GiB are "
                             "free; fewer frequencies or a smaller batch need less",
                             total / 1073741824.0, (int)F, ctx->four_batch, fr / 1073741824.0);
        ctx->four_rows = rows;
        ctx->store_held = acc + ring;
        return FWI_OK;
    }

    // The table of one sweep over N = ceil(nt / S) samples, formed in fp64 and uploaded before the time loop begins (a
    // captured loop then holds launches only): block k, row j = (cos theta_kj, sin theta_kj), theta_kj = 2 pi f_k j S dt
    // with f_k j S dt reduced to its fractional part first; `synthesis`: both times w_k = 1 / N at f_k = 0 and at the
    // Nyquist frequency 1 / (2 S dt) of the sampled axis, else 2 / N, times the caller's a_k = fw[k] (nullptr: ones; the
    // Fourier Born sweeps).  The rows from N on stay zero.
    static int fourier_table(fwi_ctx *ctx, int nt, bool synthesis, const double *fw = nullptr) {
        const int S = ctx->istride, N = (nt + S - 1) / S, rows = ctx->four_rows, F = (int)ctx->four_freqs.size();
        const double sdt = (double)S * ctx->cfg.dt;
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // the upload of the sweep before may still read the host copy
        std::vector<double> &t = ctx->four_tw_host;
        t.assign((size_t)F * rows * 2, 0.0);
        for (int k = 0; k < F; ++k) {
            const double f = ctx->four_freqs[k];
            const bool edge = f == 0.0 || std::fabs(2.0 * f * sdt - 1.0) <= FOURIER_NYQUIST_RTOL;
            const double w = (synthesis ? (edge ? 1.0 : 2.0) / N : 1.0) * (fw ? fw[k] : 1.0);
            for (int j = 0; j < N; ++j) {
                const double x = f * sdt * j, th = 2.0 * M_PI * (x - std::floor(x));
                t[((size_t)k * rows + j) * 2] = w * std::cos(th);
                t[((size_t)k * rows + j) * 2 + 1] = w * std::sin(th);
            }
        }
        HIPCHK(ctx, hipMemcpyAsync(ctx->four_tw, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        return FWI_OK;
    }

    static int forward(fwi_ctx *ctx, int32_t nt, int32_t nsrc, const int32_t *src_idx,
                       const T *wavelet, int32_t nrec, const int32_t *rec_idx, int32_t save,
                       T *seis_out) {
        const GridDesc &g = ctx->gd;
        const int K = ctx->ckpt;  // 0 = store every step's imaging term, K > 0 = snapshot every K steps
        const bool four = save && !ctx->four_freqs.empty();  // ... or their Fourier coefficients (K = 0 then)
        ctx->four_sweep = four;
        int rc;
        if ((rc = upload_points(ctx, nsrc, src_idx, nrec, rec_idx))) return rc;
        if (four && (rc = fourier_alloc(ctx))) return rc;
        size_t total, fr;
        if (save && K == 0 && !four && !ctx->q_store) {
            if ((rc = alloc_all(ctx, {{&ctx->q_store, "q_store", Store(ctx).bytes(ctx->cfg.nt_max), false}}, &total, &fr)))
                return rc != FWI_ENOMEM ? rc : ctx->fail(FWI_ENOMEM,
                                 "forward-term store needs %.1f GiB (nt_max=%d) but only %.1f GiB are free; "
                                 "set ckpt_interval (recomputation) or image_stride (decimated imaging)",
                                 total / 1073741824.0, ctx->cfg.nt_max, fr / 1073741824.0);
            ctx->store_held = total;
        }
        if (save && K > 0 && !ctx->ckpt_ready) {
            // snapshots of (u^n, u^{n-1}) per segment, K + 1 imaging-term slots, the recomputation's field
            // pair(s).  All or nothing: a partial set would let a later adjoint run on null buffers.
            const int nseg = (ctx->cfg.nt_max + K - 1) / K;
            const size_t fb = (size_t)g.ptot * sizeof(T);
            const size_t *pb = ctx->pml_bytes;
            ctx->pml_snap_stride = 2 * (pb[0] + pb[1] + pb[2]);
            if ((rc = alloc_all(ctx, {
                     {&ctx->snap, "snap", (size_t)nseg * 2 * fb, false},
                     {&ctx->q_store, "q_store", (size_t)(K + 1) * g.npts * sizeof(T), false},  // K slots + carry
                     // (padded fields are zeroed at allocation: in increment form fwd[1] only ever receives interior points and
                     // its halo must read 0 -- found by the option fuzz reusing device memory of earlier contexts; the others
                     // are overwritten whole before use, but fwi_check_padding looks at every padded field of the context)
                     {&ctx->fwd[0], "fwd", fb, true},
                     {&ctx->fwd[1], "fwd", fb, true, 1}, {&ctx->fwv, "fwv", ctx->inc ? fb : 0, true},
                     {&ctx->fwx[0], "fwx", ctx->fused2d ? fb : 0, true}, {&ctx->fwx[1], "fwx", ctx->fused2d ? fb : 0, true, 1},
                     {&ctx->pml_psi_fw[0], "pml_psi_fw", pb[0], false}, {&ctx->pml_zeta_fw[0], "pml_zeta_fw", pb[0], false},
                     {&ctx->pml_psi_fw[1], "pml_psi_fw", pb[1], false, 1}, {&ctx->pml_zeta_fw[1], "pml_zeta_fw", pb[1], false, 1},
                     {&ctx->pml_psi_fw[2], "pml_psi_fw", pb[2], false, 2}, {&ctx->pml_zeta_fw[2], "pml_zeta_fw", pb[2], false, 2},
                     {&ctx->pml_snap, "pml_snap", (size_t)nseg * ctx->pml_snap_stride, false}}, &total, &fr)))
                return rc != FWI_ENOMEM ? rc : ctx->fail(FWI_ENOMEM,
                                 "checkpoint buffers need %.1f GiB (nt_max=%d, ckpt_interval=%d) but only %.1f GiB "
                                 "are free; a ckpt_interval near sqrt(2 nt_max) needs the least memory",
                                 total / 1073741824.0, ctx->cfg.nt_max, K, fr / 1073741824.0);
            ctx->ckpt_ready = true;
            ctx->store_held = total;
        }
        // the pinned staging buffer at its final size for this shot, before any copy is queued on it
        if ((rc = stage_reserve(ctx, (size_t)nt * std::max(std::max(nsrc, nrec), 1) * sizeof(T)))) return rc;
        if ((rc = ensure(ctx, ctx->wav, (size_t)nt * std::max(nsrc, 1) * sizeof(T)))) return rc;
        if ((rc = ensure(ctx, ctx->amp, (size_t)nt * std::max(nrec, 1) * sizeof(T)))) return rc;
        if ((rc = ensure(ctx, ctx->series, (size_t)nt * std::max(std::max(nsrc, nrec), 1) * sizeof(T)))) return rc;
        ctx->nt = nt;
        ctx->nsrc = nsrc;
        ctx->nrec = nrec;
        hipStream_t s = ctx->stream;  // (no shot to speak of from here to the end: drop_forward, the callers' first statement)
        if (nsrc && (rc = upload_amplitudes(ctx, ctx->wav.p, wavelet, nt, nsrc, ctx->src_sp))) return rc;
        Sweep sw;
        if ((rc = start_sweep(ctx, sw))) return rc;
        const Store st(ctx);
        T *q_store = (T *)ctx->q_store;
        T *series = (T *)ctx->series.p;
        const bool fused = use_fused(ctx, nt);  // 2-D: FUSED2D_STEPS time steps per launch
        // a step count that is not a multiple of FUSED2D_STEPS: the bulk fused, the last 1-3 steps one per launch
        const int nfused = mixed_fused_steps(ctx, nt);
        void *spare[2] = {ctx->fx[0], ctx->fx[1]};
        // 3-D: a forward sweep that keeps nothing for imaging runs two time steps per pass (the last step of an
        // odd count goes through the single-step kernel)
        const int npair = (ctx->pair3d && !save && base_args(ctx, 0).damp == 0) ? (nt & ~1) : 0;
        if ((fused || nfused || npair) && (rc = zero_fields(ctx, spare[0], spare[1]))) return rc;
        if (four) {
            if ((rc = fourier_table(ctx, nt, false))) return rc;
            HIPCHK(ctx, hipMemsetAsync(ctx->four_acc, 0, 2 * ctx->four_freqs.size() * (size_t)g.npts * sizeof(T), s));
        }
        TimeLoop loop(ctx);
        if ((rc = loop.begin())) return rc;
        if (npair) {
            if ((rc = run_pairs(ctx, sw, spare, 0, npair, ctx->src, (const T *)ctx->wav.p, &ctx->rec, series, T(1))))
                return rc;
            if ((rc = run_steps(ctx, sw, npair, 1, nt - npair, ctx->src, (const T *)ctx->wav.p, &ctx->rec, series, T(1),
                                none, noq)))
                return rc;
        } else if (save && K > 0) {
            for (int n0 = 0, seg = 0; n0 < nt; n0 += K, ++seg) {
                if ((rc = save_segment(ctx, sw, seg))) return rc;
                const int cnt = std::min(K, nt - n0);
                if (fused)
                    rc = run_fused(ctx, sw, spare, n0, 1, cnt, ctx->src, (const T *)ctx->wav.p, &ctx->rec, series,
                                   T(1), 0, nullptr);
                else
                    rc = run_steps(ctx, sw, n0, 1, cnt, ctx->src, (const T *)ctx->wav.p, &ctx->rec, series, T(1),
                                   none, noq);
                if (rc) return rc;
            }
        } else if (four) {
            // one step per launch; q^{jS} goes to ring slot j % (B + 1), and every B samples (and behind the last, partial
            // batch) the analysis adds the batch to the accumulators
            const int ks = ctx->istride, B = ctx->four_batch, R = B + 1, N = (nt + ks - 1) / ks;
            auto qo = [&](int n) -> T * { return n % ks == 0 ? st.ring_slot(n) : nullptr; };
            for (int j0 = 0; j0 < N; j0 += B) {
                const int nb = std::min(B, N - j0), n0 = j0 * ks, n1 = std::min((int)nt, (j0 + nb) * ks);
                if ((rc = run_steps(ctx, sw, n0, 1, n1 - n0, ctx->src, (const T *)ctx->wav.p, &ctx->rec, series, T(1), qo,
                                    noq)))
                    return rc;
                HIPCHK(ctx, launch_fourier_analyse<T>((T *)ctx->four_acc, st.ring, g.npts, R, j0 % R, j0, nb,
                                                      (const double *)ctx->four_tw, ctx->four_rows,
                                                      (int)ctx->four_freqs.size(), s));
            }
        } else if (fused) {
            if ((rc = run_fused(ctx, sw, spare, 0, 1, nt, ctx->src, (const T *)ctx->wav.p, &ctx->rec, series, T(1),
                                save ? 1 : 0, q_store)))
                return rc;
        } else {
            const int ks = ctx->istride;  // q^n is kept for n % ks == 0, in slot n / ks
            auto qo = [&](int n) -> T * { return (save && n % ks == 0) ? (T *)st.slot(n) : nullptr; };
            if (nfused && (rc = run_fused(ctx, sw, spare, 0, 1, nfused, ctx->src, (const T *)ctx->wav.p, &ctx->rec, series,
                                          T(1), save ? 1 : 0, q_store)))
                return rc;
            if ((rc = run_steps(ctx, sw, nfused, 1, nt - nfused, ctx->src, (const T *)ctx->wav.p, &ctx->rec, series, T(1),
                                qo, noq)))
                return rc;
        }
        if ((rc = flush_record(ctx, sw, ctx->rec, series, T(1)))) return rc;
        if ((rc = loop.end())) return rc;
        adopt(ctx, sw, spare);
        if ((rc = download_samples(ctx, (nrec && seis_out) ? seis_out : nullptr, ctx->series.p, nt, nrec, ctx->rec_sp,
                                   &ctx->pts_d)))
            return rc;
        ctx->have_forward = true;
        ctx->have_syn = true;
        ctx->have_q = save != 0;
        return FWI_OK;
    }

    // Spectral imaging: the 2 F accumulators of the adjoint field, all or nothing, by the first fwi_adjoint_spectral
    static int fourier_adjoint_alloc(fwi_ctx *ctx) {
        if (ctx->four_adj) return FWI_OK;
        const size_t F = ctx->four_freqs.size(), bytes = 2 * F * (size_t)ctx->gd.npts * sizeof(T);
        size_t total, fr;
        if (int rc = alloc_all(ctx, {{&ctx->four_adj, "four_adj", bytes, true}}, &total, &fr))
            return rc != FWI_ENOMEM ? rc : ctx->fail(FWI_ENOMEM,
                             "fwi_adjoint_spectral: the adjoint accumulators need %.1f GiB (%d frequencies) but only "
                             "%.1f GiB are free; fewer frequencies need less",
                             total / 1073741824.0, (int)F, fr / 1073741824.0);
        ctx->store_held += bytes;
        return FWI_OK;
    }

    // `spectral` (fwi_adjoint_spectral; image = 0 then): the sweep of image = 0 one step per launch, with the Fourier
    // analysis of the adjoint field at the imaging samples riding behind it.  g_acc is not touched.
    static int adjoint(fwi_ctx *ctx, const T *residual, int32_t image, T *adj_src_out, bool spectral = false) {
        const GridDesc &g = ctx->gd;
        const int nt = ctx->nt, K = ctx->ckpt;
        hipStream_t s = ctx->stream;
        int rc;
        if (ctx->nrec && residual && (rc = upload_amplitudes(ctx, ctx->amp.p, residual, nt, ctx->nrec, ctx->rec_sp)))
            return rc;  // (residual == nullptr: the one fwi_misfit_l2 left in ctx->amp)
        ctx->have_dev_residual = false;  // consumed: ctx->series is about to be overwritten
        ctx->have_syn = false;           // ... by this sweep's source-side series (fwi_misfit_l2 must not read them)
        const bool four = image && !ctx->four_freqs.empty();  // imaging against the Fourier store: one step per launch
        ctx->four_sweep = four || spectral;
        if (spectral && (rc = fourier_adjoint_alloc(ctx))) return rc;
        const T rs = (T)(1.0 / std::pow(ctx->cfg.h, g.ndim));
        Sweep sw;
        if ((rc = start_sweep(ctx, sw))) return rc;
        const Store st(ctx);
        T *q_store = (T *)ctx->q_store;
        T *series = (T *)ctx->series.p;
        const T *amp = (const T *)ctx->amp.p;
        const bool fused = use_fused(ctx, nt);
        const int nfused = mixed_fused_steps(ctx, nt);
        void *spare[2] = {ctx->fx[0], ctx->fx[1]};
        // checkpointed: the forward recomputation, which ping-pongs between its own two buffer pairs (fwd, fwx) when fused
        Sweep fw = recompute_sweep(ctx);
        void *fspare[2] = {ctx->fwx[0], ctx->fwx[1]};
        if ((fused || nfused) && (rc = zero_fields(ctx, spare[0], spare[1]))) return rc;
        if (four && (rc = fourier_table(ctx, nt, true))) return rc;
        if (spectral) {
            ctx->have_m = false;
            if ((rc = fourier_table(ctx, nt, false))) return rc;
            HIPCHK(ctx, hipMemsetAsync(ctx->four_adj, 0, 2 * ctx->four_freqs.size() * (size_t)g.npts * sizeof(T), s));
        }
        TimeLoop loop(ctx);
        if ((rc = loop.begin())) return rc;
        const T *q0 = nullptr;  // q^0, for the last pairing (mu^1 with q^0)
        // Lagged imaging: adjoint step n (which reads mu^{n+2} as u_cur and mu^{n+3} as u_prev) owns
        // the pairing P(n) = (mu^{n+2}, q^{n+1}).  Steps are taken in pairs: P(n+1) is deferred and
        // taken at step n together with P(n) -- u_prev there is still mu^{n+3} -- so the gradient
        // accumulator is read and written every other step only.  plan() fills, for the steps
        // n = hi .. lo (descending) of one run, the q pointers of P(n) and of a deferred P(n+1).
        std::vector<const T *> pq, pq2;
        auto plan = [&](int hi, int lo, auto qptr /* n -> q^{n+1} or nullptr */) {
            pq.assign(hi - lo + 1, nullptr);
            pq2.assign(hi - lo + 1, nullptr);
            const T *pending = nullptr;  // deferred pairing of the step above
            for (int n = hi; n >= lo; --n) {
                const T *mine = qptr(n);
                if (pending) {  // second step of a pair: take both (mine is valid whenever pending is)
                    pq[hi - n] = mine;
                    pq2[hi - n] = pending;
                    pending = nullptr;
                } else if (mine && n > lo && ctx->istride == 1) {  // (increment form too since round 4: u_prev = u - v)
                    pending = mine;  // first step of a pair: defer (every step images: the next one pairs)
                } else {
                    pq[hi - n] = mine;  // single (last step of an odd run, or nothing to pair)
                }
            }
        };
        bool imaged_all = false;  // the fused kernel pairs mu^{n+1} with q^n inside the launch (no lag)
        if (image && K > 0) {
            // Checkpointed: per segment (last to first) restore the snapshot, recompute the forward steps storing q into the
            // K-slot buffer, then take the adjoint steps of that segment against those slots.  Fused, nothing lags.  One
            // step per launch, q^{n+1} at a segment's first adjoint step is the first q of the segment processed before,
            // kept in the carry slot.
            for (int seg = (nt + K - 1) / K - 1; seg >= 0; --seg) {
                const int n0 = seg * K, cnt = std::min(K, nt - n0), hi = n0 + cnt - 1;
                if ((rc = restore_segment(ctx, fw, seg))) return rc;
                auto qo = [&](int n) -> T * { return st.seg_slot(n, n0); };
                rc = fused ? run_fused(ctx, fw, fspare, n0, 1, cnt, ctx->src, (const T *)ctx->wav.p, nullptr, nullptr, T(0), 1,
                                       st.seg_slot(0, n0))
                           : run_steps(ctx, fw, n0, 1, cnt, ctx->src, (const T *)ctx->wav.p, nullptr, nullptr, T(0), qo, noq);
                if (rc) return rc;
                if ((rc = illum_accumulate(ctx, q_store, cnt))) return rc;  // slots 0 .. cnt - 1, before they are reused
                if (fused) {
                    if ((rc = run_fused(ctx, sw, spare, hi, -1, cnt, ctx->rec, amp, &ctx->src, series, rs, 2,
                                        st.seg_slot(0, n0))))
                        return rc;
                    continue;
                }
                plan(hi, n0, [&](int n) -> const T * {
                    if (n + 1 >= nt) return nullptr;
                    return (n + 1 < n0 + cnt) ? st.seg_slot(n + 1, n0) : st.carry();
                });
                auto qi = [&](int n, const T *&p, const T *&p2) { p = pq[hi - n]; p2 = pq2[hi - n]; };
                if ((rc = run_steps(ctx, sw, hi, -1, cnt, ctx->rec, amp, &ctx->src, series, rs, none, qi)))
                    return rc;
                HIPCHK(ctx, hipMemcpyAsync(st.carry(), q_store, (size_t)g.npts * sizeof(T), hipMemcpyDeviceToDevice, s));
            }
            imaged_all = fused;
            q0 = st.carry();  // (one step per launch: the last pairing is still owed)
        } else if (fused) {
            if ((rc = run_fused(ctx, sw, spare, nt - 1, -1, nt, ctx->rec, amp, &ctx->src, series, rs, image ? 2 : 0,
                                q_store)))
                return rc;
            imaged_all = true;
        } else if (four) {
            // Fourier store: batch by batch (last to first) the synthesis rebuilds the band-limited q~ of the batch's samples
            // in their ring slots, then the adjoint steps n = (j0 + nb) S - 1 .. j0 S of the batch run with the lagged
            // pairing.  The first of them pairs with the lowest sample of the batch above: with B + 1 slots that one is
            // still there (a batch fills B consecutive slots), so nothing is carried.  plan() starts afresh per batch: a
            // pairing deferred across the boundary would need the second-lowest sample of the batch above, whose slot
            // this batch's synthesis has just taken.
            const int ks = ctx->istride, B = ctx->four_batch, R = B + 1, N = (nt + ks - 1) / ks;
            for (int j0 = ((N - 1) / B) * B; j0 >= 0; j0 -= B) {
                const int nb = std::min(B, N - j0), lo = j0 * ks, hi = std::min(nt, (j0 + nb) * ks) - 1;
                HIPCHK(ctx, launch_fourier_synthesise<T>(st.ring, (const T *)ctx->four_acc, g.npts, R, j0 % R, j0, nb,
                                                         (const double *)ctx->four_tw, ctx->four_rows,
                                                         (int)ctx->four_freqs.size(), s));
                plan(hi, lo, [&](int n) -> const T * {
                    return (n + 1 < nt && (n + 1) % ks == 0) ? st.ring_slot(n + 1) : nullptr;
                });
                auto qi = [&](int n, const T *&p, const T *&p2) { p = pq[hi - n]; p2 = pq2[hi - n]; };
                if ((rc = run_steps(ctx, sw, hi, -1, hi - lo + 1, ctx->rec, amp, &ctx->src, series, rs, none, qi)))
                    return rc;
            }
            q0 = st.ring_slot(0);  // sample 0: slot 0, written by the synthesis of the lowest batch
        } else if (spectral) {
            // Spectral imaging: batch by batch (last to first) the adjoint steps n = (j0 + nb) S - 1 .. j0 S run without
            // imaging; behind every sampled step n = j S the field it has just written, mu^{jS+1} (what the imaging
            // condition pairs with q^{jS}), is packed into ring slot j % (B + 1), which the forward sweep no longer needs,
            // and behind the lowest sample of the batch the analysis adds the batch to the adjoint accumulators
            const int ks = ctx->istride, B = ctx->four_batch, R = B + 1, N = (nt + ks - 1) / ks;
            for (int j0 = ((N - 1) / B) * B; j0 >= 0; j0 -= B) {
                const int nb = std::min(B, N - j0);
                for (int j = j0 + nb - 1; j >= j0; --j) {
                    const int hi = std::min(nt, (j + 1) * ks) - 1, lo = j * ks;
                    if ((rc = run_steps(ctx, sw, hi, -1, hi - lo + 1, ctx->rec, amp, &ctx->src, series, rs, none, noq)))
                        return rc;
                    HIPCHK(ctx, launch_fimage_pack<T>(g, (const T *)sw.f[sw.cur], st.ring_slot(lo), s));
                }
                HIPCHK(ctx, launch_fourier_analyse<T>((T *)ctx->four_adj, st.ring, g.npts, R, j0 % R, j0, nb,
                                                      (const double *)ctx->four_tw, ctx->four_rows,
                                                      (int)ctx->four_freqs.size(), s));
            }
        } else {
            // steps nt-1 .. nfused one per launch (all of them when nfused == 0), lagged pairing; the pairing owed
            // at the lower end, (mu^{nfused+1}, q^{nfused}), is the "last pairing" of that run
            const int ks = ctx->istride;
            plan(nt - 1, nfused, [&](int n) -> const T * {
                return (image && n + 1 < nt && (n + 1) % ks == 0) ? (const T *)st.slot(n + 1) : nullptr;
            });
            auto qi = [&](int n, const T *&p, const T *&p2) { p = pq[nt - 1 - n]; p2 = pq2[nt - 1 - n]; };
            if ((rc = run_steps(ctx, sw, nt - 1, -1, nt - nfused, ctx->rec, amp, &ctx->src, series, rs, none, qi)))
                return rc;
            q0 = (nfused % ks == 0) ? (const T *)st.slot(nfused) : nullptr;
            if (nfused) {
                // ... then the first nfused steps, FUSED2D_STEPS per launch (pairing inside the launch, no lag)
                if ((rc = flush_record(ctx, sw, ctx->src, series, rs))) return rc;
                sw.prev_n = -1;
                if (image && q0)
                    HIPCHK(ctx, launch_image<T>(g, (const T *)sw.f[sw.cur], q0, (T *)ctx->g_acc, ctx->qbf16, s));
                if ((rc = run_fused(ctx, sw, spare, nfused - 1, -1, nfused, ctx->rec, amp, &ctx->src, series, rs,
                                    image ? 2 : 0, q_store)))
                    return rc;
                imaged_all = true;
            }
        }
        adopt(ctx, sw, spare);
        adopt_recompute(ctx, fw, fspare);
        if ((rc = flush_record(ctx, sw, ctx->src, series, rs))) return rc;
        if (image && !imaged_all)  // the last pairing: mu^1 with q^0
            HIPCHK(ctx, launch_image<T>(g, (const T *)sw.f[sw.cur], q0, (T *)ctx->g_acc, ctx->qbf16, s));
        if (image && ctx->qbf16 && ctx->nsrc > 0)
            // the store holds C L u rounded to bf16; the source's own share C w / h^D of the forward term is paired
            // exactly, in closed form: g(x_s) += cq_s sum_n mu^{n+1}(x_s) w_s^n, with mu at the sources = the series
            // this sweep has just recorded (scaled by rs)
            // (per node, in the sorted order of the source set: two sources on one node add in a fixed order)
            HIPCHK(ctx, launch_source_image<T>((const T *)ctx->series.p, (const T *)ctx->wav.p, (const int64_t *)ctx->src.s_cidx,
                                               (const T *)ctx->src.s_cq, (const int *)ctx->src.s_col,
                                               (const int *)ctx->src.s_run, (T *)ctx->g_acc, nt, ctx->nsrc, ctx->istride,
                                               (T)(1.0 / (double)rs), s));
        if (image && K == 0) {  // the whole store: the ceil(nt / S) slots of this shot, once
            if ((rc = illum_accumulate(ctx, q_store, (nt + ctx->istride - 1) / ctx->istride))) return rc;
            if (ctx->h_acc && ctx->qbf16 && ctx->nsrc > 0)  // the source's exact share at its nodes (closed form)
                HIPCHK(ctx, launch_illum_source_bf16((float *)ctx->h_acc, ctx->q_store, g.npts, (const float *)ctx->wav.p,
                                                     (const int64_t *)ctx->src.cidx, (const float *)ctx->src.cq, nt,
                                                     ctx->nsrc, ctx->istride, s));
        }
        if ((rc = loop.end())) return rc;
        if ((rc = download_samples(ctx, (adj_src_out && ctx->nsrc) ? adj_src_out : nullptr, ctx->series.p, nt, ctx->nsrc,
                                   ctx->src_sp, nullptr)))
            return rc;
        ctx->have_m = spectral || ctx->have_m;
        return FWI_OK;
    }

    // Born modelling dd = J dm (include/fwi.h, fwi_born / fwi_born_imaging).  dm comes from the host (`dm_host`) or from a
    // compact device vector (`dm_dev`).  The Born field du obeys the wavefield's recursion with the distributed source
    // w q^n, w = dC / C, in the place of the point source: the sweep runs the ordinary one-step launches of run_steps on
    // zeroed fields (no injection, nothing stored) and adds A w q^n to du^{n+1} after step n (fwi_born.hip); the receiver
    // sampling that rides on the next step launch then sees the completed field.  `fused` (born_fused_supported
    // contexts): the step kernel itself adds w q^n inside q (fwi_born3d.hip) and there is no second pass.  The store and
    // the snapshots are read, never written.
    //
    // The imaging operator J_img (the transpose of what adjoint(image) + gradient compute on THIS context's store) is the
    // same sweep on whatever the store holds:
    //  - image_stride S > 1: the scattering source acts on the stored steps n % S == 0 only, from slot n / S, with the
    //    quadrature weight S folded into w; the steps in between are plain launches, batched into one run_steps call.
    //  - bf16 store: the slot holds bf16(C L u^n); the source's exact share w(x_s) C src^n(x_s) joins du^{n+1} through the
    //    step launch's fused injection at the source nodes (amplitudes ctx->born_src; entries of one node summed first).
    //  - ckpt_interval K > 0: segment by segment in ascending order, the forward state is restored from its snapshot and
    //    the segment's q^n are recomputed into the slot buffer by the recomputation fields of the adjoint (fwd, fwv, fwx,
    //    the forward set of memory variables); the Born field then sweeps those slots in u[], vf and the main set.
    //  - Fourier store (`spec`: fwi_fourier_born*, the 2 F coefficient volumes the source is synthesised from, Q_k or the
    //    extended spectrum P_k of fwi_fbornx.h; `a`: the a_k folded into the synthesis table): batch by batch in
    //    ascending order the synthesis rebuilds the batch's samples in their ring slots, which the stored steps then read
    //    as they read a native slot.  Neither dm_host nor dm_dev (the extended sweep): dm = 1, w = -c^2 S.
    static int born(fwi_ctx *ctx, int32_t wrt, const T *dm_host, const void *dm_dev, bool fused, T *seis_out,
                    const T *spec = nullptr, const double *a = nullptr) {
        const GridDesc &g = ctx->gd;
        const int nt = ctx->nt, nrec = ctx->nrec, S = ctx->istride, K = ctx->ckpt;
        hipStream_t s = ctx->stream;
        int rc;
        if ((rc = dev_first_use(ctx, &ctx->born_w, (size_t)g.npts * sizeof(T), "born_w"))) return rc;
        if (dm_host && (rc = upload_compact<T>(ctx, ctx->born_w, dm_host))) return rc;
        if (!dm_host && !dm_dev) {  // ones, pad columns zero: 1 / (0 + 1)
            HIPCHK(ctx, hipMemsetAsync(ctx->born_w, 0, (size_t)g.npts * sizeof(T), s));
            HIPCHK(ctx, launch_vec_recip<T>(g, (T *)ctx->born_w, 1.0, 1.0, s));
        }
        if (S > 1)
            HIPCHK(ctx, launch_born_weight_strided<T>(g, (const T *)(dm_dev ? dm_dev : ctx->born_w), (const T *)ctx->c_dev,
                                                      (T *)ctx->born_w, wrt == FWI_WRT_VELOCITY, S, s));
        else
            HIPCHK(ctx, launch_born_weight<T>(g, (const T *)(dm_dev ? dm_dev : ctx->born_w), (const T *)ctx->c_dev,
                                              (T *)ctx->born_w, wrt == FWI_WRT_VELOCITY, s));
        if (spec) {
            ctx->four_sweep = true;
            if ((rc = fourier_table(ctx, nt, true, a))) return rc;
        }
        const fwi_ctx::PointSet nobody;
        const fwi_ctx::PointSet *share = &nobody;  // bf16 store: the sources, injected with the share's amplitudes
        const T *share_amp = nullptr;
        if (ctx->qbf16 && ctx->nsrc > 0) {
            if constexpr (std::is_same<T, float>::value) {
                if ((rc = ensure(ctx, ctx->born_src, (size_t)nt * ctx->nsrc * sizeof(T)))) return rc;
                HIPCHK(ctx, launch_born_source_share((const float *)ctx->born_w, (const int64_t *)ctx->src.cidx,
                                                     (const float *)ctx->wav.p, (float *)ctx->born_src.p, nt, ctx->nsrc, s));
                share = &ctx->src;
                share_amp = (const T *)ctx->born_src.p;
            } else {
                return ctx->fail(FWI_ESTATE, "the bf16 store is fp32 only");
            }
        }
        ctx->have_syn = false;           // ctx->series is about to hold dd instead of the forward's synthetics
        ctx->have_dev_residual = false;  // ... and ctx->amp a copy of it, once the sweep has ended
        Sweep sw;
        if ((rc = start_sweep(ctx, sw))) return rc;
        const Store st(ctx);
        T *series = (T *)ctx->series.p;
        const int damp = base_args(ctx, 0).damp;
        // steps first .. first + cnt - 1 of the Born sweep; slot(n): what the store holds of step n (n % S == 0)
        auto born_steps = [&](int first, int cnt, auto slot) -> int {
            const int end = first + cnt;
            for (int n = first; n < end;) {
                if (n % S != 0) {  // up to the next stored step: the plain launches, one call
                    const int m = std::min(end, (n / S + 1) * S) - n;
                    sw.born_w = nullptr;
                    if ((rc = run_steps(ctx, sw, n, 1, m, nobody, (const T *)nullptr, &ctx->rec, series, T(1), none, noq)))
                        return rc;
                    n += m;
                    continue;
                }
                if (fused) {
                    const int m = S == 1 ? end - n : 1;
                    sw.born_w = ctx->born_w;
                    auto qn = [&](int k, const T *&p, const T *&p2) { p = (const T *)slot(k); p2 = nullptr; };
                    if ((rc = run_steps(ctx, sw, n, 1, m, *share, share_amp, &ctx->rec, series, T(1), none, qn))) return rc;
                    n += m;
                    continue;
                }
                if ((rc = run_steps(ctx, sw, n, 1, 1, *share, share_amp, &ctx->rec, series, T(1), none, noq))) return rc;
                if (ctx->qbf16) {
                    if constexpr (std::is_same<T, float>::value)
                        HIPCHK(ctx, launch_born_scatter_bf16(g, (float *)sw.f[sw.cur], slot(n), (const float *)ctx->born_w,
                                                             (const float *)ctx->dz, (const float *)ctx->dy,
                                                             (const float *)ctx->dx, damp, s));
                } else {
                    HIPCHK(ctx, launch_born_scatter<T>(g, (T *)sw.f[sw.cur], (T *)sw.v, (const T *)slot(n),
                                                       (const T *)ctx->born_w, (const T *)ctx->dz, (const T *)ctx->dy,
                                                       (const T *)ctx->dx, damp, s));
                }
                ++n;
            }
            return FWI_OK;
        };
        const bool fused2d = K > 0 && use_fused(ctx, nt);  // the recomputation takes FUSED2D_STEPS steps per launch
        void *fspare[2] = {ctx->fwx[0], ctx->fwx[1]};
        TimeLoop loop(ctx);
        if ((rc = loop.begin())) return rc;
        if (K > 0) {
            Sweep fw = recompute_sweep(ctx);
            for (int n0 = 0, seg = 0; n0 < nt; n0 += K, ++seg) {
                const int cnt = std::min(K, nt - n0);
                if ((rc = restore_segment(ctx, fw, seg))) return rc;
                auto qo = [&](int n) -> T * { return st.seg_slot(n, n0); };
                rc = fused2d ? run_fused(ctx, fw, fspare, n0, 1, cnt, ctx->src, (const T *)ctx->wav.p, nullptr, nullptr, T(0), 1,
                                         st.seg_slot(0, n0))
                             : run_steps(ctx, fw, n0, 1, cnt, ctx->src, (const T *)ctx->wav.p, nullptr, nullptr, T(0), qo, noq);
                if (rc || (rc = born_steps(n0, cnt, [&](int n) -> const void * { return st.seg_slot(n, n0); }))) return rc;
            }
            adopt_recompute(ctx, fw, fspare);
        } else if (spec) {
            // (born_steps' fused path takes all the steps it is given in one run_steps call when S = 1: a batch at a time)
            const int B = ctx->four_batch, R = B + 1, N = (nt + S - 1) / S;
            for (int j0 = 0; j0 < N; j0 += B) {
                const int nb = std::min(B, N - j0), n0 = j0 * S, n1 = std::min(nt, (j0 + nb) * S);
                HIPCHK(ctx, launch_fourier_synthesise<T>(st.ring, spec, g.npts, R, j0 % R, j0, nb,
                                                         (const double *)ctx->four_tw, ctx->four_rows,
                                                         (int)ctx->four_freqs.size(), s));
                if ((rc = born_steps(n0, n1 - n0, [&](int n) -> const void * { return st.ring_slot(n); }))) return rc;
            }
        } else {
            if ((rc = born_steps(0, nt, [&](int n) -> const void * { return st.slot(n); }))) return rc;
        }
        if ((rc = flush_record(ctx, sw, ctx->rec, series, T(1)))) return rc;
        if ((rc = loop.end())) return rc;
        ctx->born_path = fused ? "fused" : "scatter";
        // dd stays on the device as the residual of the next fwi_adjoint(ctx, NULL, ...): per node in ctx->amp (off-grid
        // receivers: gathered per point for the caller, then spread back onto the nodes, as fwi_misfit_l2 does)
        const fwi_ctx::SpreadSet &sp = ctx->rec_sp;
        const void *out = ctx->series.p;
        size_t out_bytes = (size_t)nt * nrec * sizeof(T);
        if (nrec && sp.npts) {
            if ((rc = ensure(ctx, ctx->pts_d, (size_t)nt * sp.npts * sizeof(T)))) return rc;
            HIPCHK(ctx, launch_gather_series<T>((const T *)ctx->series.p, (T *)ctx->pts_d.p, (const int *)sp.pt_start,
                                                (const T *)sp.weight, nt, sp.npts, nrec, s));
            HIPCHK(ctx, launch_scatter_series<T>((const T *)ctx->pts_d.p, (T *)ctx->amp.p, (const int *)sp.owner,
                                                 (const T *)sp.weight, nt, sp.npts, nrec, s));
            out = ctx->pts_d.p;
            out_bytes = (size_t)nt * sp.npts * sizeof(T);
        } else if (nrec) {
            HIPCHK(ctx, hipMemcpyAsync(ctx->amp.p, ctx->series.p, out_bytes, hipMemcpyDeviceToDevice, s));
        }
        if ((rc = download_series(ctx, seis_out, out, (nrec && seis_out) ? out_bytes : 0))) return rc;
        ctx->have_dev_residual = true;
        ctx->resid_pts_in = (nrec && sp.npts) ? fwi_ctx::RESID_PTS_D : fwi_ctx::RESID_PTS_NONE;
        return FWI_OK;
    }

    // Extended Born modelling (fwi_fourier_born_extended[_vec]): the spectrum P_k of the gather goes, one lag per launch
    // (fwi_fbornx.h), into the 2 F volumes that hold M_k, which it destroys; the Born sweep then synthesises its source
    // from P_k with w = -c^2 S.  The images come from the host (`images_host`, nlag model-shaped arrays one behind the
    // other, each through born_w) or from device vectors (`images_dev`).  `axis`: 0 = z, 1 = y, 2 = x of the GridDesc.
    static int fourier_born_extended(fwi_ctx *ctx, bool lag, int axis, int nlag, const int32_t *offsets, const double *taus,
                                     const T *images_host, const void *const *images_dev, const double *a, bool fused,
                                     T *seis_out) {
        const GridDesc &g = ctx->gd;
        const int F = (int)ctx->four_freqs.size();
        int rc = fourier_adjoint_alloc(ctx);
        if (rc) return rc;
        ctx->have_m = false;
        if ((rc = dev_first_use(ctx, &ctx->born_w, (size_t)g.npts * sizeof(T), "born_w"))) return rc;
        const size_t nlog = (size_t)g.nz * g.ny * g.nx;
        for (int l = 0; l < nlag; ++l) {
            const T *img = images_dev ? (const T *)images_dev[l] : (const T *)ctx->born_w;
            if (images_host && (rc = upload_compact<T>(ctx, ctx->born_w, images_host + l * nlog))) return rc;
            if (lag) {
                if ((rc = fourier_weights<T>(ctx, nullptr, &taus[l], true))) return rc;
                HIPCHK(ctx, launch_fbornx_lag<T>((T *)ctx->four_adj, (const T *)ctx->four_acc, img,
                                                 (const double *)ctx->four_w, g.npts, F, l > 0, ctx->stream));
            } else {
                HIPCHK(ctx, launch_fbornx_offset<T>(g, (T *)ctx->four_adj, (const T *)ctx->four_acc, img, F, axis,
                                                    (int64_t)offsets[l], l > 0, ctx->stream));
            }
        }
        return born(ctx, FWI_WRT_SLOWNESS2, nullptr, nullptr, fused, seis_out, (const T *)ctx->four_adj, a);
    }

    // illumination accumulator += sum of the squares of `nslots` store slots (no-op while illumination is disabled)
    static int illum_accumulate(fwi_ctx *ctx, const void *store, int nslots) {
        if (!ctx->h_acc) return FWI_OK;
        HIPCHK(ctx, launch_illum_accumulate<T>((T *)ctx->h_acc, store, ctx->gd.npts, nslots, ctx->qbf16 ? 1 : 0,
                                               ctx->stream));
        return FWI_OK;
    }
};

int create_impl(fwi_ctx *ctx) {
    const fwi_config &c = ctx->cfg;
    const GridDesc &g = ctx->gd;
    const size_t es = ctx->esize;
    int rc;
    auto alloc = [ctx](auto **slot, const char *member, size_t bytes, int index = 0) {
        return dev_acquire(ctx, (void **)slot, bytes, member, index);
    };
    HIPCHK(ctx, hipSetDevice(c.device));
    HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
    HIPCHK(ctx, hipEventCreate(&ctx->ev0));
    HIPCHK(ctx, hipEventCreate(&ctx->ev1));
    const size_t fslack = ctx->place_kind == 2 ? ctx->place_pad : 0;  // (tune_placement may move C; the u buffers
                                                                       // change roles with others and stay where they are)
    for (int i = 0; i < 2; ++i) {
        if ((rc = alloc(&ctx->u[i], "u", (size_t)g.ptot * es, i))) return rc;
        HIPCHK(ctx, hipMemsetAsync(ctx->u[i], 0, (size_t)g.ptot * es, ctx->stream));
    }
    if ((rc = alloc(&ctx->C, "C", (size_t)g.ptot * es + fslack))) return rc;
    HIPCHK(ctx, hipMemsetAsync(ctx->C, 0, (size_t)g.ptot * es + fslack, ctx->stream));
    if ((rc = alloc(&ctx->c_dev, "c_dev", (size_t)g.npts * es))) return rc;
    if ((rc = alloc(&ctx->g_acc, "g_acc", (size_t)g.npts * es))) return rc;
    HIPCHK(ctx, hipMemsetAsync(ctx->g_acc, 0, (size_t)g.npts * es, ctx->stream));
    if ((rc = alloc(&ctx->g_out, "g_out", (size_t)g.npts * es))) return rc;
    if ((rc = alloc(&ctx->dz, "dz", (size_t)g.nz * es))) return rc;
    if ((rc = alloc(&ctx->dy, "dy", (size_t)g.ny * es))) return rc;
    if ((rc = alloc(&ctx->dx, "dx", (size_t)g.nx * es))) return rc;
    if ((rc = alloc(&ctx->red, "red", 64))) return rc;
    if (ctx->fused2d) {  // tile order of the fused 2-D kernel on grids of more than one round of tiles (on THIS device)
        std::vector<int> order;
        fused2d_tile_order(g, ctx->fused_ft, c.npml, order, ctx->cpml ? 1 : 0);
        if (!order.empty()) {
            if ((rc = alloc(&ctx->fused_order, "fused_order", order.size() * sizeof(int)))) return rc;
            HIPCHK(ctx, hipMemcpy(ctx->fused_order, order.data(), order.size() * sizeof(int), hipMemcpyHostToDevice));
        }
    }
    double sm = c.sigma_max;
    const int np_sponge = ctx->cpml ? 0 : c.npml;  // with the CPML the damping factors are off (A = B = 1)
    profile(ctx->pz, g.nz, np_sponge, sm, c.dt);
    profile(ctx->px, g.nx, np_sponge, sm, c.dt);
    if (g.ndim == 3) profile(ctx->py, g.ny, np_sponge, sm, c.dt); else ctx->py.assign(1, 0.0);
    if (ctx->cpml) {
        const int nd[3] = {g.nz, g.ny, g.nx};
        for (int d = 0; d < 3; ++d) {
            if (d == 1 && g.ndim == 2) continue;
            const int n = nd[d], nslab = std::min(n, 2 * c.npml);
            size_t cnt = (size_t)nslab;  // rows padded to cx (16-byte lanes of the z / y border kernels)
            for (int o = 0; o < 3; ++o)
                if (o != d) cnt *= (size_t)(o == 2 ? g.cx : nd[o]);
            ctx->pml_bytes[d] = cnt * es;
            const size_t slack = (d == 2 && ctx->place_kind == 1) ? ctx->place_pad : 0;  // (the x border's arrays can be moved: tune_placement)
            if ((rc = alloc(&ctx->pml_psi[d], "pml_psi", ctx->pml_bytes[d] + slack, d))) return rc;
            if ((rc = alloc(&ctx->pml_zeta[d], "pml_zeta", ctx->pml_bytes[d] + slack, d))) return rc;
            if (ctx->fused2d) {  // the set the fused launch writes (see fwi_ctx::pml_spare_psi)
                if ((rc = alloc(&ctx->pml_spare_psi[d], "pml_spare_psi", ctx->pml_bytes[d], d))) return rc;
                if ((rc = alloc(&ctx->pml_spare_zeta[d], "pml_spare_zeta", ctx->pml_bytes[d], d))) return rc;
                HIPCHK(ctx, hipMemsetAsync(ctx->pml_spare_psi[d], 0, ctx->pml_bytes[d], ctx->stream));
                HIPCHK(ctx, hipMemsetAsync(ctx->pml_spare_zeta[d], 0, ctx->pml_bytes[d], ctx->stream));
            }
            if ((rc = alloc(&ctx->pml_a[d], "pml_a", (size_t)n * es, d))) return rc;
            if ((rc = alloc(&ctx->pml_b[d], "pml_b", (size_t)n * es, d))) return rc;
            std::vector<double> pa(n), pb(n);  // cpml_profiles() of the oracle
            for (int i = 0; i < n; ++i) {
                const double dist = std::max(0.0, std::max((double)c.npml - i, (double)i - (n - 1 - c.npml)));
                const double x = dist / c.npml, sig = sm * x * x, alp = c.pml_alpha_max * (1.0 - x);
                pb[i] = std::exp(-(sig + alp) * c.dt);
                pa[i] = sig > 0.0 ? sig / (sig + alp) * (pb[i] - 1.0) : 0.0;
            }
            int rc2;
            if (c.dtype == FWI_F32) {
                if ((rc2 = upload_vec<float>(ctx, ctx->pml_a[d], pa)) || (rc2 = upload_vec<float>(ctx, ctx->pml_b[d], pb)))
                    return rc2;
            } else {
                if ((rc2 = upload_vec<double>(ctx, ctx->pml_a[d], pa)) || (rc2 = upload_vec<double>(ctx, ctx->pml_b[d], pb)))
                    return rc2;
            }
        }
    }
    if (ctx->cpml && ctx->pml_lines == 3) {
        // the handed-over border terms: (shell rows of z, ny, cx) and (nz + 1, shell rows of y, cx) -- one plane more than
        // the grid, the stream kernel's prefetch runs one plane past the end.  Zeroed once: rows off a thread's shell
        // re-read the first vectors of the arrays and discard them, which must not be NaNs of an earlier allocation.
        const size_t bz = (size_t)pml_shell_rows(g.nz, c.npml, g.r) * g.ny * g.cx * es;
        const size_t by = (size_t)(g.nz + 1) * pml_shell_rows(g.ny, c.npml, g.r) * g.cx * es;
        const size_t slack = ctx->place_kind == 1 ? ctx->place_pad : 0;
        if ((rc = alloc(&ctx->pml_tz, "pml_tz", bz + slack))) return rc;
        if ((rc = alloc(&ctx->pml_ty, "pml_ty", by + slack))) return rc;
        HIPCHK(ctx, hipMemsetAsync(ctx->pml_tz, 0, bz + slack, ctx->stream));
        HIPCHK(ctx, hipMemsetAsync(ctx->pml_ty, 0, by + slack, ctx->stream));
        if (ctx->place_kind == 1) {  // search order: the positions that decided the slab experiments first
            ctx->movable(&ctx->pml_ty, by);
            ctx->movable(&ctx->pml_zeta[2], ctx->pml_bytes[2]);
            ctx->movable(&ctx->pml_tz, bz);
            ctx->movable(&ctx->pml_psi[2], ctx->pml_bytes[2]);
        }
    }
    if (c.dtype == FWI_F32) {
        if ((rc = upload_vec<float>(ctx, ctx->dz, ctx->pz))) return rc;
        if ((rc = upload_vec<float>(ctx, ctx->dy, ctx->py))) return rc;
        if ((rc = upload_vec<float>(ctx, ctx->dx, ctx->px))) return rc;
    } else {
        if ((rc = upload_vec<double>(ctx, ctx->dz, ctx->pz))) return rc;
        if ((rc = upload_vec<double>(ctx, ctx->dy, ctx->py))) return rc;
        if ((rc = upload_vec<double>(ctx, ctx->dx, ctx->px))) return rc;
    }
    return FWI_OK;
}

}  // namespace

extern "C" {

int fwi_abi_version(void) { return FWI_ABI_VERSION; }

int fwi_device_count(int32_t *n_out) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (n_out) *n_out = (e == hipSuccess) ? n : 0;
    return (e == hipSuccess && n > 0) ? FWI_OK : FWI_EHIP;
}

const char *fwi_last_error(const fwi_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

const char *fwi_kernel_name(const fwi_ctx *ctx) { return ctx ? plan_kernel_name(*ctx) : ""; }

int fwi_create(const fwi_config *cfg, fwi_ctx **out) {
    if (!cfg || !out) {
        g_create_error = "fwi_create: null argument";
        return FWI_EINVAL;
    }
    *out = nullptr;
    auto bad = [&](const char *m) {
        g_create_error = std::string("fwi_create: ") + m;
        return FWI_EINVAL;
    };
    if (cfg->struct_size != (int32_t)sizeof(fwi_config)) return bad("struct_size mismatch (ABI)");
    if (cfg->ndim != 2 && cfg->ndim != 3) return bad("ndim must be 2 or 3");
    if (cfg->nz < 1 || cfg->nx < 1 || (cfg->ndim == 3 && cfg->ny < 1)) return bad("empty grid");
    if (cfg->order != 2 && cfg->order != 4 && cfg->order != 8) return bad("order must be 2, 4 or 8");
    if (cfg->nt_max < 1) return bad("nt_max must be >= 1");
    if (cfg->npml < 0) return bad("npml must be >= 0");
    if (!(cfg->h > 0) || !(cfg->dt > 0)) return bad("h and dt must be > 0");
    if (cfg->dtype != FWI_F32 && cfg->dtype != FWI_F64) return bad("dtype must be FWI_F32 or FWI_F64");
    if (cfg->npml > 0 && !(cfg->sigma_max >= 0)) return bad("sigma_max must be >= 0 when npml > 0");
    if (cfg->kernel < FWI_KERNEL_AUTO || cfg->kernel > FWI_KERNEL_STREAM) return bad("unknown kernel id");
    if (cfg->ckpt_interval < 0) return bad("ckpt_interval must be >= 0");
    if (cfg->image_stride < 0) return bad("image_stride must be >= 0");
    if (cfg->image_stride > 1 && cfg->ckpt_interval > 0)
        return bad("image_stride > 1 and ckpt_interval > 0 cannot be combined");
    if (cfg->update_form != FWI_UPDATE_STANDARD && cfg->update_form != FWI_UPDATE_INCREMENT)
        return bad("unknown update_form");
    if (cfg->abc != FWI_ABC_SPONGE && cfg->abc != FWI_ABC_CPML) return bad("unknown abc");
    if (cfg->store_dtype != FWI_STORE_NATIVE && cfg->store_dtype != FWI_STORE_BF16) return bad("unknown store_dtype");
    if (cfg->store_dtype == FWI_STORE_BF16 && cfg->dtype != FWI_F32) return bad("store_dtype bf16 needs an fp32 context");
    if (cfg->launch_mode < FWI_LAUNCH_AUTO || cfg->launch_mode > FWI_LAUNCH_GRAPH) return bad("unknown launch_mode");
    if (!(cfg->pml_alpha_max >= 0)) return bad("pml_alpha_max must be >= 0");
    if (cfg->store_dtype == FWI_STORE_BF16 &&
        (cfg->ndim != 3 || cfg->order != 8 || cfg->kernel == FWI_KERNEL_POINT || cfg->ckpt_interval > 0 ||
         cfg->update_form != FWI_UPDATE_STANDARD || (cfg->abc == FWI_ABC_CPML && cfg->npml > 0)))
        return bad("store_dtype bf16: 3-D fp32 O(8) stream kernel, standard update form, sponge border, no checkpointing");

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
        g_create_error = "fwi_create: no HIP device available (this library has no CPU fallback)";
        return FWI_EHIP;
    }
    if (cfg->device < 0 || cfg->device >= ndev) return bad("device ordinal out of range");

    // Whatever else can refuse the configuration is looked at before the context exists (plan_context: which path the
    // context takes, from the configuration and the creation-time hooks alone): every failure behind `new` leaves through
    // fwi_destroy at the end.
    const Hooks hooks = Hooks::from_env();
    Plan plan;
    std::string why;
    const int planned = plan_context(*cfg, hooks, &plan, &why);
    // (a refused "fixed:" is found after the path is decided, plan_context: the line is still written)
    if (hooks.debug_pml && (planned == FWI_OK || plan.place_kind)) {
        char line[160];
        plan_report(plan, line, sizeof line);
        fprintf(stderr, "%s\n", line);
    }
    if (planned) return bad(why.c_str());

    fwi_ctx *ctx = new (std::nothrow) fwi_ctx;
    if (!ctx) {
        g_create_error = "fwi_create: out of host memory";
        return FWI_ENOMEM;
    }
    static_cast<Plan &>(*ctx) = plan;
    ctx->cfg = *cfg;
    // launch_mode AUTO = stream launches.  hipGraph capture of the time loop was built and measured in round 4 (VERDICT r03
    // item 3) with the mode switched between sweeps of ONE context: -0.6 % (3-D CPML, two kernels per step) ... +1.4 %
    // (2-D 256^2) of the loop time, nothing near the 3 % that would justify a second launch path by default; the host is
    // far ahead of the GPU either way (1.3 ms to submit 500 launches that run 3.1 ms at 256^2).  A first probe that ran the
    // two modes on two contexts side by side had shown the graph 6 - 13 % ahead on the 3-D CPML: an artefact of that set-up
    // (the stream-mode context ran 6 % slower than it does alone), which is why the A/B is done on one context now.
    ctx->graph_mode = cfg->launch_mode == FWI_LAUNCH_GRAPH;
    int rc = create_impl(ctx);
    const size_t vslack = ctx->place_kind ? ctx->place_pad : 0;
    if (rc == FWI_OK && ctx->inc &&
        (ctx->mem.acquire(&ctx->vf, (size_t)ctx->gd.ptot * ctx->esize + vslack, "vf") != hipSuccess ||
         hipMemset(ctx->vf, 0, (size_t)ctx->gd.ptot * ctx->esize + vslack) != hipSuccess))
        rc = ctx->fail(FWI_ENOMEM, "allocating the increment field failed");
    if (rc == FWI_OK && ctx->place_kind && ctx->inc) ctx->movable(&ctx->vf, (size_t)ctx->gd.ptot * ctx->esize);
    if (rc == FWI_OK && ctx->place_kind == 2) ctx->movable(&ctx->C, (size_t)ctx->gd.ptot * ctx->esize);
    if (rc == FWI_OK && (ctx->fused2d || ctx->pair3d)) {
        for (int i = 0; i < 2 && rc == FWI_OK; ++i) {
            if (ctx->mem.acquire(&ctx->fx[i], (size_t)ctx->gd.ptot * ctx->esize, "fx", i) != hipSuccess ||
                hipMemset(ctx->fx[i], 0, (size_t)ctx->gd.ptot * ctx->esize) != hipSuccess)
                rc = ctx->fail(FWI_ENOMEM, "allocating the fused 2-D buffer pair failed");
        }
    }
    if (rc == FWI_OK && ctx->place_mode == PLACE_FIXED) {
        // every allocation was zeroed over its whole padded length where its content matters before the first write
        // (tz, ty, v, C; the x border's psi / zeta are zeroed where they lie at the start of every sweep)
        for (int i = 0; i < ctx->nmov; ++i) {
            ctx->mov_shift[i] = (size_t)ctx->fixed_k[i] * ((size_t)2 << 20);
            *ctx->mov_slot[i] = (char *)*ctx->mov_slot[i] + ctx->mov_shift[i];
        }
    } else if (rc == FWI_OK && ctx->place_mode == PLACE_SEARCH) {
        rc = Impl<float>::tune_placement(ctx);
    }
    if (rc) {
        const std::string msg = "fwi_create: " + ctx->err;
        fwi_destroy(ctx);
        g_create_error = msg;  // (the reason the creation failed, not what fwi_destroy may have had to say after it)
        return rc;
    }
    g_create_error.clear();
    *out = ctx;
    return FWI_OK;
}

void fwi_destroy(fwi_ctx *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->cfg.device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->graph_exec) (void)hipGraphExecDestroy(ctx->graph_exec);
    if (ctx->graph) (void)hipGraphDestroy(ctx->graph);
    if (ctx->comm) (void)ncclCommDestroy(ctx->comm);
    // Every device allocation, from the context's record: each base once, wherever the members point by now -- into a
    // padded allocation (fwi_create, Impl::tune_placement) or at each other's (adopt).  The function returns nothing, so
    // the FIRST free the runtime refuses is reported through the thread's creation error (fwi_last_error(NULL)):
    // "fwi_destroy: hipFree(<member>[<index>]): <HIP error>", <member> being the one the allocation was MADE for (after a
    // sweep that swapped buffers, not necessarily the one that holds it).  The rest is still freed.
    ctx->mem.release_all([](const char *member, int index, int code) {
        char msg[256];
        snprintf(msg, sizeof msg, "fwi_destroy: hipFree(%s[%d]): %s", member, index, hipGetErrorString((hipError_t)code));
        g_create_error = msg;
    });
    if (ctx->pin) (void)hipHostFree(ctx->pin);
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    for (hipEvent_t ev : ctx->awi_ev)
        if (ev) (void)hipEventDestroy(ev);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

int fwi_set_model(fwi_ctx *ctx, const void *c_host) {
    if (!ctx) return FWI_EINVAL;
    if (!c_host) return ctx->fail(FWI_EINVAL, "fwi_set_model: null model");
    (void)hipSetDevice(ctx->cfg.device);
    return DISPATCH(ctx, Impl<float>::set_model(ctx, (const float *)c_host),
                    Impl<double>::set_model(ctx, (const double *)c_host));
}

// What a forward call begins with (include/fwi.h, "a forward call that fails"): the shot before it is given up before
// the first argument is looked at, so that no error return -- a refused argument, a receiver outside the grid found after
// the source set has been replaced, an allocation that does not fit -- leaves flags that describe the old shot beside
// point sets, sizes or buffers of the new one.
static void drop_forward(fwi_ctx *ctx) {
    ctx->have_forward = ctx->have_q = ctx->have_m = ctx->have_syn = ctx->have_dev_residual = ctx->have_irls = false;
    ctx->resid_pts_in = fwi_ctx::RESID_PTS_NONE;
}

int fwi_forward(fwi_ctx *ctx, int32_t nt, int32_t nsrc, const int32_t *src_idx, const void *wavelet,
                int32_t nrec, const int32_t *rec_idx, int32_t save, void *seis_out) {
    if (!ctx) return FWI_EINVAL;
    drop_forward(ctx);
    if (!ctx->have_model) return ctx->fail(FWI_ESTATE, "fwi_forward: call fwi_set_model first");
    if (nt < 1 || nt > ctx->cfg.nt_max)
        return ctx->fail(FWI_EINVAL, "fwi_forward: nt=%d outside [1, nt_max=%d]", nt, ctx->cfg.nt_max);
    if (nsrc < 0 || nrec < 0) return ctx->fail(FWI_EINVAL, "fwi_forward: negative point count");
    if ((nsrc && (!src_idx || !wavelet)) || (nrec && (!rec_idx || !seis_out)))
        return ctx->fail(FWI_EINVAL, "fwi_forward: null buffer");
    (void)hipSetDevice(ctx->cfg.device);
    ctx->src_sp.npts = ctx->rec_sp.npts = 0;  // node-based call
    return DISPATCH(ctx,
                    Impl<float>::forward(ctx, nt, nsrc, src_idx, (const float *)wavelet, nrec, rec_idx,
                                         save, (float *)seis_out),
                    Impl<double>::forward(ctx, nt, nsrc, src_idx, (const double *)wavelet, nrec,
                                          rec_idx, save, (double *)seis_out));
}

// nodes of point p = entries pt_start[p] .. pt_start[p + 1] of the node list (at most 8); weight per entry
static int set_spread(fwi_ctx *ctx, fwi_ctx::SpreadSet &sp, int32_t npts, int32_t nnodes, const int32_t *pt_start,
                      const void *weight, const char *what) {
    sp.npts = 0;
    const SpreadOwners so = spread_owners(npts, nnodes, pt_start, weight != nullptr);
    switch (so.check) {
        case SPREAD_OK: break;
        case SPREAD_BAD_SET: return ctx->fail(FWI_EINVAL, "fwi_forward_spread: bad %s point set", what);
        case SPREAD_NODES_WITHOUT_POINTS: return ctx->fail(FWI_EINVAL, "fwi_forward_spread: %s nodes without points", what);
        case SPREAD_BAD_RANGE:
            return ctx->fail(FWI_EINVAL, "fwi_forward_spread: %s pt_start must run from 0 to the node count", what);
        case SPREAD_BAD_COUNT:
            return ctx->fail(FWI_EINVAL, "fwi_forward_spread: %s point %d has %d nodes (0..8 allowed)", what, so.point,
                             so.count);
    }
    if (npts == 0) return FWI_OK;
    const size_t need = (size_t)std::max(nnodes, npts + 1) * 8 + 16;
    if (int rc = ensure_all(ctx, sp.member, 0, {&sp.pt_start, &sp.owner, &sp.weight}, &sp.cap, need)) return rc;
    HIPCHK(ctx, hipMemcpyAsync(sp.pt_start, pt_start, (size_t)(npts + 1) * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(sp.owner, so.owner.data(), (size_t)nnodes * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(sp.weight, weight, (size_t)nnodes * ctx->esize, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // `owner` goes out of scope
    sp.npts = npts;
    return FWI_OK;
}

int fwi_forward_spread(fwi_ctx *ctx, int32_t nt, int32_t nsrc_pts, int32_t nsrc_nodes, const int32_t *src_idx,
                       const int32_t *src_pt_start, const void *src_weight, const void *wavelet, int32_t nrec_pts,
                       int32_t nrec_nodes, const int32_t *rec_idx, const int32_t *rec_pt_start, const void *rec_weight,
                       int32_t save, void *seis_out) {
    if (!ctx) return FWI_EINVAL;
    drop_forward(ctx);
    if (!ctx->have_model) return ctx->fail(FWI_ESTATE, "fwi_forward_spread: call fwi_set_model first");
    if (nt < 1 || nt > ctx->cfg.nt_max)
        return ctx->fail(FWI_EINVAL, "fwi_forward_spread: nt=%d outside [1, nt_max=%d]", nt, ctx->cfg.nt_max);
    if (nsrc_nodes < 0 || nrec_nodes < 0) return ctx->fail(FWI_EINVAL, "fwi_forward_spread: negative node count");
    if ((nsrc_nodes && (!src_idx || !wavelet)) || (nrec_nodes && (!rec_idx || !seis_out)))
        return ctx->fail(FWI_EINVAL, "fwi_forward_spread: null buffer");
    (void)hipSetDevice(ctx->cfg.device);
    int rc = set_spread(ctx, ctx->src_sp, nsrc_pts, nsrc_nodes, src_pt_start, src_weight, "source");
    if (!rc) rc = set_spread(ctx, ctx->rec_sp, nrec_pts, nrec_nodes, rec_pt_start, rec_weight, "receiver");
    if (rc) {
        ctx->src_sp.npts = ctx->rec_sp.npts = 0;
        return rc;
    }
    return DISPATCH(ctx,
                    Impl<float>::forward(ctx, nt, nsrc_nodes, src_idx, (const float *)wavelet, nrec_nodes, rec_idx, save,
                                         (float *)seis_out),
                    Impl<double>::forward(ctx, nt, nsrc_nodes, src_idx, (const double *)wavelet, nrec_nodes, rec_idx,
                                          save, (double *)seis_out));
}

int fwi_adjoint(fwi_ctx *ctx, const void *residual, int32_t image, void *adj_src_out) {
    if (!ctx) return FWI_EINVAL;
    if (!ctx->have_forward) return ctx->fail(FWI_ESTATE, "fwi_adjoint: no forward run to adjoin");
    if (image && !ctx->have_q)
        return ctx->fail(FWI_ESTATE, "fwi_adjoint: imaging needs fwi_forward(save=1) first");
    if (ctx->nrec && !residual && !ctx->have_dev_residual)
        return ctx->fail(FWI_EINVAL, "fwi_adjoint: null residual (and no fwi_misfit_l2 residual on the device)");
    (void)hipSetDevice(ctx->cfg.device);
    return DISPATCH(ctx, Impl<float>::adjoint(ctx, (const float *)residual, image, (float *)adj_src_out),
                    Impl<double>::adjoint(ctx, (const double *)residual, image, (double *)adj_src_out));
}

int fwi_set_model_vec(fwi_ctx *ctx, int32_t slot) {
    if (!ctx) return FWI_EINVAL;
    VEC_OR_FAIL(ctx, v, slot);
    (void)hipSetDevice(ctx->cfg.device);
    return DISPATCH(ctx, Impl<float>::set_model_vec(ctx, v), Impl<double>::set_model_vec(ctx, v));
}

// FWI_BORN_AUTO on a context that has both paths: decided by measurement (tools/born_probe.py; on the
// bf16, strided and checkpointed stores too: profiles/r06_born_modes.json)
constexpr bool BORN_AUTO_IS_FUSED = true;

// contexts whose step kernel has the Born variants of fwi_born3d.hip (bf16 store: fwi_born3d_bf16.hip)
static bool born_fused_supported(const fwi_ctx *ctx) {
    return ctx->gd.ndim == 3 && ctx->cfg.dtype == FWI_F32 && ctx->cfg.order == 8 && ctx->kernel == K_STREAM && !ctx->cpml;
}

// the argument and state checks the Born calls share; *fused: the path the sweep takes.  `imaging`: fwi_born_imaging[_vec],
// defined on every store; the exact operator needs every q^n, in the field's type, resident at once.
static int born_callable(fwi_ctx *ctx, const char *who, bool imaging, int32_t wrt, int32_t mode, bool *fused) {
    if (wrt != FWI_WRT_VELOCITY && wrt != FWI_WRT_SLOWNESS2)
        return ctx->fail(FWI_EINVAL, "%s: unknown parametrisation %d", who, (int)wrt);
    if (mode != FWI_BORN_AUTO && mode != FWI_BORN_SCATTER && mode != FWI_BORN_FUSED)
        return ctx->fail(FWI_EINVAL, "%s: unknown mode %d", who, (int)mode);
    if (!imaging) {
        if (ctx->istride > 1)
            return ctx->fail(FWI_EINVAL, "%s: not available with image_stride > 1 (the store holds every %d-th step only; "
                                         "fwi_born_imaging serves this context)", who, ctx->istride);
        if (ctx->qbf16)
            return ctx->fail(FWI_EINVAL, "%s: not available with store_dtype = bf16 (fwi_born_imaging serves this context)", who);
        if (ctx->ckpt > 0)
            return ctx->fail(FWI_EINVAL, "%s: not available with ckpt_interval > 0 (the store holds one segment at a time; "
                                         "fwi_born_imaging serves this context)", who);
    }
    if (mode == FWI_BORN_FUSED && !born_fused_supported(ctx))
        return ctx->fail(FWI_EINVAL, "%s: FWI_BORN_FUSED: this context has no fused Born path (3-D fp32 O(8) stream "
                                     "kernel without the CPML only)", who);
    *fused = mode == FWI_BORN_FUSED || (mode == FWI_BORN_AUTO && BORN_AUTO_IS_FUSED && born_fused_supported(ctx));
    if (!ctx->four_freqs.empty())
        return ctx->fail(FWI_ESTATE, "%s: this context keeps the forward term as Fourier coefficients "
                                     "(fwi_set_fourier_store), which no Born sweep reads; switch it off first", who);
    if (!ctx->have_forward || !ctx->have_q)
        return ctx->fail(FWI_ESTATE, "%s: needs fwi_forward(save=1) on this context first", who);
    return FWI_OK;
}

static int born_host(fwi_ctx *ctx, const char *who, bool imaging, int32_t wrt, const void *dm_host, int32_t mode,
                     void *seis_out) {
    if (!ctx) return FWI_EINVAL;
    if (!dm_host) return ctx->fail(FWI_EINVAL, "%s: null model perturbation", who);
    bool fused = false;
    int rc = born_callable(ctx, who, imaging, wrt, mode, &fused);
    if (rc) return rc;
    (void)hipSetDevice(ctx->cfg.device);
    return DISPATCH(ctx, Impl<float>::born(ctx, wrt, (const float *)dm_host, nullptr, fused, (float *)seis_out),
                    Impl<double>::born(ctx, wrt, (const double *)dm_host, nullptr, fused, (double *)seis_out));
}

static int born_vec(fwi_ctx *ctx, const char *who, bool imaging, int32_t wrt, int32_t slot, int32_t mode, void *seis_out) {
    if (!ctx) return FWI_EINVAL;
    void *v = vec_slot(ctx, slot);
    if (!v) return ctx->fail(FWI_EINVAL, "%s: vector slot %d does not exist", who, (int)slot);
    bool fused = false;
    int rc = born_callable(ctx, who, imaging, wrt, mode, &fused);
    if (rc) return rc;
    (void)hipSetDevice(ctx->cfg.device);
    return DISPATCH(ctx, Impl<float>::born(ctx, wrt, nullptr, v, fused, (float *)seis_out),
                    Impl<double>::born(ctx, wrt, nullptr, v, fused, (double *)seis_out));
}

int fwi_born(fwi_ctx *ctx, int32_t wrt, const void *dm_host, int32_t mode, void *seis_out) {
    return born_host(ctx, "fwi_born", false, wrt, dm_host, mode, seis_out);
}

int fwi_born_vec(fwi_ctx *ctx, int32_t wrt, int32_t slot, int32_t mode, void *seis_out) {
    return born_vec(ctx, "fwi_born_vec", false, wrt, slot, mode, seis_out);
}

int fwi_born_imaging(fwi_ctx *ctx, int32_t wrt, const void *dm_host, int32_t mode, void *seis_out) {
    return born_host(ctx, "fwi_born_imaging", true, wrt, dm_host, mode, seis_out);
}

int fwi_born_imaging_vec(fwi_ctx *ctx, int32_t wrt, int32_t slot, int32_t mode, void *seis_out) {
    return born_vec(ctx, "fwi_born_imaging_vec", true, wrt, slot, mode, seis_out);
}

const char *fwi_born_path(const fwi_ctx *ctx) { return ctx ? ctx->born_path : ""; }

// the argument and state checks the Born calls on the Fourier store share; *fused as born_callable sets it
static int fourier_born_callable(fwi_ctx *ctx, const char *who, int32_t mode, const double *fw, bool *fused) {
    if (mode != FWI_BORN_AUTO && mode != FWI_BORN_SCATTER && mode != FWI_BORN_FUSED)
        return ctx->fail(FWI_EINVAL, "%s: unknown mode %d", who, (int)mode);
    if (mode == FWI_BORN_FUSED && !born_fused_supported(ctx))
        return ctx->fail(FWI_EINVAL, "%s: FWI_BORN_FUSED: this context has no fused Born path (3-D fp32 O(8) stream "
                                     "kernel without the CPML only)", who);
    *fused = mode == FWI_BORN_FUSED || (mode == FWI_BORN_AUTO && BORN_AUTO_IS_FUSED && born_fused_supported(ctx));
    if (int rc = fourier_callable(ctx, who, false)) return rc;
    return fourier_weight_args(ctx, who, fw, false);
}

// `dm_host`: fwi_fourier_born, else the device vector `dm_dev` of fwi_fourier_born_vec
static int fourier_born(fwi_ctx *ctx, const char *who, int32_t wrt, const void *dm_host, const void *dm_dev,
                        const double *fw, int32_t mode, void *seis_out) {
    if (wrt != FWI_WRT_VELOCITY && wrt != FWI_WRT_SLOWNESS2)
        return ctx->fail(FWI_EINVAL, "%s: unknown parametrisation %d", who, (int)wrt);
    bool fused = false;
    if (int rc = fourier_born_callable(ctx, who, mode, fw, &fused)) return rc;
    (void)hipSetDevice(ctx->cfg.device);
    return DISPATCH(ctx, Impl<float>::born(ctx, wrt, (const float *)dm_host, dm_dev, fused, (float *)seis_out,
                                           (const float *)ctx->four_acc, fw),
                    Impl<double>::born(ctx, wrt, (const double *)dm_host, dm_dev, fused, (double *)seis_out,
                                       (const double *)ctx->four_acc, fw));
}

int fwi_fourier_born(fwi_ctx *ctx, int32_t wrt, const void *dm_host, const double *freq_weights, int32_t mode,
                     void *seis_out) {
    if (!ctx) return FWI_EINVAL;
    if (!dm_host) return ctx->fail(FWI_EINVAL, "fwi_fourier_born: null model perturbation");
    return fourier_born(ctx, "fwi_fourier_born", wrt, dm_host, nullptr, freq_weights, mode, seis_out);
}

int fwi_fourier_born_vec(fwi_ctx *ctx, int32_t wrt, int32_t slot, const double *freq_weights, int32_t mode,
                         void *seis_out) {
    if (!ctx) return FWI_EINVAL;
    VEC_OR_FAIL(ctx, v, slot);
    return fourier_born(ctx, "fwi_fourier_born_vec", wrt, nullptr, v, freq_weights, mode, seis_out);
}

// `images_host`: fwi_fourier_born_extended, else the vector slots `slots` of fwi_fourier_born_extended_vec
static int fourier_born_extended(fwi_ctx *ctx, const char *who, int32_t kind, int32_t axis, int32_t nlag,
                                 const int32_t *offsets, const double *taus, const void *images_host,
                                 const int32_t *slots, const double *fw, int32_t mode, void *seis_out) {
    if (kind != FWI_EXT_OFFSET && kind != FWI_EXT_TIMELAG)
        return ctx->fail(FWI_EINVAL, "%s: unknown kind %d", who, (int)kind);
    const bool lag = kind == FWI_EXT_TIMELAG;
    if (nlag < 1) return ctx->fail(FWI_EINVAL, "%s: nlag=%d is below 1", who, (int)nlag);
    if (lag ? !taus : !offsets) return ctx->fail(FWI_EINVAL, "%s: null %s", who, lag ? "taus" : "offsets");
    int ax = 0;
    if (!lag)
        if (int rc = fourier_axis(ctx, who, axis, &ax)) return rc;
    std::vector<const void *> dev;
    for (int l = 0; slots && l < nlag; ++l) {
        dev.push_back(vec_slot(ctx, slots[l]));
        if (!dev.back())
            return ctx->fail(FWI_EINVAL, "%s: slots[%d]: vector slot %d does not exist", who, l, (int)slots[l]);
    }
    for (int l = 0; l < nlag; ++l) {
        if (lag)
            if (int rc = fourier_tau_ok(ctx, who, taus[l], l, false)) return rc;
        for (int m = 0; m < l; ++m)
            if (lag ? taus[m] == taus[l] : offsets[m] == offsets[l])
                return ctx->fail(FWI_EINVAL, "%s: %s[%d] repeats %s[%d]", who, lag ? "taus" : "offsets", l,
                                 lag ? "taus" : "offsets", m);
    }
    bool fused = false;
    if (int rc = fourier_born_callable(ctx, who, mode, fw, &fused)) return rc;
    for (int l = 0; lag && l < nlag; ++l)
        if (int rc = fourier_tau_ok(ctx, who, taus[l], l, true)) return rc;
    (void)hipSetDevice(ctx->cfg.device);
    const void *const *d = slots ? dev.data() : nullptr;
    return DISPATCH(ctx, Impl<float>::fourier_born_extended(ctx, lag, ax, nlag, offsets, taus, (const float *)images_host, d,
                                                            fw, fused, (float *)seis_out),
                    Impl<double>::fourier_born_extended(ctx, lag, ax, nlag, offsets, taus, (const double *)images_host, d,
                                                        fw, fused, (double *)seis_out));
}

int fwi_fourier_born_extended(fwi_ctx *ctx, int32_t kind, int32_t axis, int32_t nlag, const int32_t *offsets,
                              const double *taus, const void *images_host, const double *freq_weights, int32_t mode,
                              void *seis_out) {
    if (!ctx) return FWI_EINVAL;
    if (!images_host) return ctx->fail(FWI_EINVAL, "fwi_fourier_born_extended: null images");
    return fourier_born_extended(ctx, "fwi_fourier_born_extended", kind, axis, nlag, offsets, taus, images_host, nullptr,
                                 freq_weights, mode, seis_out);
}

int fwi_fourier_born_extended_vec(fwi_ctx *ctx, int32_t kind, int32_t axis, int32_t nlag, const int32_t *offsets,
                                  const double *taus, const int32_t *slots, const double *freq_weights, int32_t mode,
                                  void *seis_out) {
    if (!ctx) return FWI_EINVAL;
    if (!slots) return ctx->fail(FWI_EINVAL, "fwi_fourier_born_extended_vec: null slots");
    return fourier_born_extended(ctx, "fwi_fourier_born_extended_vec", kind, axis, nlag, offsets, taus, nullptr, slots,
                                 freq_weights, mode, seis_out);
}

int fwi_set_illumination(fwi_ctx *ctx, int32_t on) {
    if (!ctx) return FWI_EINVAL;
    if (on && !ctx->four_freqs.empty())
        return ctx->fail(FWI_EINVAL, "fwi_set_illumination: not available with the Fourier forward-term store "
                                     "(fwi_set_fourier_store): the band-limited term is no measure of the illumination");
    (void)hipSetDevice(ctx->cfg.device);
    const size_t bytes = (size_t)ctx->gd.npts * ctx->esize;
    if (on && !ctx->h_acc) {
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        if (int rc = dev_acquire(ctx, &ctx->h_acc, bytes, "h_acc")) return rc;
        hipError_t e = hipMemsetAsync(ctx->h_acc, 0, bytes, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) {
            (void)ctx->mem.release(&ctx->h_acc);
            return ctx->fail(FWI_EHIP, "fwi_set_illumination: %s", hipGetErrorString(e));
        }
    } else if (!on && ctx->h_acc) {
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // no sweep in flight still adds into it
        return dev_release(ctx, &ctx->h_acc, "h_acc");
    }
    return FWI_OK;
}

// Frees the arrays of the Fourier store; the context is back on its configured store.
static int fourier_release(fwi_ctx *ctx) {
    // the state first: a synchronise or a free that the runtime refuses must not leave a context that says it holds
    // Q_k or M_k beside arrays already given up (fwi_adjoint(image) would synthesise from a null pointer)
    if (!ctx->four_freqs.empty()) {
        ctx->store_held = 0;
        ctx->have_q = false;
    }
    ctx->four_freqs.clear();
    ctx->four_batch = ctx->four_rows = 0;
    ctx->four_sweep = false;
    ctx->have_m = false;
    const struct {
        void **slot;
        const char *member;
    } arrays[] = {{&ctx->four_acc, "four_acc"}, {&ctx->four_ring, "four_ring"}, {&ctx->four_tw, "four_tw"},
                  {&ctx->four_adj, "four_adj"}, {&ctx->four_w, "four_w"}};
    if (std::any_of(std::begin(arrays), std::end(arrays), [](const auto &a) { return *a.slot != nullptr; }))
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // no sweep still uses them
    for (const auto &a : arrays)
        if (int rc = dev_release(ctx, a.slot, a.member)) return rc;  // (the pointer is null by then: dev_release)
    return FWI_OK;
}

int fwi_set_fourier_store(fwi_ctx *ctx, int32_t nfreq, const double *freqs_hz, int32_t batch) {
    if (!ctx) return FWI_EINVAL;
    (void)hipSetDevice(ctx->cfg.device);
    if (nfreq == 0) return fourier_release(ctx);
    if (nfreq < 0 || nfreq > FWI_FOURIER_FMAX)
        return ctx->fail(FWI_EINVAL, "fwi_set_fourier_store: nfreq=%d outside [0, %d]", (int)nfreq, FWI_FOURIER_FMAX);
    if (!freqs_hz) return ctx->fail(FWI_EINVAL, "fwi_set_fourier_store: null frequencies");
    if (batch < 1 || batch > FWI_FOURIER_BMAX)
        return ctx->fail(FWI_EINVAL, "fwi_set_fourier_store: batch=%d outside [1, %d]", (int)batch, FWI_FOURIER_BMAX);
    if (ctx->ckpt > 0)
        return ctx->fail(FWI_EINVAL, "fwi_set_fourier_store: not available with ckpt_interval > 0 (checkpointing recomputes "
                                     "the forward term; the Fourier store replaces it)");
    if (ctx->qbf16)
        return ctx->fail(FWI_EINVAL, "fwi_set_fourier_store: not available with store_dtype = bf16 (the coefficients are "
                                     "kept in the field's type)");
    if (ctx->h_acc)
        return ctx->fail(FWI_EINVAL, "fwi_set_fourier_store: not available while illumination is enabled "
                                     "(fwi_set_illumination): the band-limited term is no measure of it");
    const double nyq = 1.0 / (2.0 * ctx->istride * ctx->cfg.dt);
    for (int k = 0; k < nfreq; ++k) {
        const double f = freqs_hz[k];
        if (!std::isfinite(f)) return ctx->fail(FWI_EINVAL, "fwi_set_fourier_store: frequency %d is not finite", k);
        if (f < 0.0) return ctx->fail(FWI_EINVAL, "fwi_set_fourier_store: frequency %d is negative (%g Hz)", k, f);
        if (f > nyq * (1.0 + FOURIER_NYQUIST_RTOL))
            return ctx->fail(FWI_EINVAL, "fwi_set_fourier_store: frequency %d (%g Hz) is above the Nyquist frequency %g Hz "
                                         "of the sampled time axis (image_stride %d, dt %g s)", k, f, nyq, ctx->istride,
                             ctx->cfg.dt);
        for (int m = 0; m < k; ++m)
            if (freqs_hz[m] == f)
                return ctx->fail(FWI_EINVAL, "fwi_set_fourier_store: frequencies %d and %d are equal (%g Hz)", m, k, f);
    }
    if (int rc = fourier_release(ctx)) return rc;
    ctx->store_held = 0;
    ctx->have_q = false;  // (before the free below can fail: the store it speaks of is about to go)
    if (ctx->q_store) {  // the native store of an earlier forward: its memory is what this store is there to save
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        if (int rc = dev_release(ctx, &ctx->q_store, "q_store")) return rc;
    }
    ctx->four_freqs.assign(freqs_hz, freqs_hz + nfreq);
    ctx->four_batch = batch;
    return FWI_OK;
}

int fwi_adjoint_spectral(fwi_ctx *ctx, const void *residual, void *adj_src_out) {
    if (!ctx) return FWI_EINVAL;
    if (int rc = fourier_callable(ctx, "fwi_adjoint_spectral", false)) return rc;
    if (ctx->nrec && !residual && !ctx->have_dev_residual)
        return ctx->fail(FWI_EINVAL, "fwi_adjoint_spectral: null residual (and no fwi_misfit_l2 residual on the device)");
    (void)hipSetDevice(ctx->cfg.device);
    return DISPATCH(ctx, Impl<float>::adjoint(ctx, (const float *)residual, 0, (float *)adj_src_out, true),
                    Impl<double>::adjoint(ctx, (const double *)residual, 0, (double *)adj_src_out, true));
}

int fwi_store_bytes(fwi_ctx *ctx, int64_t *bytes_out) {
    if (!ctx) return FWI_EINVAL;
    if (!bytes_out) return ctx->fail(FWI_EINVAL, "fwi_store_bytes: null output");
    *bytes_out = (int64_t)ctx->store_held;
    return FWI_OK;
}

int fwi_last_loop_ms(fwi_ctx *ctx, double *ms_out) {
    if (!ctx || !ms_out) return FWI_EINVAL;
    if (!ctx->have_loop_time) return ctx->fail(FWI_ESTATE, "fwi_last_loop_ms: no time loop has run");
    (void)hipSetDevice(ctx->cfg.device);
    HIPCHK(ctx, hipEventSynchronize(ctx->ev1));
    float ms = 0.f;
    HIPCHK(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    *ms_out = ms;
    return FWI_OK;
}

int fwi_set_launch_mode(fwi_ctx *ctx, int32_t mode) {
    if (!ctx) return FWI_EINVAL;
    if (mode < FWI_LAUNCH_AUTO || mode > FWI_LAUNCH_GRAPH) return ctx->fail(FWI_EINVAL, "fwi_set_launch_mode: unknown mode %d", mode);
    ctx->graph_mode = mode == FWI_LAUNCH_GRAPH;  // (AUTO = stream, see fwi_create)
    return FWI_OK;
}

int fwi_check_padding(fwi_ctx *ctx, int64_t *dirty_out) {
    if (!ctx || !dirty_out) return FWI_EINVAL;
    (void)hipSetDevice(ctx->cfg.device);
    unsigned long long *cnt = (unsigned long long *)(ctx->red + 6);
    HIPCHK(ctx, hipMemsetAsync(cnt, 0, sizeof(unsigned long long), ctx->stream));
    for (void *f : {ctx->u[0], ctx->u[1], ctx->C, ctx->vf, ctx->fwv, ctx->fx[0], ctx->fx[1], ctx->fwd[0], ctx->fwd[1],
                    ctx->fwx[0], ctx->fwx[1]}) {
        if (!f) continue;
        HIPCHK(ctx, DISPATCH(ctx, launch_count_dirty_padding<float>(ctx->gd, (const float *)f, cnt, ctx->stream),
                             launch_count_dirty_padding<double>(ctx->gd, (const double *)f, cnt, ctx->stream)));
    }
    unsigned long long n = 0;
    HIPCHK(ctx, hipMemcpyAsync(&n, cnt, sizeof n, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    *dirty_out = (int64_t)n;
    return FWI_OK;
}

int fwi_placement_info(fwi_ctx *ctx, double *us_before_out, double *us_after_out, int64_t *shift_bytes_out) {
    if (!ctx) return FWI_EINVAL;
    if (us_before_out) *us_before_out = ctx->place_us[0];
    if (us_after_out) *us_after_out = ctx->place_us[1];
    if (shift_bytes_out)
        for (int i = 0; i < 8; ++i) shift_bytes_out[i] = i < ctx->nmov ? (int64_t)ctx->mov_shift[i] : 0;
    return FWI_OK;
}

int fwi_last_host_ms(fwi_ctx *ctx, double *submit_ms_out, double *graph_build_ms_out) {
    if (!ctx) return FWI_EINVAL;
    if (!ctx->have_loop_time) return ctx->fail(FWI_ESTATE, "fwi_last_host_ms: no time loop has run");
    if (submit_ms_out) *submit_ms_out = ctx->host_submit_ms;
    if (graph_build_ms_out) *graph_build_ms_out = ctx->host_graph_ms;
    return FWI_OK;
}

int fwi_synchronize(fwi_ctx *ctx) {
    if (!ctx) return FWI_EINVAL;
    (void)hipSetDevice(ctx->cfg.device);
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return FWI_OK;
}

}  // extern "C"

namespace fwi {
void set_global_error(const std::string &msg) { g_create_error = msg; }
}  // namespace fwi
