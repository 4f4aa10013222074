// What the host units of the C ABI share (fwi_api.hip and fwi_api_{misfit,fourier,vec,eikonal,comm}.hip): the context, the
// error and dispatch macros, and the few helpers that cross from one unit into another.  Private, like the launch
// headers; whatever a single unit uses stays in that unit.
#pragma once

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>  // fwi_ctx::comm

#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/fwi.h"
#include "fwi_devmem.h"
#include "fwi_kernels.h"

using namespace fwi;

namespace fwi {

// Fourier store: a frequency within this relative distance of 1 / (2 S dt) is the Nyquist frequency of the sampled axis
// (weight 1 / N; fourier.NYQUIST_RTOL of the NumPy twin), and none may lie further above it
constexpr double FOURIER_NYQUIST_RTOL = 1e-9;

inline std::string vformat(const char *fmt, va_list ap) {
    char buf[512];
    vsnprintf(buf, sizeof buf, fmt, ap);
    return buf;
}

// A device buffer the context owns and grows on demand (ensure); `member`[`index`] is what fwi_ctx::mem records it as
struct Buf {
    const char *member;
    int index;
    void *p = nullptr;
    size_t cap = 0;
    explicit Buf(const char *m, int i = 0) : member(m), index(i) {}
};

inline int hip_malloc_code(void **p, size_t bytes) { return (int)hipMalloc(p, bytes); }
inline int hip_free_code(void *p) { return (int)hipFree(p); }

}  // namespace fwi

// The context: what was decided for it before anything was allocated (fwi::Plan: gd, kernel, tune, inc, cpml, fused2d, ...;
// fwi_plan.h), and everything it owns and remembers since.
struct fwi_ctx : fwi::Plan {
    fwi_config cfg;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool have_loop_time = false;
    // FWI_LAUNCH_GRAPH: the time loop of a sweep is captured and launched as one hipGraph.  The executable graph of
    // the last sweep is kept until the next sweep (or destroy) replaces it -- it may still be running when the call
    // that launched it returns its samples.
    bool graph_mode = false;
    hipGraph_t graph = nullptr;
    hipGraphExec_t graph_exec = nullptr;
    double host_submit_ms = 0.0, host_graph_ms = 0.0;

    // Every device allocation of the context is made through `mem` (dev_acquire, ensure, alloc_all) and recorded there
    // under the member it is made for; fwi_destroy frees from that record, whatever the members point at by then.
    DeviceMemory mem{hip_malloc_code, hip_free_code};

    // device fields
    void *u[2] = {nullptr, nullptr};  // padded wavefields (ping-pong)
    void *vf = nullptr, *fwv = nullptr;  // increment form: v of the running sweep / of the checkpointed forward recomputation
    int *fused_order = nullptr;  // Fused2dArgs::tile_order (device; grids of more than one round of tiles with a border)
    // convolutional PML: memory variables per axis (z, y, x), compact over that axis' border, and 1-D coefficients;
    // pml_tz / pml_ty: the term T_d that the line launch of an axis in pml_lines hands to the step kernel, arrays compact
    // over the axis' shell (StepArgs::pml_tz / pml_ty; scratch within one time step: one pair serves every sweep)
    void *pml_tz = nullptr, *pml_ty = nullptr;
    void *pml_psi[3] = {nullptr, nullptr, nullptr}, *pml_zeta[3] = {nullptr, nullptr, nullptr};
    // Placement (Plan::place_kind): each movable array sits mov_shift bytes into an allocation place_pad bytes longer than
    // the array -- at the position Impl::tune_placement measured as the fastest, or where "fixed:" asked (0 = not moved)
    int nmov = 0;                 // the movable arrays in search order: the member that points at them, their size,
    void **mov_slot[8] = {};      // how far into their allocation they currently sit
    size_t mov_bytes[8] = {}, mov_shift[8] = {};
    void movable(void **slot, size_t bytes) {
        if (place_pad && nmov < 8) {
            mov_slot[nmov] = slot;
            mov_bytes[nmov] = bytes;
            mov_shift[nmov++] = 0;
        }
    }
    float place_us[2] = {0.f, 0.f};  // step time before / after the placement search (fwi_placement_info)
    // with checkpointing: the memory variables of the forward recomputation (the running adjoint sweep keeps its own
    // in the set above) and, per snapshot, a copy of the forward set (psi then zeta, axis by axis)
    void *pml_psi_fw[3] = {nullptr, nullptr, nullptr}, *pml_zeta_fw[3] = {nullptr, nullptr, nullptr};
    // 2-D contexts that carry the CPML inside the fused launch: the set of arrays the launch writes (swapped with the
    // set it read after every launch; zeroed once -- the pad columns of the z border's rows are never written)
    void *pml_spare_psi[3] = {nullptr, nullptr, nullptr}, *pml_spare_zeta[3] = {nullptr, nullptr, nullptr};
    void *pml_snap = nullptr;
    size_t pml_snap_stride = 0;  // bytes of one snapshot of the memory variables
    void *pml_a[3] = {nullptr, nullptr, nullptr}, *pml_b[3] = {nullptr, nullptr, nullptr};
    size_t pml_bytes[3] = {0, 0, 0};
    void *C = nullptr;                // padded dt^2 c^2
    void *c_dev = nullptr;            // compact velocity
    void *dz = nullptr, *dy = nullptr, *dx = nullptr;
    void *q_store = nullptr;  // nt_max x npts forward terms (every istride-th step)
    void *logical = nullptr;  // nz x ny x nx staging array for host <-> compact copies when cx != nx
    void *g_acc = nullptr;    // compact gradient accumulator
    void *g_out = nullptr;    // compact scratch for fwi_gradient (and fwi_illumination)
    // source-side illumination (fwi_set_illumination): compact accumulator of sum q^2 over the imaging steps of every
    // fwi_adjoint(image) since the last fwi_gradient_reset; nullptr = disabled (the default: no launch, no memory)
    void *h_acc = nullptr;
    // Fourier-compressed forward-term store (fwi_set_fourier_store; fwi_fourier.hip): four_freqs.size() = F > 0 while
    // it is on.  2 F compact accumulator volumes (Re Q_k, Im Q_k), four_batch + 1 compact ring slots (sample j in slot
    // j % (four_batch + 1)) and the twiddle table of the running sweep, all allocated by the first fwi_forward(save):
    // four_acc, four_ring, four_tw
    std::vector<double> four_freqs;
    int four_batch = 0;
    int four_rows = 0;        // rows per frequency of four_tw: ceil(nt_max / istride) + FOURIER_BMAX - 1
    bool four_sweep = false;  // the running sweep goes through the Fourier store: one step per launch
    std::vector<double> four_tw_host;
    // Spectral imaging (fwi_adjoint_spectral; fwi_fimage.hip): 2 F compact accumulator volumes (Re M_k, Im M_k) of the
    // adjoint field (four_adj), allocated by the first fwi_adjoint_spectral; have_m: they hold the M_k that go with the Q_k of the
    // latest forward(save).  four_w: the F weights a_k w_k of the running image / illumination pass on the device (the
    // 2 F of a time-lag image, fwi_feximage.hip; the F of a split image with its taps behind them at FWI_FOURIER_FMAX,
    // fwi_fsplit.hip; room for 2 FWI_FOURIER_FMAX doubles).
    void *four_acc = nullptr, *four_ring = nullptr, *four_tw = nullptr, *four_adj = nullptr, *four_w = nullptr;
    bool have_m = false;
    std::vector<double> four_w_host;
    size_t store_held = 0;    // device bytes held for the forward store of whichever kind (fwi_store_bytes)
    // Born modelling (fwi_born): w = dC / C of the last perturbation, compact; allocated by the first fwi_born call
    void *born_w = nullptr;
    const char *born_path = "none";  // path of the last Born sweep (fwi_born_path)
    double *red = nullptr;    // reduction scalars

    // host copies
    std::vector<double> pz, py, px;
    bool have_model = false;

    // per-shot point sets (device) and their sizes
    int nt = 0, nsrc = 0, nrec = 0;
    bool have_forward = false, have_q = false;
    bool have_syn = false;  // ctx->series still holds the last forward's synthetics (an adjoint sweep records its
                            // source-side series into the same buffer)
    bool have_dev_residual = false;  // ctx->amp holds the residual fwi_misfit_l2 formed on the device
    // A point set on the device: original order (sampling, POINT-kernel injection) and the
    // copy sorted by stream-kernel tile with its CSR offsets (fused injection).  The tables are built on the host by
    // fwi_points.h (StepTable, Fused2dTables, Pair3dTable), which knows no device; Impl<T>::upload_set permutes the typed
    // coefficients by each table's `col` and uploads them, on every forward call.
    struct PointSet {
        const char *member;  // "src" / "rec": what the set's arrays are recorded as (indices 0 ... 25, in upload_set's order)
        explicit PointSet(const char *m = "") : member(m), s_start(m, 10), pr_start(m, 24), pr_ent(m, 25) {}
        int n = 0;
        void *pidx = nullptr, *cidx = nullptr, *cu = nullptr, *cq = nullptr;
        void *s_pidx = nullptr, *s_cidx = nullptr, *s_cu = nullptr, *s_cq = nullptr,
             *s_col = nullptr, *s_run = nullptr;
        Buf s_start;
        size_t cap = 0;
        // tables for the 2-D fused kernel: injection entries per tile (extended region) and
        // sampling entries per tile (interior)
        void *fi_start = nullptr, *fi_lz = nullptr, *fi_lx = nullptr, *fi_col = nullptr, *fi_int = nullptr,
             *fi_cidx = nullptr, *fi_cu = nullptr, *fi_cq = nullptr, *fi_run = nullptr;
        void *fr_start = nullptr, *fr_lz = nullptr, *fr_lx = nullptr, *fr_col = nullptr;
        size_t fcap = 0, fcap_start = 0;
        // entries of the 3-D two-step kernel, CSR over its workgroups
        Buf pr_start, pr_ent;
    } src{"src"}, rec{"rec"};
    // Off-grid points of the last forward (fwi_forward_spread): per point set the CSR over points, the owner of
    // every node entry and its interpolation weight; time series cross the boundary per POINT and are scattered /
    // gathered on the device.  npts = 0: node-based call.  (set_spread; the set's checks and the owner table: spread_owners,
    // fwi_points.h)
    struct SpreadSet {
        const char *member;
        int npts = 0;
        void *pt_start = nullptr, *owner = nullptr, *weight = nullptr;
        size_t cap = 0;
    } src_sp{"src_sp"}, rec_sp{"rec_sp"};
    // pts_a: (nt, npts) per-point series being uploaded / downloaded
    // pts_d: (nt, nrec points) gathered synthetics of the last forward (fwi_misfit_l2)
    // wav: (nt, nsrc) source wavelets of the last forward (kept for recomputation)
    // amp: (nt, nrec) residual being back-propagated
    // series: (nt, n) sampled series of the running sweep
    // born_src: Born modelling on a bf16 store: (nt, nsrc) amplitudes w(x_s) wav^n_s of the source's exact share
    // (launch_born_source_share)
    Buf pts_a{"pts_a"}, pts_d{"pts_d"}, wav{"wav"}, amp{"amp"}, series{"series"}, born_src{"born_src"};
    std::vector<void *> vecs;  // optimiser vectors (compact, model-sized)
    // smooth_tmp: compact ping-pong vector of fwi_vec_smooth; allocated by its first call
    // reg_part: block partial sums (and their total) of fwi_vec_regularizer; allocated by its first call
    // sum_part: the same of fwi_vec_dot, fwi_dot and fwi_misfit_l2 (SUM_MAX_BLOCKS + 1 doubles); allocated by the first
    // of those calls
    void *smooth_tmp = nullptr, *reg_part = nullptr, *sum_part = nullptr;
    // the data misfits and fwi_residual_weight (Impl<T>::Misfit), each allocated by the first call that needs it: the
    // series between two passes (e; g1 of the envelope), the weights, the taps of B, the block partial sums of J (and
    // their total), the filtered synthetics s' and data d' of the misfits that filter first (with taps; s' later holds
    // their adjoint source), and the weights per trace of the misfits that take any (data_*)
    // fwi_misfit_matched (fwi_match.hip): the slices of the normal equations, G and b, the filter
    // fwi_misfit_envelope (fwi_envelope.hip): g2, the Hilbert taps
    // fwi_misfit_correlation (fwi_corr.hip): the per-tile sums and the terms of J, alpha / beta / rho
    // fwi_misfit_traveltime (fwi_ttime.hip): the partial correlations and the terms of J, tau and the three coefficients
    // of every trace, the picked lags
    // fwi_misfit_transport (fwi_ot.hip): densities, CDFs, potentials and every sum (ot_work_doubles), which traces count
    // fwi_misfit_spectral (fwi_spec.hip): the segment sums, G / phi / a and the terms of J, which pairs count, the
    // frequency weights, and the twiddle table with the (nt, frequencies) it was formed for (dt is the context's)
    Buf data_tmp{"data_tmp"}, data_w{"data_w"}, data_taps{"data_taps"}, data_part{"data_part"}, data_s{"data_s"},
        data_d{"data_d"}, data_tw{"data_tw"};
    Buf match_part{"match_part"}, match_norm{"match_norm"}, match_f{"match_f"};
    Buf env_g2{"env_g2"}, env_h{"env_h"};
    Buf corr_part{"corr_part"}, corr_coef{"corr_coef"};
    Buf tt_part{"tt_part"}, tt_coef{"tt_coef"}, tt_lag{"tt_lag"};
    Buf ot_work{"ot_work"}, ot_counts{"ot_counts"};
    Buf spec_part{"spec_part"}, spec_coef{"spec_coef"}, spec_counts{"spec_counts"}, spec_fw{"spec_fw"},
        spec_table{"spec_table"};
    // fwi_misfit_adaptive (fwi_awi.hip): the correlations of both kinds, z / the filters / W / the terms of J, which
    // traces count; the events around the three phases of the last call (created by the first), fwi_misfit_adaptive_ms
    Buf awi_part{"awi_part"}, awi_work{"awi_work"}, awi_counts{"awi_counts"};
    hipEvent_t awi_ev[4] = {nullptr, nullptr, nullptr, nullptr};
    bool have_awi_ms = false;
    // fwi_misfit_robust, fwi_residual_median (fwi_robust.hip): the per-tile sums of rho and the terms per trace, the
    // counts beyond the threshold likewise, the thresholds, the IRLS weight W = tw M^2 psi(e) of the last call that
    // kept one (have_irls: it belongs to the forward the context holds; fwi_residual_weight_robust), the medians with
    // their counts and the whole-gather select's bins
    Buf robust_part{"robust_part"}, robust_cnt{"robust_cnt"}, robust_thresh{"robust_thresh"}, robust_w{"robust_w"},
        robust_med{"robust_med"};
    bool have_irls = false;
    // fwi_eikonal*, fwi_vec_scatter_points, fwi_vec_gather_points (fwi_eikonal.hip): the compact indices and the values
    // of the point list of the running call, the gathered values, the change flags of a batch of launches
    Buf eik_idx{"eik_idx"}, eik_val{"eik_val"}, eik_out{"eik_out"}, eik_flags{"eik_flags"};
    int spec_table_nt = 0;
    std::vector<double> spec_table_freqs, spec_table_host;
    // off-grid receivers: where the per-POINT series of the device residual lie (the nodes' are in ctx->amp)
    enum { RESID_PTS_NONE = 0, RESID_PTS_A = 1, RESID_PTS_D = 2 };
    int resid_pts_in = RESID_PTS_NONE;
    void *pin = nullptr;     // pinned host staging for the time series
    size_t cap_pin = 0;
    // checkpointing (Plan::ckpt): q_store holds ckpt + 1 slots and fwd[] the recomputed fields
    bool ckpt_ready = false;  // every checkpoint buffer below is allocated
    void *snap = nullptr, *fwd[2] = {nullptr, nullptr};
    // temporal blocking (fused2d, pair3d): second buffer pair the kernel writes into
    void *fx[2] = {nullptr, nullptr};   // second pair for the time sweep in flight
    void *fwx[2] = {nullptr, nullptr};  // second pair for the checkpointed forward recomputation

    ncclComm_t comm = nullptr;
    int nranks = 1;

    std::string err;

    int fail(int code, const char *fmt, ...) {
        va_list ap;
        va_start(ap, fmt);
        err = vformat(fmt, ap);
        va_end(ap);
        return code;
    }
};

#define HIPCHK(ctx, call)                                                                     \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return (ctx)->fail(e_ == hipErrorOutOfMemory ? FWI_ENOMEM : FWI_EHIP, "%s: %s",   \
                               #call, hipGetErrorString(e_));                                 \
    } while (0)

#define DISPATCH(ctx, expr32, expr64) ((ctx)->cfg.dtype == FWI_F32 ? (expr32) : (expr64))
// ... of one member of Impl<float> or Impl<double>, with the argument list written once (the caller's arrays: typed(p))
#define DISPATCH_CALL(ctx, fn, ...) DISPATCH(ctx, Impl<float>::fn(ctx, __VA_ARGS__), Impl<double>::fn(ctx, __VA_ARGS__))

inline void *vec_slot(fwi_ctx *ctx, int32_t slot) {
    return (slot >= 0 && slot < (int32_t)ctx->vecs.size()) ? ctx->vecs[slot] : nullptr;
}

#define VEC_OR_FAIL(ctx, name, slot)                                                            \
    void *name = vec_slot(ctx, slot);                                                           \
    if (!name) return (ctx)->fail(FWI_EINVAL, "%s: vector slot %d does not exist", __func__, (int)(slot))

namespace fwi {

// What HIPCHK makes of a failed hipMalloc / hipFree, from the code fwi_ctx::mem returns for `member`
inline int dev_fail(fwi_ctx *ctx, const char *call, const char *member, int code) {
    if (code == DeviceMemory::UNKNOWN) return ctx->fail(FWI_EHIP, "%s(%s): not an allocation of this context", call, member);
    return ctx->fail(code == hipErrorOutOfMemory ? FWI_ENOMEM : FWI_EHIP, "%s(%s): %s", call, member,
                     hipGetErrorString((hipError_t)code));
}
// *slot := `bytes` of device memory, recorded as `member`[`index`]; *slot is null where it fails
inline int dev_acquire(fwi_ctx *ctx, void **slot, size_t bytes, const char *member, int index = 0) {
    const int code = ctx->mem.acquire(slot, bytes, member, index);
    return code ? dev_fail(ctx, "hipMalloc", member, code) : FWI_OK;
}
// ... and given back.  *slot is null BEFORE the runtime is asked, so a free it refuses leaves no pointer to memory that
// may be gone; a null *slot is a no-op
inline int dev_release(fwi_ctx *ctx, void **slot, const char *member) {
    const int code = ctx->mem.release(slot);
    return code ? dev_fail(ctx, "hipFree", member, code) : FWI_OK;
}
// a buffer of a fixed size that the first call which needs it allocates
inline int dev_first_use(fwi_ctx *ctx, void **slot, size_t bytes, const char *member) {
    return *slot ? FWI_OK : dev_acquire(ctx, slot, bytes, member);
}

// Defined in fwi_api.hip.  ensure: `b` holds at least `bytes` (its content is not kept when it grows)
int ensure(fwi_ctx *ctx, Buf &b, size_t bytes);
int upload_series(fwi_ctx *ctx, void *dst, const void *src, size_t bytes);
int sum_partials(fwi_ctx *ctx, double **part);
// ... host array (model-shaped) <-> compact device array, in the context's dtype T
template <typename T> int upload_compact(fwi_ctx *ctx, void *dst, const void *host);
template <typename T> int download_compact(fwi_ctx *ctx, void *host, const void *src);
extern template int upload_compact<float>(fwi_ctx *, void *, const void *);
extern template int upload_compact<double>(fwi_ctx *, void *, const void *);
extern template int download_compact<float>(fwi_ctx *, void *, const void *);
extern template int download_compact<double>(fwi_ctx *, void *, const void *);

// Defined in fwi_api_fourier.hip: the weights of one pass -> ctx->four_w; the checks the Fourier-store calls share
template <typename T>
int fourier_weights(fwi_ctx *ctx, const double *fw, const double *tau = nullptr, bool unit = false,
                    const double *taps = nullptr, int ntaps = 0);
extern template int fourier_weights<float>(fwi_ctx *, const double *, const double *, bool, const double *, int);
extern template int fourier_weights<double>(fwi_ctx *, const double *, const double *, bool, const double *, int);
int fourier_callable(fwi_ctx *ctx, const char *who, bool need_m);
int fourier_weight_args(fwi_ctx *ctx, const char *who, const double *fw, bool nonneg);
int fourier_axis(fwi_ctx *ctx, const char *who, int32_t axis, int *ax);
int fourier_tau_ok(fwi_ctx *ctx, const char *who, double tau, int l, bool phase);

}  // namespace fwi
