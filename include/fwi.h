/* fwi.h -- C ABI of the MI355X-native acoustic forward / adjoint / gradient engine.
 *
 * Drop-in boundary.  The reference (Kevin2599/full_waveform_inversion) has NO
 * plugin / operator / FFI interface and no wave-propagation code
 * (SURVEY.md s.0, s.8b): its only seams are plain Python functions called
 * positionally -- forward_model(green_func_array, M)
 * (full_waveform_inversion.py:253), compare_synth_to_real_waveforms(...)
 * (:584) and perform_monte_carlo_sampled_waveform_inversion(...) (:786).
 * The entry points below are therefore the ones BASELINE.json's north_star
 * names -- forward(model, src, rec), adjoint(residual), gradient() -- bound
 * from Python through ctypes (full_waveform_inversion_amd/_lib.py); each
 * declaration says which north_star item / SURVEY.md s.8(a-1) row it serves
 * and, where one exists, the nearest reference line.
 *
 * Conventions
 *  - Plain pointers and sizes only; no torch / numpy types.
 *  - Every function returns 0 on success or an FWI_E* code; the message is
 *    available from fwi_last_error().  The library never calls exit()
 *    (the reference print+sys.exit()s, full_waveform_inversion.py:124-125).
 *  - Host buffers are caller-owned, C-contiguous, x fastest: a model is
 *    (nz, nx) or (nz, ny, nx); time series are (nt, n).  Their element type is
 *    the context's dtype (float for FWI_F32, double for FWI_F64).
 *  - The library owns all device memory inside the context.  One context per
 *    GPU, used from one host thread at a time.  It is stateful: fwi_adjoint()
 *    consumes what the last fwi_forward(save=1) stored, fwi_gradient()
 *    returns what the adjoint calls since the last fwi_gradient_reset()
 *    accumulated (the sum over this rank's shots).
 *  - Grid indices are int32 triples/pairs (z[, y], x).
 */
#ifndef FWI_H
#define FWI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Stays 14 with the Born calls (fwi_born, fwi_born_vec, fwi_born_path; fwi_born_imaging, fwi_born_imaging_vec): they
 * are purely additive -- new symbols, fwi_config and every existing call unchanged -- so a client built against the
 * earlier 14 keeps working. */
/* ... and with the Fourier store (fwi_set_fourier_store, fwi_fourier_spectrum, fwi_store_bytes), additive in the same way. */
/* ... and with spectral imaging on it (fwi_adjoint_spectral, fwi_fourier_image, fwi_fourier_gradient[_vec],
 * fwi_fourier_adjoint_spectrum, fwi_fourier_illumination[_vec]). */
/* ... and with the extended images (fwi_fourier_offset_image[_vec], fwi_fourier_lag_image[_vec]). */
/* ... and with the tangent of the first-arrival traveltimes (fwi_eikonal_tangent). */
#define FWI_ABI_VERSION 14

enum { FWI_F32 = 0, FWI_F64 = 1 };

/* Stencil kernel selection (FWI_KERNEL_AUTO picks the fastest valid one). */
enum {
    FWI_KERNEL_AUTO = 0,
    FWI_KERNEL_POINT = 1,  /* one thread per grid point, neighbours through L1/L2 */
    FWI_KERNEL_STREAM = 2  /* 16-byte-per-lane kernels with LDS-staged halo tiles, any grid size: 3-D
                              z-marching register queue (step3d_stream, fp32 / fp64), 2-D fp32 row
                              tiles (step2d_tile) and 4-steps-per-launch tiles (step2d_fused) */
};

enum { FWI_WRT_VELOCITY = 0, FWI_WRT_SLOWNESS2 = 1 };
enum { FWI_UPDATE_STANDARD = 0, FWI_UPDATE_INCREMENT = 1 };
enum { FWI_ABC_SPONGE = 0, FWI_ABC_CPML = 1 };
enum { FWI_STORE_NATIVE = 0, FWI_STORE_BF16 = 1 };
enum { FWI_LAUNCH_AUTO = 0, FWI_LAUNCH_STREAM = 1, FWI_LAUNCH_GRAPH = 2 };

enum {
    FWI_OK = 0,
    FWI_EINVAL = 1,   /* bad argument / configuration */
    FWI_EHIP = 2,     /* a HIP runtime call failed */
    FWI_ESTATE = 3,   /* call order violated (e.g. adjoint before forward) */
    FWI_ENOMEM = 4,   /* device or host allocation failed */
    FWI_ECOMM = 5     /* RCCL failure */
};

typedef struct fwi_ctx fwi_ctx;

typedef struct fwi_config {
    int32_t struct_size; /* = sizeof(fwi_config); ABI guard */
    int32_t ndim;        /* 2 or 3 */
    int32_t nz, ny, nx;  /* ny is ignored (treated as 1) when ndim == 2 */
    int32_t order;       /* spatial order 2, 4 or 8 */
    int32_t nt_max;      /* largest number of time steps a shot will use */
    int32_t npml;        /* absorbing border width in cells; 0 = off */
    int32_t device;      /* HIP device ordinal */
    int32_t dtype;       /* FWI_F32 or FWI_F64 */
    int32_t kernel;      /* FWI_KERNEL_* */
    int32_t zchunk;      /* 3-D STREAM kernel: planes marched per workgroup; 0 = auto */
    int32_t ckpt_interval; /* 0: keep the imaging term of every step (nt_max x npts elements);
                              K > 0: snapshot the wavefields every K steps and recompute each
                              K-step forward segment during fwi_adjoint (one extra forward sweep,
                              ~(2 nt_max / K + K) x npts elements)  [SURVEY s.8f-3] */
    int32_t image_stride; /* 0 / 1: the imaging condition uses every time step (the exact discrete
                              gradient).  S > 1: the forward term is stored and correlated every S-th
                              step only, weighted by S (a Riemann sum over the oversampled time axis):
                              the store shrinks to ceil(nt_max / S) x npts elements and the adjoint
                              sweep skips the imaging traffic on the other steps.  Not combinable with
                              ckpt_interval. */
    int32_t update_form;  /* FWI_UPDATE_STANDARD: u' = A (2u - B u_prev + q).  FWI_UPDATE_INCREMENT: the same
                              recursion carried as (u, v = u - u_prev): v' = A (B v + q), u' = u + v'.  In fp32 the
                              round-off of the standard form is amplified by ~1 / (omega dt) (the cancellation in
                              2u - u_prev); the increment form rounds u' relative to u: ~4x smaller errors on
                              seismograms and gradient.  Kernels: 3-D stream (fp32; 20 instead of 16 B/update),
                              2-D fused (fp32; same traffic, the tile holds u twice, v and C) and the point kernel. */
    int32_t abc;          /* absorbing boundary of the npml border: FWI_ABC_SPONGE (damping factors A, B) or
                              FWI_ABC_CPML (convolutional PML: memory variables in the border only) */
    int32_t store_dtype;  /* forward-term store: FWI_STORE_NATIVE (the field type) or FWI_STORE_BF16 (fp32 contexts:
                              half the store and half its traffic; imaging error ~1e-3) */
    int32_t launch_mode;  /* How the launches of a sweep's time loop reach the GPU.  FWI_LAUNCH_STREAM: one by one on the
                              context's HIP stream, as they are formed.  FWI_LAUNCH_GRAPH: the whole time loop of a sweep
                              (every line / step / record launch of fwi_forward or fwi_adjoint) is captured into a hipGraph
                              and launched once -- same kernels, same arguments, same order, bit-identical results
                              (SURVEY s.7.2 "or capture the step loop in a hipGraph").  FWI_LAUNCH_AUTO (0, the default)
                              resolves to STREAM: measured on one context with the mode switched between sweeps
                              (profiles/r04_graph_probe.jsonl), the graph changes the loop time by -0.6 ... +1.4 % on every
                              configuration tried (2-D 256^2 ... 1024^2 with and without the CPML, 3-D 256^3 with one and
                              with two launches per step) and costs the host the same ~2.3 us per launch to build: a
                              recorded negative result, DESIGN.md s.4.  (was reserved0 up to ABI 11) */
    double h;            /* grid spacing (m) */
    double dt;           /* time step (s) */
    double sigma_max;    /* peak damping rate (1/s) of the absorbing border, >= 0 (used when npml > 0) */
    double pml_alpha_max; /* CPML only: peak of the frequency-shift profile alpha (1/s), ~ pi f0; 0 = plain PML */
} fwi_config;

/* Context life cycle.  [north_star: "thin ctypes C-ABI shim"; SURVEY s.8b] */
/* fwi_create reads FWI_PLACEMENT_TUNE from the environment (the placement of fwi_placement_info below): unset = the
 * search runs where the context is large enough; "0" = no padded allocations, no search; "pad" = padded allocations, no
 * search; "force" = the search also on grids below its size threshold; "fixed:<k0>,<k1>,..." = on any grid size and
 * WITHOUT a search, movable array i (search order of fwi_placement_info) sits k_i * 2 MiB into its padded allocation,
 * the last value repeating for the arrays not listed (tests: a layout that is asked for, not timed).  One to eight
 * values, each 0 ... 7; anything else makes fwi_create fail with FWI_EINVAL.  A context that places nothing (2-D, fp64,
 * the point kernel, the plain sponge in standard form) ignores "force" and "fixed:" alike. */
int fwi_create(const fwi_config *cfg, fwi_ctx **out);
/* Frees everything the context owns; every device array through the pointer its allocation returned, wherever the
 * placement left the array.  The function returns nothing: if the runtime refuses a free, the FIRST such failure is
 * written to the calling thread's creation-error text, the one fwi_last_error(NULL) returns, as
 * "fwi_destroy: hipFree(<member>[<index>]): <HIP error>", and the remaining arrays are still freed. */
void fwi_destroy(fwi_ctx *ctx);
/* Last error text of ctx.  With ctx == NULL: the calling thread's creation-error text -- the reason of the last failed
 * fwi_create, or a "fwi_destroy: ..." message (above).  A successful fwi_create on that thread clears it. */
const char *fwi_last_error(const fwi_ctx *ctx);
int fwi_abi_version(void);

/* Upload the velocity model c (m/s), model-shaped.  The `model` argument of
 * north_star's forward(model, src, rec).  [SURVEY s.8(a-1) row forward] */
int fwi_set_model(fwi_ctx *ctx, const void *c_host);

/* forward(model, src, rec): nt leapfrog steps of the 2-D/3-D O(2|4|8) stencil
 * with sponge update, injection of wavelet (nt, nsrc) at src_idx (nsrc, ndim)
 * and sampling at rec_idx (nrec, ndim) into seis_out (nt, nrec).  save != 0
 * keeps the per-step forward term the imaging condition needs.
 * [SURVEY s.8(a-1) rows forward / stencil / PML / source / receiver; the
 * structurally analogous reference slot is forward_model(),
 * full_waveform_inversion.py:253-264: unknowns -> synthetic seismograms] */
int fwi_forward(fwi_ctx *ctx, int32_t nt, int32_t nsrc, const int32_t *src_idx,
                const void *wavelet, int32_t nrec, const int32_t *rec_idx, int32_t save,
                void *seis_out);

/* forward() with OFF-GRID sources / receivers (multilinear interpolation onto the surrounding nodes).  The node
 * lists (src_idx / rec_idx, as for fwi_forward) hold every point's nodes contiguously: point p owns entries
 * pt_start[p] .. pt_start[p + 1] (at most 8 = 2^3; pt_start has npts + 1 entries), each with its interpolation
 * weight (context dtype).  Time series cross the boundary PER POINT -- wavelet (nt, nsrc_pts), seis_out
 * (nt, nrec_pts) -- and are scattered onto / gathered from the nodes on the device, the gather by a wave-level
 * __shfl_down reduction over each point's 8 lanes.  The following fwi_adjoint / fwi_misfit_l2 take and return
 * per-point series too.  npts = 0 with nodes = 0: no points of that kind.
 * [north_star "__shfl-based wavefront reductions for the receiver gather"; SURVEY s.8(a-1) row receiver sampling] */
int fwi_forward_spread(fwi_ctx *ctx, int32_t nt, int32_t nsrc_pts, int32_t nsrc_nodes, const int32_t *src_idx,
                       const int32_t *src_pt_start, const void *src_weight, const void *wavelet, int32_t nrec_pts,
                       int32_t nrec_nodes, const int32_t *rec_idx, const int32_t *rec_pt_start, const void *rec_weight,
                       int32_t save, void *seis_out);

/* A forward call that fails.  fwi_forward and fwi_forward_spread give up the shot before them as their first act, so
 * whatever they return an error for -- a refused argument (nt, a null buffer), a point outside the grid, a point set
 * with more than 8 nodes, a store that does not fit -- the context is left WITHOUT A FORWARD: fwi_adjoint,
 * fwi_adjoint_spectral, fwi_born*, every fwi_misfit_*, fwi_residual_weight and the fwi_fourier_* calls that need Q_k or
 * M_k return FWI_ESTATE until the next forward succeeds.  The model, the gradient and illumination accumulators, the
 * vectors, the launch mode and the Fourier settings are untouched.  (The point sets, the sizes and the series buffers
 * are replaced one by one on the way and a receiver is looked at after the sources are in place: a context that still
 * called the old shot its forward would sweep the new points with the old counts.)
 * The other calls that replace state need no such rule, each for its own reason.  fwi_adjoint and fwi_born* mark the
 * synthetics and the device residual as used up before their first launch and only read the store: after an error inside
 * the sweep the forward and its store are still those of the last fwi_forward, and the call may be repeated with a
 * residual of the caller's.  fwi_adjoint_spectral drops the M_k before it zeroes them.  fwi_set_fourier_store checks all
 * of its arguments before it touches anything, then forgets what the context stored (Q_k, M_k, the configured store)
 * BEFORE it frees the arrays: a free the runtime refuses leaves a context that says it has no store. */

/* adjoint(residual): reverse-time propagation of residual (nt, nrec) injected
 * at the receivers of the last forward.  image != 0 accumulates the zero-lag
 * forward x adjoint correlation into the gradient accumulator.  residual == NULL
 * back-propagates the residual fwi_misfit_l2() left on the device.  adj_src_out,
 * if not NULL, receives F^T residual as (nt, nsrc).
 * [SURVEY s.8(a-1) rows adjoint / imaging condition] */
int fwi_adjoint(fwi_ctx *ctx, const void *residual, int32_t image, void *adj_src_out);

/* Least-squares misfit on the device: with d_syn the seismograms of the last fwi_forward (still resident),
 * forms the residual r = d_syn - d_obs there, returns J = 1/2 sum r^2 (wave64 __shfl_down reduction, fp64
 * accumulate, block sums added in a fixed order: equal inputs give equal bits on every call) and keeps r as the residual of the next fwi_adjoint(ctx, NULL, ...): neither the residual nor a
 * second copy of the data crosses PCIe.  [SURVEY s.8(a-1) row "gradient dot-products / J"] */
int fwi_misfit_l2(fwi_ctx *ctx, const void *d_obs /* (nt, nrec) */, double *J_out);

/* Band-limited, weighted least squares on the device.  With x = d_syn - d_obs of the last fwi_forward, shaped (nt, ntr)
 * (ntr = nrec, or the receiver POINTS after fwi_forward_spread), B a symmetric FIR filter along time with the taps
 * b_0 .. b_R (b_-k = b_k) on the zero-extended trace,
 *     (B x)[n, j] = sum_{k = -R .. R} b_|k| x[n + k, j],   terms with n + k outside [0, nt) omitted   (so B^T = B),
 * and M per-sample weights >= 0 of the shape of the data (context dtype):
 *     e = M . (B x),     J = 1/2 sum e^2,     r = dJ/dd_syn = B (M . e).
 * taps == NULL (with R = 0): B = I;  weights == NULL: M = 1.  *J_out = J, and r stays on the device as the residual of
 * the next fwi_adjoint(ctx, NULL, ...): neither the synthetics nor the residual cross PCIe.  With off-grid receivers the
 * filter and the weights act per point and r is then spread onto the nodes, as fwi_misfit_l2 does.  The difference
 * d_syn - d_obs, the filter sums (over ascending k) and the weighting are fp64; e and r are each rounded to the
 * context's dtype once.  J is summed from the unrounded e in fp64 in a fixed order (block partial sums, no atomics):
 * equal inputs give equal bits.  With taps == NULL and weights == NULL the call is fwi_misfit_l2 with that fixed-order
 * sum: r is its residual bit for bit and J is summed, as there, from the squares of the residual as stored (rounded to
 * the context's dtype; in fp32 that J differs by some 1e-9 relative from the sum over the unrounded differences which
 * taps = {1.0} gives).  R may exceed nt - 1: the taps beyond meet no sample.  State rules of fwi_misfit_l2:
 * FWI_ESTATE without a forward or once an fwi_adjoint / fwi_born has run since.  FWI_EINVAL: a null J_out, a null d_obs
 * with nrec > 0, R < 0, R > 4096, null taps with R > 0.  Negative or non-finite weights and taps are NOT checked (the
 * weights would have to come back from the device): a negative weight acts as its absolute value, in J and in r.
 * The work buffers are the context's own (allocated by the first call, freed by fwi_destroy).  No reference counterpart. */
int fwi_misfit_weighted(fwi_ctx *ctx, const void *d_obs /* (nt, ntr) */, const void *weights /* (nt, ntr) or NULL */,
                        const double *taps /* R + 1, or NULL */, int32_t R, double *J_out);
/* The Gauss-Newton counterpart: residual := B M^2 B residual, in place on the residual that fwi_born / fwi_born_imaging
 * (or one of the misfit calls) left on the device, so that fwi_forward(save), fwi_born_imaging_vec, this call,
 * fwi_adjoint(NULL, image = 1), fwi_gradient_vec is H v = J^T B M^2 B J v.  Per node, or per point after
 * fwi_forward_spread (FWI_ESTATE when the per-point series of the residual were not kept).  Same arithmetic, arguments
 * and FWI_EINVAL cases as above; FWI_ESTATE without a residual on the device.  Synchronises the stream. */
int fwi_residual_weight(fwi_ctx *ctx, const void *weights /* (nt, ntr) or NULL */, const double *taps /* R + 1, or NULL */,
                        int32_t R);

/* Matching-filter (source-independent) misfit on the device: a short two-sided filter per shot takes up the unknown
 * source signature and is eliminated by variable projection.  With s = d_syn of the last forward and d = d_obs, both
 * (nt, ntr) as above, B and M as above, f = (f_-L .. f_L), K = 2 L + 1 coefficients stored f[k + L], acting along time
 * on the zero-extended trace:
 *     s' = B s,   d' = B d                                  (each rounded to the context's dtype once)
 *     (C_f x)[n, j]   = sum_{k = -L .. L} f_k x[n - k, j]      terms with n - k outside [0, nt) omitted
 *     (C_f^T y)[m, j] = sum_{k = -L .. L} f_k y[m + k, j]      terms with m + k outside [0, nt) omitted
 *     e = M . (C_f s' - d'),     Phi(f; s) = 1/2 sum e^2 + mu/2 |f|^2          (mu >= 0 absolute, the caller's)
 *     G[k, l] = sum_{n, j} M^2[n, j] s'[n - k, j] s'[n - l, j],     b[k] = sum_{n, j} M^2[n, j] s'[n - k, j] d'[n, j]
 *     f* = (G + mu I)^-1 b,     J(s) = Phi(f*; s),     r = dJ/ds = B C_f*^T (M . e)     (dPhi/df = 0 at f*)
 * G is not Toeplitz (the weights, the truncation at both ends of the trace) and is formed as defined.  mu does not
 * depend on s: one that did would add a term to the gradient.  f_in == NULL: f = f* is estimated (normal equations on
 * the device, fwi_match_solve on the host); otherwise f = f_in is used as given, and r is then dPhi/ds at that f.
 * *J_out = Phi(f; s); f_out, if not NULL, receives the K coefficients used; normal_out, if not NULL, receives G (K K
 * doubles, row-major, full, exactly symmetric, without mu) and then b (K doubles).  r stays on the device as the
 * residual of the next fwi_adjoint(ctx, NULL, ...).  L = 0, f_in = {1}, mu = 0 is fwi_misfit_weighted's e and r (bit for
 * bit without taps).  All sums are fp64 in a fixed order, without atomics: equal inputs give equal bits.  L may exceed
 * nt - 1: the shifts beyond meet no sample, and mu > 0 carries them.  State rules, off-grid receivers and work buffers as
 * fwi_misfit_weighted.  FWI_EINVAL: a null J_out, a null d_obs with nrec > 0, the tap errors of fwi_misfit_weighted,
 * L < 0, L > FWI_MATCH_LMAX, mu < 0 or not finite, a non-finite f_in entry, and a G + mu I that is not positive definite
 * (raise mu): then no residual is left on the device, the forward's synthetics remain and the call may be repeated.
 * No reference counterpart. */
#define FWI_MATCH_LMAX 64
int fwi_misfit_matched(fwi_ctx *ctx, const void *d_obs /* (nt, ntr) */, const void *weights /* (nt, ntr) or NULL */,
                       const double *taps /* R + 1, or NULL */, int32_t R, int32_t L, double mu,
                       const double *f_in /* 2L+1, or NULL: estimate */, double *f_out /* 2L+1, or NULL */,
                       double *normal_out /* K*K of G then K of b, or NULL */, double *J_out);
/* f_out := (G + mu I)^-1 b for a symmetric K x K matrix G (row-major; the upper triangle is read): fp64 Cholesky, then
 * forward and back substitution.  Pure host code: no context, no HIP call.  FWI_EINVAL: a null argument, K < 1,
 * K > 2 FWI_MATCH_LMAX + 1, mu < 0 or not finite, a pivot that is not positive and finite. */
int fwi_match_solve(const double *G /* K*K row-major */, const double *b, int32_t K, double mu, double *f_out);

/* Envelope misfit on the device: the envelope of a trace carries its low-frequency content even where its spectrum does
 * not, which widens the basin of attraction against cycle skipping.  With s = d_syn of the last forward and d = d_obs,
 * both (nt, ntr) as above, B and M as above, H the antisymmetric Hilbert FIR filter with one-sided taps h_1 .. h_Q,
 * stored hilbert[k - 1], acting along time on the zero-extended trace (H^T = -H exactly), power p in {1, 2}:
 *     s' = B s,   d' = B d                                       (each rounded to the context's dtype once, with taps)
 *     (H x)[n, j] = sum_{k = 1 .. Q} h_k (x[n - k, j] - x[n + k, j])     terms outside [0, nt) omitted
 *     E(x) = sqrt(x^2 + (H x)^2 + eps^2)                         eps absolute: it must not depend on s
 *     e = M . (E(s')^p - E(d')^p),     J = 1/2 sum e^2
 *     c = p . M . e . E(s')^(p - 2),   g1 = c . s',   g2 = c . (H s')      (each rounded to the context's dtype once)
 *     r = dJ/ds = B (g1 - H g2)                                  (g1 - H g2 rounded once; without taps it is r)
 * *J_out = J; r stays on the device as the residual of the next fwi_adjoint(ctx, NULL, ...).  Q may exceed nt - 1:
 * min(Q, nt - 1) taps are used.  Everything between the loads and the roundings named above is fp64; all sums run in a
 * fixed order, without atomics: equal inputs give equal bits.  State rules, off-grid receivers and work buffers as
 * fwi_misfit_weighted.  FWI_EINVAL: a null J_out, a null d_obs with nrec > 0, a null hilbert, the tap errors of
 * fwi_misfit_weighted, Q < 1, Q > 4096, a non-finite hilbert entry, power other than 1 or 2, eps < 0 or not finite,
 * eps == 0 with power 1 (E is not differentiable at 0).  No reference counterpart. */
int fwi_misfit_envelope(fwi_ctx *ctx, const void *d_obs /* (nt, ntr) */, const void *weights /* (nt, ntr) or NULL */,
                        const double *taps /* R + 1, or NULL */, int32_t R, const double *hilbert /* Q: h_1 .. h_Q */,
                        int32_t Q, int32_t power, double eps, double *J_out);

/* Trace-normalised zero-lag correlation misfit on the device (Choi & Alkhalifah 2012): every misfit above is a difference
 * of amplitudes; this one reads phase only and ignores the gain of every trace, which a constant-density acoustic engine
 * cannot model on field data.  With s = d_syn of the last forward and d = d_obs, both (nt, ntr) as above, B and M as
 * above, w_j >= 0 optional weights per trace (NULL: 1) and eps >= 0 an absolute floor that must not depend on s:
 *     s' = B s,  d' = B d            (rounded to the context's dtype once, only when taps are given)
 *     sh = M . s',  dh = M . d'
 *     a_j = sum_n sh[n,j]^2    b_j = sum_n dh[n,j]^2    c_j = sum_n sh[n,j] dh[n,j]
 *     ns_j = sqrt(a_j + eps^2)  nd_j = sqrt(b_j + eps^2)   rho_j = c_j / (ns_j nd_j)
 *     trace j counts iff  b_j > 0 and a_j + eps^2 > 0;  otherwise J_j = 0, rho_j = 0 and its adjoint source is 0
 *     J = sum_j w_j (1 - rho_j)
 *     alpha_j = -w_j / (ns_j nd_j)     beta_j = c_j / ns_j^2
 *     g = M . alpha_j (dh - beta_j sh)           (rounded to the dtype once)
 *     r = dJ/ds = B g
 * A scale per trace inside M cancels: w is the only way to down-weight a trace.  *J_out = J (the sum itself, not half of
 * it); rho_out, if not NULL, receives the ntr values rho_j; r stays on the device as the residual of the next
 * fwi_adjoint(ctx, NULL, ...).  The synthetics are left alone: the call can be repeated.  Everything between the loads
 * and the roundings named above is fp64; a thread adds its 8 consecutive times in ascending order, a block its four
 * waves in wave order, a trace its time tiles in ascending order and J its traces in a fixed order, without atomics:
 * equal inputs give equal bits.  State rules, off-grid receivers (ntr is then the number of points) and work buffers as
 * fwi_misfit_weighted.  FWI_EINVAL: a null J_out, a null d_obs with nrec > 0, the tap errors of fwi_misfit_weighted,
 * eps < 0 or not finite, a trace weight that is negative or not finite.  The reference's CC measure (Pearson correlation
 * per trace, averaged) is J / ntr at eps = 0, M = 1, B = I on mean-free traces. */
int fwi_misfit_correlation(fwi_ctx *ctx, const void *d_obs /* (nt, ntr) */, const void *weights /* (nt, ntr) or NULL */,
                           const double *taps /* R + 1, or NULL */, int32_t R,
                           const double *trace_weights /* ntr, or NULL */, double eps, double *J_out,
                           double *rho_out /* ntr, or NULL */);

/* Cross-correlation traveltime misfit on the device (Luo & Schuster 1991; the traveltime adjoint source of Tromp et al.
 * 2005): every misfit above compares the data at zero lag; this one measures HOW LATE each trace is, grows with the
 * square of the time shift however many periods the shift spans, and ignores the gain of every trace.  With s = d_syn of
 * the last forward and d = d_obs, both (nt, ntr) as above, B and M as above, w_j >= 0 optional weights per trace (NULL:
 * 1), K = max_lag >= 1 in samples, Ke = min(K, nt - 1) and dt the context's time step:
 *     s' = B s,  d' = B d            (rounded to the context's dtype once, only when taps are given)
 *     sh = M . s',  dh = M . d'
 *     c_j(k) = sum_n sh[n + k, j] dh[n, j],   k = -Ke .. Ke       (terms with n + k outside [0, nt) omitted)
 *     k*_j = the smallest k with c_j(k) = max_k c_j(k)
 *     c-, c0, c+ = c_j(k* - 1), c_j(k*), c_j(k* + 1);   N = c- - c+,   Q = c- - 2 c0 + c+
 *     trace j counts iff  |k*| < Ke, c0 > 0 and Q < 0;  otherwise tau_j = 0, J_j = 0 and its adjoint source is 0
 *     delta_j = N / (2 Q) in [-1/2, 1/2],   tau_j = (k* + delta_j) dt,   J = 1/2 sum_j w_j tau_j^2     (s^2)
 *     D- = (Q - N) / (2 Q^2),  D0 = N / Q^2,  D+ = (-Q - N) / (2 Q^2)
 *     g[m, j] = M[m, j] w_j tau_j dt (D- dh[m - k* + 1, j] + D0 dh[m - k*, j] + D+ dh[m - k* - 1, j])
 *     r = dJ/ds = B g                (g rounded to the dtype once; rows outside [0, nt) contribute 0)
 * tau > 0: the synthetics arrive late (for s(t) = d(t - tau), c peaks at +tau).  A dead trace has c = 0 everywhere, picks
 * k* = -Ke and does not count; neither does a trace whose shift lies beyond the window (|k*| = Ke).  r is the exact
 * gradient of this discrete J (the picked lag is locally constant, c is linear in sh).  J is NOT differentiable where a
 * trace starts or stops counting; tau is continuous where k* moves between neighbouring lags.  *J_out = J; tau_out, if
 * not NULL, receives the ntr delays in seconds (0 where a trace does not count), lag_out, if not NULL, the ntr picked
 * lags k* (counting or not); r stays on the device as the residual of the next fwi_adjoint(ctx, NULL, ...).  The
 * synthetics are left alone: the call can be repeated.  Everything between the loads and the roundings named above is
 * fp64; c_j(k) is added by fma over ascending time within a time slice and over the slices in ascending order, the
 * number of slices a function of (nt, ntr, Ke) only, the lags are scanned in ascending order and J adds its traces in a
 * fixed order, without atomics: equal inputs give equal bits.  State rules, off-grid receivers (ntr is then the number of
 * points) and work buffers as fwi_misfit_weighted.  FWI_EINVAL: a null J_out, a null d_obs with nrec > 0, the tap errors
 * of fwi_misfit_weighted, max_lag < 1 or > FWI_TT_KMAX, a trace weight that is negative or not finite.  No receivers:
 * J = 0 and nothing is launched; nt = 1: Ke = 0, no trace counts, J = 0 and r = 0. */
#define FWI_TT_KMAX 1024
int fwi_misfit_traveltime(fwi_ctx *ctx, const void *d_obs /* (nt, ntr) */, const void *weights /* (nt, ntr) or NULL */,
                          const double *taps /* R + 1, or NULL */, int32_t R,
                          const double *trace_weights /* ntr, or NULL */, int32_t max_lag, double *J_out,
                          double *tau_out /* ntr, or NULL */, int32_t *lag_out /* ntr, or NULL: k*, counting or not */);

/* Trace-by-trace optimal-transport (quadratic Wasserstein, W2) misfit on the device (Engquist & Froese 2014; Yang,
 * Engquist, Sun & Hamfeldt 2018): the envelope widens the basin of attraction by dropping the phase, the traveltime
 * misfit by reducing a trace to one pick; this one compares the whole traces as densities along time, needs no pick and
 * no window, and grows with the square of a time shift however many periods the shift spans.  With s = d_syn of the last
 * forward and d = d_obs, both (nt, ntr) as above, B, M and w_j exactly as in fwi_misfit_traveltime, dt the context's time
 * step and P the positivisation below, per trace j:
 *     s' = B s,  d' = B d            (rounded to the context's dtype once, only when taps are given)
 *     sh = M . s',  dh = M . d'
 *     p_n = P(sh[n,j]),  q_n = P(dh[n,j])
 *     S_s = sum_n p_n,  S_d = sum_n q_n;   f_n = p_n / S_s,  g_n = q_n / S_d
 *     F_n = sum_{i<=n} f_i,  G_n = sum_{i<=n} g_i                 n = 0 .. nt-1
 *     for n = 1 .. nt-1, with the level y = F_{n-1}:
 *         m+(n) = min(#{m : G_m <= y}, nt-1),   m-(n) = min(#{m : G_m < y}, nt-1)
 *         a_n = 2n - 1 - m+(n) - m-(n)                            an integer
 *       and the same with f and g exchanged: n+(m), n-(m), b_m = 2m - 1 - n+(m) - n-(m)
 *     phi_0 = psi_0 = 0,  phi_n = sum_{i=1..n} a_i,  psi_m = sum_{i=1..m} b_i      integers, exact
 *     W_j = dt^2 (sum_n phi_n f_n + sum_m psi_m g_m)              (s^2)
 *     J = 1/2 sum_j w_j W_j
 *     phibar_j = sum_n phi_n f_n
 *     g[n,j] = M[n,j] (w_j / 2) dt^2 (phi_n - phibar_j) / S_s  P'(sh[n,j])     (rounded to the dtype once)
 *     r = dJ/ds = B g
 * W_j is the exact squared 2-Wasserstein distance between the atomic measures sum f_n delta(t_n) and sum g_n delta(t_n),
 * (phi, psi) dt^2 an optimal pair of Kantorovich potentials, and r the gradient of this discrete J wherever no level F_n
 * equals a level G_m.  J is piecewise smooth and NOT differentiable where a level of F crosses a level of G: the gradient
 * jumps there.  At a tie the two-sided count m+ + m- selects the midpoint subgradient, so that d_obs == d_syn gives
 * phi = psi = 0, J = 0 and r = 0 exactly.  Zero-mass atoms are allowed (they are ties).
 * transform and param (absolute; like eps elsewhere param must not depend on s):
 *     FWI_OT_LINEAR    P(x) = x + c,  P' = 1,  c = param > 0
 *     FWI_OT_SOFTPLUS  P(x) = log(1 + exp(b x)) / b,  P'(x) = 1 / (1 + exp(-b x)),  b = param > 0; evaluated as
 *                      (max(b x, 0) + log1p(exp(-|b x|))) / b, the sigmoid by the branch of the sign of x: no overflow
 * A trace counts iff every p_n and q_n is finite and >= 0 and S_s, S_d are finite and > 0; otherwise W_j = 0, its term of
 * J is 0 and its adjoint source is 0 (under FWI_OT_LINEAR a trace that goes below -c drops out; softplus only fails on
 * non-finite data).  *J_out = J; w2_out, if not NULL, receives the ntr values W_j in s^2, counts_out, if not NULL, 1 for
 * a trace that counts and 0 otherwise; r stays on the device as the residual of the next fwi_adjoint(ctx, NULL, ...).
 * The synthetics are left alone: the call can be repeated.  Everything between the loads and the roundings named above is
 * fp64, the potentials integers carried in fp64.  The time axis is cut into slices whose number is a function of
 * (nt, ntr) only; S, the CDFs (as (offset of the slice + sum within the slice) / S, non-decreasing by construction), the
 * potentials and the two dual sums are added over ascending time within a slice and over the slices in ascending order,
 * and J adds its traces in a fixed order, without atomics: equal inputs give equal bits.  State rules, off-grid receivers
 * (ntr is then the number of points) and work buffers as fwi_misfit_weighted.  FWI_EINVAL: a null J_out, a null d_obs
 * with nrec > 0, the tap errors of fwi_misfit_weighted, an unknown transform, param <= 0 or not finite, a trace weight
 * that is negative or not finite.  No receivers: J = 0 and nothing is launched; nt = 1: W = 0 and r = 0. */
#define FWI_OT_LINEAR 0
#define FWI_OT_SOFTPLUS 1
int fwi_misfit_transport(fwi_ctx *ctx, const void *d_obs /* (nt, ntr) */, const void *weights /* (nt, ntr) or NULL */,
                         const double *taps /* R + 1, or NULL */, int32_t R,
                         const double *trace_weights /* ntr, or NULL */, int32_t transform, double param, double *J_out,
                         double *w2_out /* ntr, or NULL: W_j in s^2 */, int32_t *counts_out /* ntr, or NULL: 1 / 0 */);

/* Adaptive (per-trace matching-filter) misfit on the device (adaptive waveform inversion; Warner & Guasch 2016): the
 * envelope drops the phase, the correlation the amplitude, the traveltime misfit reduces a trace to one pick, W2 needs a
 * positivisation and fwi_misfit_matched estimates one filter per shot.  This one designs one Wiener filter per TRACE that
 * turns the observed trace into the synthetic one and penalises the filter's energy away from zero lag, normalised by
 * its energy: no pick and no window, amplitude and phase are kept, it grows with the square of a time shift up to the
 * filter's half-length, and a gain per trace cancels exactly.  With s = d_syn of the last forward and d = d_obs, both
 * (nt, ntr) as above, B, M and the per-trace weights tw_j exactly as in fwi_misfit_traveltime, L >= 1 the half-length in
 * samples, K = 2 L + 1 coefficients w_k, k = -L .. L, stored at w[k + L], dt the context's time step and lam > 0 a
 * relative ridge, per trace j, every trace zero-extended outside [0, nt):
 *     s' = B s,  d' = B d            (rounded to the context's dtype once, only when taps are given)
 *     sh = M . s',  dh = M . d'
 *     a_j(m) = sum_n dh[n, j] dh[n + m, j]            m = 0 .. 2 L   (0 once m > nt - 1)
 *     c_j(k) = sum_n sh[n + k, j] dh[n, j]            k = -L .. L    (= sum_n dh[n - k, j] sh[n, j])
 *     G_j[k, l] = a_j(|k - l|) + lam a_j(0) [k == l]  exactly Toeplitz: the fit runs over the whole convolution output
 *     w_j = G_j^-1 c_j                                the filter with  w * dh ~= sh,  linear in s
 *     N_j = sum_k w_k^2
 *     W_j = sum_k (k dt)^2 w_k^2 / N_j                (s^2)
 *     J   = 1/2 sum_j tw_j W_j
 *     y_k = tw_j w_k ((k dt)^2 - W_j) / N_j
 *     z_j = G_j^-1 y_j
 *     g[n, j] = M[n, j] sum_k z_k dh[n - k, j]        (rounded to the dtype once)
 *     r = dJ/ds = B g
 * G_j depends on the data only: a ridge relative to a_j(0) adds no term to the gradient, and r is the exact gradient of
 * this discrete J.  A trace counts iff a_j(0) is finite and > 0, every Cholesky pivot of G_j is finite and > 0 and N_j is
 * finite and > 0 (a dead synthetic trace gives w = 0 and does not count); for a trace that does not count W_j = 0, its
 * term of J, its filter and its adjoint source are 0.  W_j <= (L dt)^2.  A gain on a synthetic trace cancels.  L may
 * exceed nt - 1 (the lags beyond nt - 1 are 0).  d_obs == d_syn does NOT give J = 0: it gives the second moment of
 * G^-1 a, a band-limited delta whose width the ridge and the bandwidth of the data set, and a non-zero r; sqrt(W) is
 * that width, the floor below which a shift cannot be read.  J is NOT differentiable where a trace starts or stops
 * counting.  *J_out = J; w2_out, if not NULL, receives the ntr values W_j in s^2, counts_out, if not NULL, 1 for a trace
 * that counts and 0 otherwise, filters_out, if not NULL, the filters w_j as (ntr, 2 L + 1); r stays on the device as the
 * residual of the next fwi_adjoint(ctx, NULL, ...).  The synthetics are left alone: the call can be repeated.
 * Everything between the loads and the roundings named above is fp64.  a_j and c_j are added by fma over ascending time
 * within a time slice and over the slices in ascending order, the number of slices a function of (nt, ntr, L) only; the
 * systems are solved by Cholesky, one workgroup per trace: every entry of the factor takes its terms by fma over
 * ascending index, the forward substitutions take theirs over ascending, the back substitutions over descending index,
 * N_j and the moment are added over ascending k, g by fma over ascending k, and J adds its traces in a fixed order,
 * without atomics: equal inputs give equal bits.  State rules, off-grid receivers (ntr is then the number of points) and
 * work buffers as fwi_misfit_weighted.  FWI_EINVAL: a null J_out, a null d_obs with nrec > 0, the tap errors of
 * fwi_misfit_weighted, L < 1 or > FWI_AWI_LMAX, lam <= 0 or not finite, a trace weight that is negative or not finite.
 * No receivers: J = 0 and nothing is launched. */
#define FWI_AWI_LMAX 64
int fwi_misfit_adaptive(fwi_ctx *ctx, const void *d_obs /* (nt, ntr) */, const void *weights /* (nt, ntr) or NULL */,
                        const double *taps /* R + 1, or NULL */, int32_t R,
                        const double *trace_weights /* ntr, or NULL */, int32_t L, double lam, double *J_out,
                        double *w2_out /* ntr, or NULL: W_j in s^2 */, int32_t *counts_out /* ntr, or NULL: 1 / 0 */,
                        double *filters_out /* (ntr, 2 L + 1), or NULL: w_j */);

/* The device times in milliseconds of the three phases of the last fwi_misfit_adaptive call on this context, from HIP
 * events on its stream: ms_out[0] the lag correlations a_j and c_j, ms_out[1] the per-trace solves with the sum of J,
 * ms_out[2] the adjoint source g (B g and the scatter onto the nodes are not included).  Waits for that call's kernels.
 * FWI_ESTATE before the first such call with receivers; FWI_EINVAL: a null ms_out. */
int fwi_misfit_adaptive_ms(fwi_ctx *ctx, double *ms_out /* 3 */);

/* Robust (M-estimator) data misfits on the device: Huber, the hybrid L1/L2 norm and Cauchy.  Every misfit above is
 * quadratic in what it compares, or a ratio of quadratic sums, so a few spiky traces or a noise burst dominate J and the
 * adjoint source; these grow linearly (huber, hybrid) or logarithmically (cauchy) beyond a threshold.  With s = d_syn of
 * the last forward and d = d_obs, both (nt, ntr), B and M of fwi_misfit_weighted, tw_j >= 0 weights per trace and
 * a_j > 0 a THRESHOLD per trace in the units of the data, the residual amplitude at which the norm leaves least squares
 * (a caller forms it as a_j = c sigma_j from a scale estimate sigma_j, e.g. 1.4826 times fwi_residual_median's; only a_j
 * crosses this boundary):
 *     e = M . B (s - d)                    (fp64, rounded to the context's dtype once, as fwi_misfit_weighted's e)
 *     v = (e / a_j)^2
 *     huber :  rho = e^2 / 2 if |e| <= a_j,  a_j |e| - a_j^2 / 2 otherwise          psi = min(1, a_j / |e|)  (1 at e = 0)
 *     hybrid:  rho = e^2 / (1 + sqrt(1 + v))   (= a^2 (sqrt(1 + v) - 1), written without cancellation)
 *                                                                                  psi = 1 / sqrt(1 + v)
 *     cauchy:  rho = (a_j^2 / 2) log1p(v)                                           psi = 1 / (1 + v)
 *     J = sum_j tw_j sum_n rho[n, j]        g = tw_j psi e        r = dJ/ds = B (M . g)
 * d_obs == d_syn gives J = 0 and r = 0 exactly, for every kind.  |d(psi e)/de| <= 1 for the three kinds; huber is C^1
 * and the other two are smooth, so there is no non-differentiable set.  Cauchy's d(psi e)/de reaches -1/8 at v = 3:
 * CAUCHY IS NOT CONVEX in e.  Huber alone takes a_j = +inf: then psi = 1, and with tw = 1 r is fwi_misfit_weighted's r
 * bit for bit and J is its J (the same bits where that J is summed from e as stored: an fp64 context, or neither taps
 * nor weights; otherwise fwi_misfit_weighted sums the unrounded e and the two differ by the rounding of e).  a_j MUST
 * NOT DEPEND ON s: a threshold that did would add a term to the gradient (the rule of mu in fwi_misfit_matched).
 * All arithmetic is fp64; g is rounded to the dtype once.  J is summed from the unrounded terms in a fixed order (a
 * thread's 8 consecutive times ascending, the block's 256 threads by a halving tree, the blocks in a fixed order: the
 * order of fwi_misfit_weighted), no floating-point atomics: equal inputs give equal bits.  *J_out = J; J_trace_out, if
 * not NULL, receives the ntr terms tw_j sum_n rho[n, j] (per trace: tiles of 32 times ascending; their sum is J to
 * round-off, not to the bit), nout_out, if not NULL, the number of samples of every trace with |e| > a_j.
 * keep_irls != 0 keeps W = tw_j M^2 psi(e), rounded to the dtype, in a buffer of the context for
 * fwi_residual_weight_robust.  r stays on the device as the residual of the next fwi_adjoint(ctx, NULL, ...).  State
 * rules, off-grid receivers (per point, then scattered), work buffers and the taps / weights errors as
 * fwi_misfit_weighted.  FWI_EINVAL, checked on the host before anything is uploaded: an unknown kind, null thresholds
 * with nrec > 0, a threshold that is <= 0 or NaN, or +inf for a kind other than huber, a trace weight that is negative or
 * not finite.  No reference counterpart. */
#define FWI_ROBUST_HUBER 0
#define FWI_ROBUST_HYBRID 1
#define FWI_ROBUST_CAUCHY 2
int fwi_misfit_robust(fwi_ctx *ctx, const void *d_obs /* (nt, ntr) */, const void *weights /* (nt, ntr) or NULL */,
                      const double *taps /* R + 1, or NULL */, int32_t R, int32_t kind,
                      const double *thresh /* ntr: a_j */, const double *trace_weights /* ntr, or NULL */,
                      int32_t keep_irls, double *J_trace_out /* ntr, or NULL */,
                      int32_t *nout_out /* ntr, or NULL: samples with |e| > a_j */, double *J_out);
/* The IRLS (majoriser) Gauss-Newton weight of fwi_misfit_robust: residual := B (W . (B residual)) with the W the last
 * fwi_misfit_robust(keep_irls) on this forward kept, in place on the residual fwi_born / fwi_born_imaging left on the
 * device, so that fwi_forward(save), fwi_misfit_robust(keep_irls), fwi_born_imaging, this call, fwi_adjoint(NULL,
 * image = 1) is H v = J^T B W B J v.  W >= 0, so H is positive semi-definite for every kind, cauchy included: that is
 * why psi is used and not rho''.  Two filter passes as fwi_residual_weight.  FWI_ESTATE when no W is held (none kept;
 * the first thing a forward call does is to drop it with the shot before; fwi_destroy frees it) or when no residual is
 * on the device; FWI_EINVAL: the tap errors of fwi_misfit_weighted.  Synchronises the stream. */
int fwi_residual_weight_robust(fwi_ctx *ctx, const double *taps /* R + 1, or NULL */, int32_t R);
/* The lower median of |e|, e as above, on the device: the scale estimate behind a threshold.  segment 0: per trace
 * (ntr values), 1: of the whole gather (one value).  The samples that count are all of them with weights == NULL, and
 * those with M[n, j] > 0 otherwise; count_out receives their number per segment and med_out the order statistic
 * (count - 1) / 2, 0-based, in ascending order of the bit patterns of |e| in the context's dtype with the sign bit
 * cleared: +inf and NaN sort last, as np.sort puts them, without a special case (the pass that forms e multiplies the 8
 * times of an aligned group by zero taps, so one non-finite sample of the data makes the e of its group non-finite).
 * count == 0 gives med = 0.  An exact
 * order statistic (a radix select, most significant digit first, integer atomics only): the same on every call, no
 * tolerance.  It leaves NO residual on the device (whatever was there is gone) and keeps the synthetics, so that a misfit
 * call can follow on the same forward.  State rules, off-grid receivers and tap errors as fwi_misfit_weighted; FWI_EINVAL
 * also for a null output or a segment that is neither 0 nor 1; a whole gather of more than 2^32 - 1 samples is refused
 * (FWI_EHIP). */
int fwi_residual_median(fwi_ctx *ctx, const void *d_obs /* (nt, ntr) */, const void *weights /* (nt, ntr) or NULL */,
                        const double *taps /* R + 1, or NULL */, int32_t R, int32_t segment,
                        double *med_out /* ntr, or 1 */, int64_t *count_out /* ntr, or 1 */);

/* Frequency-domain (spectral) data misfit on the device: every misfit above compares traces in the time domain; this
 * one compares their discrete Fourier coefficients at F frequencies of the caller's choice, amplitude and phase together
 * or apart (the logarithmic and phase-only misfits of Shin & Min 2006 and Bednar, Shin & Pyun 2007), with a weight per
 * frequency.  It is the data side of frequency-domain FWI from time-domain modelling, whose model side is
 * fwi_set_fourier_store.  With s = d_syn of the last forward and d = d_obs, both (nt, ntr) as above:
 *     sh = M . B d_syn,  dh = M . B d_obs    M (per-sample weights, or none) and B (taps, or none) exactly as in
 *                                            fwi_misfit_correlation; B s and B d are rounded to the context's dtype once,
 *                                            only when taps are given; ntr is the number of receivers, or of receiver
 *                                            points after fwi_forward_spread
 *     theta_kn = 2 pi frac(f_k n dt)         formed on the host in fp64 from the fractional part, as the table of
 *                                            fwi_set_fourier_store is; f_k: the F frequencies in Hz
 *     S_kj = sum_n sh[n,j] (cos theta_kn - i sin theta_kn)        O_kj likewise from dh
 *     w_kj = fw_k * tw_j                     fw: F weights per frequency (NULL: 1), tw: ntr weights per trace (NULL: 1),
 *                                            all finite and >= 0
 *     kind L2      J = 1/2 sum_kj w_kj |S_kj - O_kj|^2                         G_kj = w_kj (S_kj - O_kj)
 *     kind LOGAMP  a_kj = 1/2 ln((|S_kj|^2 + eps^2) / (|O_kj|^2 + eps^2))
 *                  J = 1/2 sum w a^2                                            G_kj = w_kj a_kj S_kj / (|S_kj|^2 + eps^2)
 *     kind PHASE   phi_kj = atan2(Im(S_kj conj O_kj), Re(S_kj conj O_kj)) in (-pi, pi]
 *                  J = 1/2 sum w phi^2                                          G_kj = w_kj phi_kj (i S_kj) / |S_kj|^2
 *     kind LOG     the sum of LOGAMP and PHASE (the logarithmic misfit), over the pairs that count under PHASE
 *     g[n,j] = M[n,j] sum_k (Re G_kj cos theta_kn - Im G_kj sin theta_kn)      (rounded to the dtype once)
 *     r = dJ/ds = B g                        the residual of the next fwi_adjoint(ctx, NULL, ...)
 * Which pairs count: under PHASE and LOG a pair (k, j) counts iff |S_kj|^2 > eps^2 and |O_kj|^2 > eps^2; otherwise its
 * term of J and its G are 0.  Under L2 and LOGAMP every pair counts (LOGAMP with eps = 0 is then infinite where a
 * coefficient vanishes: give it a floor).  eps >= 0 is in the units of |S| and, like every floor above, must not depend
 * on s.  Im(S conj O) = S_i O_r - S_r O_i is formed from two rounded products, never a fused one: equal gathers give
 * J = 0 and a zero adjoint source exactly, for every kind.  PHASE is exactly invariant under a gain on the synthetics.
 * J is NOT differentiable where phi = +-pi (a cycle skip at that frequency) nor where a pair starts or stops counting,
 * and phi wraps: a time shift beyond half a period of f_k reads as a smaller one of the other sign.  Per-frequency
 * weights whiten the spectrum; an exponential damping exp(-sigma n dt) inside M gives the Laplace-Fourier misfit.
 * *J_out = J.  The three optional outputs are (F, ntr), frequency the slow axis: phase_out receives phi_kj wherever the
 * pair passes the counting rule of PHASE (whatever the kind) and 0 elsewhere; logamp_out receives a_kj wherever the kind
 * uses it or the pair passes that rule and 0 elsewhere; counts_out 1 for a pair that counts under `kind` and 0 otherwise.
 * The synthetics are left alone: the call can be repeated.  Everything between the loads and the roundings named above
 * is fp64: a thread adds its 16 consecutive times by fma in ascending order, a block its 16 waves in wave order, a pair
 * its time segments of 256 rows in ascending order, the source its frequencies by fma in ascending order and J its terms
 * in a fixed order, without atomics: equal inputs give equal bits.  The table of twiddles is kept on the context and
 * rebuilt only when nt or the frequencies change.  State rules, off-grid receivers and work buffers as
 * fwi_misfit_weighted.  FWI_EINVAL, with the reason in the message: a null J_out, a null d_obs with nrec > 0, the tap
 * errors of fwi_misfit_weighted, nfreq outside [1, FWI_FOURIER_FMAX], null frequencies, a frequency that is negative, not
 * finite, equal to another or above 1 / (2 dt); under PHASE or LOG a frequency of 0 or within 1e-9 (relative) of
 * 1 / (2 dt), where S is real; an unknown kind; eps or a weight that is negative or not finite.  No receivers: J = 0,
 * the outputs are zeros and nothing is launched. */
enum { FWI_SPEC_L2 = 0, FWI_SPEC_PHASE = 1, FWI_SPEC_LOGAMP = 2, FWI_SPEC_LOG = 3 };
int fwi_misfit_spectral(fwi_ctx *ctx, const void *d_obs /* (nt, ntr) */, const void *weights /* (nt, ntr) or NULL */,
                        const double *taps /* R + 1, or NULL */, int32_t R, int32_t nfreq,
                        const double *freqs_hz /* nfreq */, int32_t kind, double eps,
                        const double *freq_weights /* nfreq, or NULL */, const double *trace_weights /* ntr, or NULL */,
                        double *J_out, double *phase_out /* (F, ntr) or NULL */, double *logamp_out /* (F, ntr) or NULL */,
                        uint8_t *counts_out /* (F, ntr) or NULL */);

/* gradient(): copy out the accumulated gradient, model-shaped, as dJ/dc
 * (FWI_WRT_VELOCITY) or dJ/d(1/c^2) (FWI_WRT_SLOWNESS2).
 * [SURVEY s.8(a-1) row gradient] */
int fwi_gradient(fwi_ctx *ctx, int32_t wrt, void *g_out);
int fwi_gradient_reset(fwi_ctx *ctx);
/* dst accumulator += src accumulator (two contexts of the same shape on the same GPU): several
 * contexts can work through a rank's shots concurrently -- a 2-D shot cannot fill an MI355X on
 * its own -- and are summed on the device before the exchange. */
int fwi_gradient_add(fwi_ctx *dst, fwi_ctx *src);

/* Device-side reductions for the misfit and the optimiser's dot products:
 * sum_i a[i]*b[i] over n host elements of the context dtype, wave-shuffle
 * reduced on the GPU, fp64 accumulate, in a fixed order without floating-point atomics: equal inputs give equal
 * bits on every call, context and rank (fwi_vec_dot and fwi_misfit_l2 alike).  [SURVEY s.8(a-1) row dot-products] */
int fwi_dot(fwi_ctx *ctx, const void *a_host, const void *b_host, int64_t n, double *out);

/* Device-resident, model-shaped vectors for the optimiser (L-BFGS history, search direction,
 * trial model): `count` slots owned by the context; all algebra runs on the GPU so an iteration
 * moves no model-sized array over PCIe.  [SURVEY s.8(a-1) rows L-BFGS / dot-products] */
int fwi_vec_create(fwi_ctx *ctx, int32_t count);
int fwi_vec_upload(fwi_ctx *ctx, int32_t slot, const void *host);
int fwi_vec_download(fwi_ctx *ctx, int32_t slot, void *host);
int fwi_vec_copy(fwi_ctx *ctx, int32_t dst, int32_t src);
int fwi_vec_axpby(fwi_ctx *ctx, int32_t y, double a, int32_t x, double b); /* y = a x + b y */
int fwi_vec_dot(fwi_ctx *ctx, int32_t x, int32_t y, double *out);
/* max |x| as NumPy's np.abs(x).max(): NaN if any element is NaN, +inf if any is infinite and none is NaN */
int fwi_vec_absmax(fwi_ctx *ctx, int32_t x, double *out);
/* x := min(max(x, lo), hi) as NumPy's np.clip: a NaN stays a NaN; lo > hi (or a NaN bound) is FWI_EINVAL */
int fwi_vec_clip(fwi_ctx *ctx, int32_t x, double lo, double hi);
/* model := slot (velocity), without leaving the device */
int fwi_set_model_vec(fwi_ctx *ctx, int32_t slot);
/* slot := accumulated gradient (after fwi_allreduce_gradient, if any), as fwi_gradient() */
int fwi_gradient_vec(fwi_ctx *ctx, int32_t wrt, int32_t slot);

/* Source-side illumination: the diagonal of the pseudo-Hessian (Shin et al., 2001), the usual preconditioner of an FWI
 * gradient with surface acquisition.  Off by default; while off no kernel of it runs and no memory is held.
 * With S the image stride and q^n the stored forward term (q^n = C (L u^n + src^n) ~ dt^2 d2u/dt2, what the imaging
 * condition correlates with; in bf16-store mode bf16(C L u^n) + C src^n):
 *     H_m(x) = (S / dt^4) sum_{n % S == 0} q^n(x)^2      illumination w.r.t. m = 1/c^2 (FWI_WRT_SLOWNESS2)
 *     H_c(x) = H_m(x) (2 / c(x)^3)^2                     w.r.t. velocity (FWI_WRT_VELOCITY, the Gauss-Newton diagonal)
 * It accumulates like the gradient: over every fwi_adjoint(..., image != 0) since the last fwi_gradient_reset (which
 * zeroes it), by one streaming pass over the store per shot (per checkpoint segment with ckpt_interval) -- no extra
 * wave propagation.  fwi_gradient_add sums it too when both contexts have it on (FWI_EINVAL when only one has).
 * Reading it while it is off or before a model is set is FWI_ESTATE.  No reference counterpart. */
int fwi_set_illumination(fwi_ctx *ctx, int32_t on);  /* on != 0: allocate and zero the accumulator; 0: free it */
int fwi_illumination(fwi_ctx *ctx, int32_t wrt, void *out);        /* model-shaped host buffer, context dtype */
int fwi_illumination_vec(fwi_ctx *ctx, int32_t wrt, int32_t slot); /* slot := H, as fwi_illumination() */
int fwi_allreduce_illumination(fwi_ctx *ctx);  /* in-place sum over the ranks of fwi_comm_init */

/* Fourier-compressed forward-term store: instead of the N = ceil(nt / S) sampled forward terms q^{jS} (S = image stride,
 * sample j = time step jS) the context keeps F discrete Fourier coefficients of them per cell, accumulated during
 * fwi_forward(save != 0), and fwi_adjoint(image != 0) rebuilds the band-limited term from them batch by batch, just ahead
 * of the imaging steps that read it.  Memory: 2 F + batch + 1 model-sized arrays instead of N; no second forward sweep.
 * With theta_kj = 2 pi f_k j S dt:
 *     analysis    Q_k(x)    = sum_j q^{jS}(x) (cos theta_kj - i sin theta_kj)
 *     synthesis   q~^{jS}(x) = sum_k w_k (Re Q_k(x) cos theta_kj - Im Q_k(x) sin theta_kj)
 *     weights     w_k = 1 / N where f_k = 0 or f_k = 1 / (2 S dt) (the Nyquist frequency of the sampled axis, to a
 *                 relative 1e-9), else 2 / N
 * The imaging condition pairs mu^{n+1} with q~^n exactly where it pairs it with q^n on the configured store, with the
 * same weight S; fwi_gradient and everything above it are unchanged.  On the bin frequencies f_k = k / (N S dt),
 * k = 0 .. floor(N / 2), q~ is the orthogonal projection of the sampled history onto those bins: all of them give the
 * configured store's gradient back (to round-off), fewer give the gradient of the forward term band-passed to the bins
 * kept -- an APPROXIMATION of the full gradient, as good as the bins cover the band of the source (fourier.fourier_bins
 * of the Python package lists the bins inside a band).  Frequencies off the bins are allowed (phase-sensitive
 * detection); q~ is then no projection.
 * fwi_set_fourier_store: nfreq = 0 frees the arrays and returns the context to its configured store.  Otherwise
 * 1 <= nfreq <= FWI_FOURIER_FMAX frequencies in Hz and 1 <= batch <= FWI_FOURIER_BMAX samples per transform launch
 * (batch + 1 ring slots: more slots, fewer passes over the 2 F accumulators).  FWI_EINVAL, with the reason in
 * fwi_last_error, for a frequency that is negative, not finite, equal to another one or above the Nyquist frequency,
 * for a context with ckpt_interval > 0 or store_dtype = bf16, and while illumination is enabled; fwi_set_illumination(on)
 * fails the same way on a context with this store, and fwi_born* on it are FWI_ESTATE.  The call discards what an
 * earlier forward stored (the configured store's memory too).  The arrays are allocated by the first
 * fwi_forward(save != 0) (FWI_ENOMEM when they do not fit); that sweep and fwi_adjoint(image != 0) run one time step per
 * launch, sweeps that store or read nothing keep their fast paths.  Any number of adjoint sweeps may follow one forward.
 * The coefficients are kept in the context dtype; the batch sums and the synthesis run in fp64 registers.
 * fwi_fourier_spectrum: Q_k of the last fwi_forward(save != 0), real and imaginary part as model-shaped host buffers of
 * the context dtype -- the monochromatic forward terms, for quality control and frequency-domain work.
 * fwi_store_bytes: device bytes currently held for the forward store of whichever kind (the configured store, the
 * checkpoint buffers, or the 2 F + batch + 1 arrays of this one; its twiddle table, F (N + 7) pairs of doubles, is not
 * counted); 0 before the first fwi_forward(save != 0) allocates it.  No reference counterpart. */
#define FWI_FOURIER_FMAX 64
#define FWI_FOURIER_BMAX 8
int fwi_set_fourier_store(fwi_ctx *ctx, int32_t nfreq, const double *freqs_hz, int32_t batch);
int fwi_fourier_spectrum(fwi_ctx *ctx, int32_t k, void *re_out, void *im_out);
int fwi_store_bytes(fwi_ctx *ctx, int64_t *bytes_out);

/* Spectral imaging on the Fourier store: the gradient formed in the frequency domain, per frequency (Sirgue, Etgen and
 * Albertin, 2008), instead of by synthesis plus time-domain imaging.  With M_k the same analysis applied to the adjoint
 * field at the imaging samples,
 *     M_k(x) = sum_j mu^{jS+1}(x) (cos theta_kj - i sin theta_kj)       (mu^{jS+1}: what the imaging pairs with q^{jS})
 * the band-limited imaging sum of fwi_adjoint(image != 0) is, exactly and for any set of frequencies,
 *     sum_j mu^{jS+1} q~^{jS} = sum_k w_k Re(Q_k conj M_k) = sum_k w_k (Re Q_k Re M_k + Im Q_k Im M_k)
 * in the units of the gradient accumulator, so the terms of the sum are the per-frequency gradients g_k.
 * fwi_adjoint_spectral: the reverse sweep of fwi_adjoint(ctx, residual, 0, adj_src_out) -- same residual handling
 * (residual == NULL, off-grid point sets), adj_src_out bit-identical -- one time step per launch, with M_k accumulated
 * behind it into 2 F further model-sized arrays (allocated by the first call, FWI_ENOMEM when they do not fit; zeroed by
 * every call; fwi_store_bytes counts them from then on, fwi_set_fourier_store frees them).  The adjoint field is packed
 * into the ring slots the forward sweep no longer needs.  The gradient accumulator is not touched.
 * fwi_fourier_image: gradient accumulator += sum_k a_k w_k Re(Q_k conj M_k), a_k = freq_weights[k] (NULL: ones);
 * fwi_gradient*, fwi_gradient_add and fwi_allreduce_gradient follow as after fwi_adjoint(image != 0).
 * fwi_fourier_gradient[_vec]: the gradient fwi_gradient[_vec] would return if the accumulator held that sum alone (scale
 * -S / dt^2, same `wrt`); the accumulator is not touched.  One-hot weights give g_k.
 * fwi_fourier_adjoint_spectrum: M_k, as fwi_fourier_spectrum returns Q_k.
 * fwi_fourier_illumination[_vec]: H_m = (S / dt^4) sum_k a_k w_k |Q_k|^2, H_c = H_m (2 / c^3)^2, in the units and with the
 * `wrt` of fwi_illumination; needs only the fwi_forward(save != 0).  When every f_k is a bin of the sampled axis this is
 * the illumination (S / dt^4) sum_j (q~^{jS})^2 of the band-limited term (Parseval), with all bins that of the stored
 * term; off the bins it is this formula and no such sum.
 * FWI_ESTATE, with the reason in fwi_last_error: the Fourier store is off; no fwi_forward(save != 0) since it was set; for
 * the image, the gradient and the adjoint spectrum, no fwi_adjoint_spectral after the latest fwi_forward(save != 0).
 * FWI_EINVAL: a weight that is not finite, a negative weight of the illumination, k outside [0, F).  fwi_adjoint(image != 0)
 * on the same context is unchanged and may follow or precede these calls.  No reference counterpart. */
int fwi_adjoint_spectral(fwi_ctx *ctx, const void *residual, void *adj_src_out);
int fwi_fourier_image(fwi_ctx *ctx, const double *freq_weights /* F, or NULL = ones */);
int fwi_fourier_gradient(fwi_ctx *ctx, int32_t wrt, const double *freq_weights, void *out);
int fwi_fourier_gradient_vec(fwi_ctx *ctx, int32_t wrt, const double *freq_weights, int32_t slot);
int fwi_fourier_adjoint_spectrum(fwi_ctx *ctx, int32_t k, void *re_out, void *im_out);
int fwi_fourier_illumination(fwi_ctx *ctx, int32_t wrt, const double *freq_weights, void *out);
int fwi_fourier_illumination_vec(fwi_ctx *ctx, int32_t wrt, const double *freq_weights, int32_t slot);

/* Extended images on the Fourier store: subsurface-offset (Rickett and Sava, 2002) and time-lag (Sava and Fomel, 2006)
 * common-image gathers of the last fwi_adjoint_spectral, one lag per call, each one streaming pass over the resident Q_k
 * and M_k (the bytes of one fwi_fourier_gradient call) and no further sweep.  a_k = freq_weights[k] (NULL: ones), w_k the
 * synthesis weights above, S the image stride, e_a the unit vector of grid axis a (grid order: 0 .. ndim - 1 = z, [y,] x);
 * both in the units of fwi_fourier_gradient(FWI_WRT_SLOWNESS2), and at zero lag (h = 0, tau = 0) bit-identical to it.
 * fwi_fourier_offset_image[_vec]: for an integer h in cells, of either sign,
 *     E_h(x) = -(S / dt^2) sum_k a_k w_k (Re Q_k(x - h e_a) Re M_k(x + h e_a) + Im Q_k(x - h e_a) Im M_k(x + h e_a))
 * and E_h(x) = 0 wherever x - h e_a or x + h e_a lies outside the grid (its extent n_a, not the padded row of the device
 * layout).  |h| is not limited; past (n_a - 1) / 2 the image is all zeros.  For any set of frequencies this equals
 * -(S / dt^2) sum_j mu^{jS+1}(x + h e_a) q~^{jS}(x - h e_a), the band-limited imaging sum of the shifted fields.
 * fwi_fourier_lag_image[_vec]: for a finite tau in seconds,
 *     E_tau(x) = -(S / dt^2) sum_k a_k w_k Re(Q_k(x) conj(M_k(x)) exp(-i 2 pi f_k tau))
 * Where every f_k is a bin of the sampled axis and tau = m S dt, this is the imaging sum with the sampled q~ shifted
 * circularly by m samples (the forward term delayed by tau).  Off the bins, or at any other tau, it is THIS FORMULA AND
 * NO SUCH SUM (as fwi_fourier_illumination off the bins); only tau = 0 is the gradient for every frequency set.
 * `out`: a model-shaped host buffer of the context dtype; `slot`: a vector of fwi_vec_create (pad columns zero).  Neither
 * the gradient accumulator nor Q_k or M_k is touched, and any number of calls may follow one fwi_adjoint_spectral.
 * FWI_ESTATE as for fwi_fourier_gradient: the store is off, no fwi_forward(save != 0), no fwi_adjoint_spectral since the
 * latest one.  FWI_EINVAL, naming the argument: axis outside [0, ndim), tau not finite (or so large that f_k tau is
 * not), a weight that is not finite, a null `out`, a slot that does not exist.  No reference counterpart. */
int fwi_fourier_offset_image(fwi_ctx *ctx, int32_t axis, int32_t h, const double *freq_weights, void *out);
int fwi_fourier_offset_image_vec(fwi_ctx *ctx, int32_t axis, int32_t h, const double *freq_weights, int32_t slot);
int fwi_fourier_lag_image(fwi_ctx *ctx, double tau, const double *freq_weights, void *out);
int fwi_fourier_lag_image_vec(fwi_ctx *ctx, double tau, const double *freq_weights, int32_t slot);

/* The tomographic / migration split of fwi_fourier_gradient (wavefield-decomposition imaging: Liu et al., 2011; the
 * background update of reflection waveform inversion: Xu et al., 2012), one streaming pass over the resident Q_k and M_k
 * with an antisymmetric FIR along one grid axis, no further sweep and no model-sized storage.  The state rules are those
 * of fwi_fourier_gradient (after fwi_forward(save != 0) and fwi_adjoint_spectral).  With the one-sided taps
 * t_1 .. t_R = taps[0 .. ntaps - 1] (datafit.hilbert_taps in Python: an FIR Hilbert transformer) and the grid axis a
 * (grid order: 0 .. ndim - 1 = z, [y,] x),
 *     (H u)(i) = sum_{r = 1 .. R} t_r (u(i - r) - u(i + r))      along axis a,
 * where cells outside [0, n_a) contribute nothing (zero extension against the GRID's extent, not the padded row of the
 * device layout), taps that are exactly zero are skipped, and H acts on Re and Im separately:
 *     part(x) = kappa sum_k a_k w_k [ alpha (Re Q_k Re M_k + Im Q_k Im M_k) + beta (Re HQ_k Re HM_k + Im HQ_k Im HM_k) ]
 * (alpha, beta) = (1/2, 1/2) for FWI_SPLIT_SAME: with U^+- = (U +- i H U) / 2 the parts of positive and negative
 * wavenumber along the axis, this is Re(Q+ conj M+) + Re(Q- conj M-), the pairs that travel the same way (low wavenumber,
 * tomographic); (1/2, -1/2) for FWI_SPLIT_OPPOSITE: Re(Q+ conj M-) + Re(Q- conj M+), the pairs that travel in opposite
 * directions (high wavenumber, migration); (0, 1) for FWI_SPLIT_HILBERT: the image of the filtered coefficients alone.
 * kappa and the `wrt` scaling are exactly those of fwi_fourier_gradient; a_k = freq_weights[k] (NULL: ones).  SAME +
 * OPPOSITE equals fwi_fourier_gradient(freq_weights, wrt) to round-off.  NEITHER PART IS THE GRADIENT OF THE MISFIT: they
 * are the two halves of it.  1 <= ntaps <= FWI_SPLIT_RMAX; ntaps may exceed n_a, the excess taps touch nothing.  The
 * transition band of the FIR leaves |k_a| below about 2 / (R + 1) cycles per cell in neither part cleanly, and zero
 * extension distorts the R cells next to each face of the axis.
 * `out`: a model-shaped host buffer of the context dtype (staged through the array fwi_fourier_gradient stages through);
 * `slot`: a vector of fwi_vec_create (pad columns zero).  Neither the gradient accumulator nor Q_k or M_k is written, and
 * any number of calls may follow one fwi_adjoint_spectral.
 * FWI_ESTATE as for fwi_fourier_gradient: the store is off, no fwi_forward(save != 0), no fwi_adjoint_spectral since the
 * latest one, or fwi_fourier_born_extended has overwritten M_k since.  FWI_EINVAL, naming the argument and touching
 * nothing: an unknown wrt or part, axis outside [0, ndim), ntaps outside [1, FWI_SPLIT_RMAX], null taps, a tap or weight
 * that is not finite, a null `out`, a slot that does not exist.  No reference counterpart. */
enum { FWI_SPLIT_SAME = 0, FWI_SPLIT_OPPOSITE = 1, FWI_SPLIT_HILBERT = 2 };
#define FWI_SPLIT_RMAX 64
int fwi_fourier_split_image(fwi_ctx *ctx, int32_t wrt, int32_t part, int32_t axis, int32_t ntaps, const double *taps,
                            const double *freq_weights /* F, or NULL = ones */, void *out);
int fwi_fourier_split_image_vec(fwi_ctx *ctx, int32_t wrt, int32_t part, int32_t axis, int32_t ntaps, const double *taps,
                                const double *freq_weights, int32_t slot);

/* Elementwise vector operations for a diagonal preconditioner (pad columns of the compact layout stay 0). */
int fwi_vec_mul(fwi_ctx *ctx, int32_t y, int32_t x);               /* y := x * y */
int fwi_vec_recip(fwi_ctx *ctx, int32_t y, double a, double b);    /* y := a / (y + b) */

/* Gaussian smoothing of a vector slot, in place and stream-ordered like fwi_vec_axpby: y := S y, S = S_z S_y S_x applied
 * in the order x, y, z.  `sigma`: ndim widths in cells, in grid order (z, [y,] x).  Per axis of n cells and width s:
 *   R = int(3 s + 0.5),  w_k = exp(-k^2 / 2 s^2) / sum_{j=-R..R} exp(-j^2 / 2 s^2),  (S_s x)_i = sum_k w_k x_rho(i+k),
 * rho the half-sample mirror (rho(j) = -1 - j for j < 0, 2 n - 1 - j for j >= n): scipy.ndimage.gaussian_filter with
 * mode="reflect", truncate=3.0.  S is symmetric and preserves constants (it is not positive semi-definite on its own).
 * s = 0 is the identity on that axis (no launch).  FWI_EINVAL: a negative or non-finite width, R > 32, R > n (one
 * reflection only), a slot that does not exist.  The weights are formed in fp64 and rounded to the context's dtype; the
 * summation order is fixed, so equal inputs give equal bits on every call and rank.  Pad columns stay zero.  The
 * ping-pong vector is the context's own (allocated by the first call, freed by fwi_destroy).  No reference counterpart. */
int fwi_vec_smooth(fwi_ctx *ctx, int32_t y, const double *sigma);

/* First-order Tikhonov and smoothed isotropic total-variation regularisation of a vector slot, stream-ordered like
 * fwi_vec_axpby.  d = x - x0 (x0 = -1: d = x); per axis a of the grid order (z, [y,] x), with weight[a] >= 0 in cell units:
 *   (D_a d)_i = d_{i+e_a} - d_i for i_a < n_a - 1, 0 on the last cell of the axis (against nx, not the padded row),
 *   s_i = sum_a weight[a] (D_a d)_i^2,
 *   FWI_REG_TIKHONOV  R = 1/2 sum_i s_i,                    k_i = 1,
 *   FWI_REG_TV        R = sum_i (sqrt(s_i + eps^2) - eps),  k_i = 1 / sqrt(s_i + eps^2),   eps > 0,
 *   L(d; v)_j = sum_a weight[a] [k_{j-e_a}(d) (D_a v)_{j-e_a} - k_j(d) (D_a v)_j]  =  (sum_a weight[a] D_a^T diag(k) D_a v)_j.
 * The call computes out := alpha L(d; v) + beta out (v = -1: v = d, L(d; d) is the gradient of R; out = -1: the value
 * only) and, with value_out != NULL, *value_out = R(d) (this synchronises the stream).  For fixed d, L is symmetric
 * positive semi-definite in v (the exact Hessian of Tikhonov, the lagged-diffusivity one of TV) with the constants in its
 * null space.  With beta == 0 the old contents of out are not read.  All arithmetic between the loads and the final
 * rounding to the context's dtype is fp64; R is summed in fp64 in a fixed order (block partial sums in a buffer the
 * context owns, allocated by the first call and freed by fwi_destroy; no atomics): equal inputs give equal bits on
 * every call and rank.  Pad columns of out are written as zeros.  FWI_EINVAL, naming the argument and touching nothing:
 * an unknown kind; a slot that does not exist; out aliasing x, x0 or v; out == -1 with value_out == NULL; a null weight;
 * a negative or non-finite weight[a]; TV with eps not finite or <= 0; a non-finite alpha or beta.  eps is ignored by
 * Tikhonov.  No reference counterpart. */
enum { FWI_REG_TIKHONOV = 0, FWI_REG_TV = 1 };
int fwi_vec_regularizer(fwi_ctx *ctx, int32_t kind, int32_t x, int32_t x0 /* -1: none */, int32_t v /* -1: v = d */,
                        int32_t out /* -1: value only */, double alpha, double beta, const double *weight /* ndim */,
                        double eps, double *value_out /* R(d), or NULL */);

/* A weighted sum of vector slots shifted along z (depth, the first grid axis) by real numbers of cells, stream-ordered
 * like fwi_vec_axpby: the slant stack that turns a subsurface-offset gather into an angle-domain gather, and its exact
 * transpose.  For a finite s let n = floor(s) and f = s - n, formed in fp64:
 *   (S_s a)(z, .) = (1 - f) a(z + n, .) + f a(z + n + 1, .),
 * where a tap whose plane lies outside 0 .. nz - 1 contributes zero (the other tap still counts), the second tap is
 * neither read nor counted when f == 0, and |s| >= nz + 1 gives zeros (n is held in 64 bits and tested against the grid
 * before any address is formed from it).  With this masking S_s^T = S_{-s} exactly.  The call computes
 *   dst := beta dst + sum_{i < nsrc} weights[i] S_{shifts[i]} src_slots[i]
 * with one fp64 sum per cell: sources ascending, per source s = fma(w (1 - f), first tap, s) then s = fma(w f, second
 * tap, s), at the end dst = (beta == 0 ? s : fma(beta, dst, s)) rounded once to the context's dtype.  Nothing is shared
 * or atomic: equal inputs give equal bits on every call and rank.  With beta == 0 the old contents of dst are not read.
 * Pad columns of dst are written as zeros.  The same source may appear twice.  A source shifted out of the grid
 * entirely is skipped; with all of them skipped dst := beta dst still happens.  Needs no model, forward or Fourier
 * store.  FWI_EINVAL, naming the argument and touching nothing: a slot that does not exist; nsrc outside
 * [1, FWI_SHIFT_SUM_MAX]; a null src_slots or shifts; a shift, weight or beta that is not finite; dst among the
 * sources.  No reference counterpart. */
#define FWI_SHIFT_SUM_MAX 64
int fwi_vec_shift_sum(fwi_ctx *ctx, int32_t dst, int32_t nsrc, const int32_t *src_slots, const double *shifts,
                      const double *weights /* nsrc, or NULL = ones */, double beta);

/* Values at grid nodes into and out of a vector slot, so that receivers never cost a model-sized transfer.  `idx`: n
 * nodes as (n, ndim) grid coordinates (z, [y,] x), as everywhere in this header.
 *   fwi_vec_scatter_points: slot := beta slot (beta == 0: zeros, the old contents are not read), then
 *     slot[idx_k] += values[k], values rounded to the context's dtype first and each node added to once: the result is
 *     what NumPy's `a = beta * a; a[idx] += values` gives in that dtype, bit for bit.  Stream-ordered like fwi_vec_axpby.
 *     FWI_EINVAL, touching nothing: a node listed twice or outside the grid, a non-finite value or beta, a null pointer
 *     with n > 0, n < 0, a slot that does not exist.  n == 0 scales only.
 *   fwi_vec_gather_points: out[k] = slot[idx_k] as doubles (exact); the same node may be listed twice.  Synchronises.
 * Pad columns stay zero.  Neither needs a model.  No reference counterpart. */
int fwi_vec_scatter_points(fwi_ctx *ctx, int32_t slot, int32_t n, const int32_t *idx, const double *values, double beta);
int fwi_vec_gather_points(fwi_ctx *ctx, int32_t slot, int32_t n, const int32_t *idx, double *out);

/* First-arrival traveltimes of the context's model and their discrete adjoint (the definition and
 * fp64 twin is full_waveform_inversion_amd/eikonal.py).  |grad T| = 1 / c on the engine's grid (spacing fwi_config.h)
 * by the first-order Godunov upwind scheme: per cell i and axis d, t_d = min(T[i - e_d], T[i + e_d]) (outside the grid:
 * +inf; on a tie the lower-index neighbour is the upwind one), sorted a <= b <= c, f = h / c_i, b' = b - a, c' = c - a,
 *   G_i = a + f                                   if that is <= b,
 *         a + (b' + sqrt(2 f^2 - b'^2)) / 2       else, if that is <= c (always in 2-D),
 *         a + (S + sqrt(S^2 - 3 (Q - f^2))) / 3   else, with S = b' + c', Q = b'^2 + c'^2.
 * The source is an init list: n_init nodes init_idx (n_init, ndim) with their distances init_dist in metres and one
 * reference node ref_idx (ndim); T_init = (1 / c[ref]) init_dist on the listed nodes, +inf elsewhere, and the result is the
 * limit of T <- min(T, T_init, G(T)).  A listed node is source-determined exactly when its final T_i < G_i.
 *
 * fwi_eikonal: t_slot := T.  Block Jacobi between t_slot and scratch_slot: per launch a workgroup takes a tile with the
 *   cells around it frozen through K inner sweeps and writes it to the other slot, so a launch depends on its input
 *   only and equal inputs give equal bits and equal launch counts.  It stops after the first launch that changes
 *   nothing (both slots then hold T) and writes the number of launches to *launches_out (may be NULL).  max_sweeps
 *   (<= 0: 4 * the sum of the grid's extents) caps launches * K: FWI_ESTATE if the last one still changed something;
 *   t_slot then holds an upper bound of T everywhere.  scratch_slot's contents are lost.
 * fwi_eikonal_adjoint: lam_slot := the solution of lambda = rhs + A^T lambda, A_ij = dG_i/dT_j at the fixed point in
 *   t_slot: with D the axes with t_d < T_i, dG_i/dt_d = (T_i - t_d) / sum_{e in D} (T_i - t_e), zero where T_i < G_i.
 *   A is strictly causal, so the Jacobi iteration (gather form, the up to 2 ndim terms of a cell added axis by axis,
 *   lower neighbour first; no atomics on lambda) stops bit-exactly; launches, cap and count as above.  t_slot and
 *   rhs_slot are read only; scratch_slot's contents are lost.
 * fwi_eikonal_gradient: out_slot := beta out_slot + g, the gradient of sum_i rhs_i T_i with respect to the model:
 *   g_s,i = lambda_i h^2 / (c_i sum_{e in D} (T_i - t_e)), plus sum_k init_dist[k] lambda[init_idx_k] over the
 *   source-determined listed nodes (added in list order) at ref; then g = -g_s / c^2 for FWI_WRT_VELOCITY or
 *   g_s c / 2 for FWI_WRT_SLOWNESS2.  One elementwise pass; with beta == 0 out_slot is not read.  Stream-ordered.
 * The non-differentiable set (exact ties of the two neighbours on an axis, switches of the active set) gets the
 * one-sided choice above.  Pad columns of every slot stay zero.  Refused before anything is written -- FWI_EINVAL: a
 * slot that does not exist; two arguments naming the same slot (out_slot may not be t_slot or lam_slot); an empty init
 * list; a listed or reference node outside the grid or listed twice; a negative or non-finite distance or beta; an
 * unknown wrt; a null pointer.  FWI_ESTATE: no model set.  No sweep state of the context is touched.  Out of scope:
 * the factored equation, second-order stencils, anisotropy; of the later arrivals all but reflections off a fixed
 * interface (fwi_eikonal_stage below).  No reference counterpart. */
int fwi_eikonal(fwi_ctx *ctx, int32_t t_slot, int32_t scratch_slot, int32_t n_init, const int32_t *init_idx,
                const double *init_dist, const int32_t *ref_idx, int32_t max_sweeps, int32_t *launches_out);
int fwi_eikonal_adjoint(fwi_ctx *ctx, int32_t t_slot, int32_t rhs_slot, int32_t lam_slot, int32_t scratch_slot,
                        int32_t max_sweeps, int32_t *launches_out);
int fwi_eikonal_gradient(fwi_ctx *ctx, int32_t wrt, int32_t t_slot, int32_t lam_slot, int32_t out_slot, double beta,
                         int32_t n_init, const int32_t *init_idx, const double *init_dist, const int32_t *ref_idx);

/* fwi_eikonal_tangent: out_slot := dT, the derivative of the fixed point T in t_slot along the model perturbation in
 * dm_slot (the definition is `tangent` of full_waveform_inversion_amd/eikonal.py).  With the weights,
 * the active axes D and the init list of the three calls above:
 *   ds_i = -dm_i / c_i^2 for FWI_WRT_VELOCITY, dm_i c_i / 2 for FWI_WRT_SLOWNESS2 (the transposes of the gradient's
 *          g = -g_s / c^2 and g = g_s c / 2),
 *   b_i  = ds_i h^2 / (c_i sum_{e in D} (T_i - t_e)); on a listed node that is source-determined (T_i < G_i, the same
 *          decision as in fwi_eikonal_gradient) b_i = init_dist[k] ds[ref]; 0 where T_i = +inf,
 *   x    = b + A x,  (A x)_i = sum_d dG_i/dt_d x[upwind neighbour of i on axis d]: gather form, the terms of a cell
 *          added axis by axis in ascending order after b_i, the upwind neighbour being the lower-index one on a tie.
 * It is the exact transpose of fwi_eikonal_adjoint followed by fwi_eikonal_gradient: <w, dT> equals <g(w), dm> to
 * round-off for every w and dm.  A is strictly causal, so the block-Jacobi iteration between out_slot and scratch_slot
 * stops bit-exactly; launches, max_sweeps, the cap (FWI_ESTATE if the last allowed launch still changed something) and
 * *launches_out behave as for fwi_eikonal_adjoint.  b is never stored and no model-sized memory is allocated: both
 * slots start as zeros with the source-determined listed nodes set, and a launch forms b_i of a live cell from dm_i
 * and c_i.  No atomics on x.  t_slot and dm_slot are read only; scratch_slot's contents are lost; pad columns stay
 * zero.  The non-differentiable set gets the same one-sided choice as the adjoint.  Refused before anything is written
 * -- FWI_EINVAL, naming the argument: a slot that does not exist; any two of the four slots equal; an empty init list;
 * a listed or reference node outside the grid or listed twice; a negative or non-finite distance; an unknown wrt; a
 * null pointer.  FWI_ESTATE: no model set.  The values of dm are not validated.  No sweep state of the context is
 * touched.  No reference counterpart. */
int fwi_eikonal_tangent(fwi_ctx *ctx, int32_t wrt, int32_t t_slot, int32_t dm_slot, int32_t out_slot,
                        int32_t scratch_slot, int32_t n_init, const int32_t *init_idx, const double *init_dist,
                        const int32_t *ref_idx, int32_t max_sweeps, int32_t *launches_out);

/* Walled and slot-started solves, and what chains two of them into the reflection off a FIXED interface (DESIGN.md
 * s.4y; the definitions are `solve_from`, `handover` and `tangent(..., b0)` of full_waveform_inversion_amd/eikonal.py).
 * A wall is a vector slot: a cell whose value there is != 0 holds T = +inf from start to end, whatever the start says,
 * and is never updated, so that to every other cell it is a neighbour outside the grid.  A node is source-determined
 * when its final T_i is finite and < G_i; then T_i is its start's.  Reflection off the nodes Gamma inside a wall:
 * stage 1 is fwi_eikonal_stage from the source's list with the wall, stage 2 fwi_eikonal_stage with n_init == 0 from a
 * slot that holds stage 1's times on Gamma and +inf elsewhere; backwards lambda_2 = adjoint(T_2), fwi_eikonal_handover
 * (T_2, lambda_2) is the right-hand side of stage 1's adjoint, and the gradient is fwi_eikonal_gradient_field(T_2,
 * lambda_2) + fwi_eikonal_gradient(T_1, lambda_1); forwards x_1 = fwi_eikonal_tangent(T_1), x_2 =
 * fwi_eikonal_tangent_stage(T_2, b0 = fwi_eikonal_handover(T_2, x_1), n_init = 0).  The two are exact transposes.
 * fwi_eikonal_adjoint needs no wall: a walled cell is not live and nobody's upwind neighbour.
 *
 * fwi_eikonal_stage: t_slot := the limit of T <- min(T, G(T)) from T_init.  n_init > 0: T_init comes from the list as in
 *   fwi_eikonal; n_init == 0: t_slot holds T_init (finite and >= 0 on the secondary sources, +inf elsewhere; the list
 *   pointers are not read).  wall_slot == -1: no wall, and nothing is read for one; with a list the times, both slots
 *   and *launches_out are then those of fwi_eikonal bit for bit (the same launches).  With a wall every launch reads
 *   one more value per cell.  Launches, K, max_sweeps, the cap (FWI_ESTATE, an upper bound of T in t_slot) and
 *   *launches_out as for fwi_eikonal; both slots end equal, walled cells +inf in both.  Synchronises once more than
 *   fwi_eikonal when n_init == 0 (the check of the start).
 * fwi_eikonal_handover: out_slot := beta out_slot + [T_i finite and T_i < G_i] in_slot, G from the neighbours' times in
 *   t_slot as in fwi_eikonal_gradient.  One elementwise pass; with beta == 0 out_slot is not read.  Stream-ordered.
 * fwi_eikonal_gradient_field: fwi_eikonal_gradient without the source term (no list): the gradient of a stage whose
 *   start is handed over and not a function of the model at a reference node.
 * fwi_eikonal_tangent_stage: out_slot := the solution of x = b(dm) + b0 + A x with b and A of fwi_eikonal_tangent and
 *   b0 the values of b0_slot (-1: none), added after b_i and before the axis terms.  n_init == 0: no list, no source
 *   term.  Both slots start as 0 + b0_i on the cells that are not live (a listed source-determined node:
 *   init_dist[k] ds[ref] + b0_i) and 0 on the live ones.  Without b0_slot the launches are fwi_eikonal_tangent's.
 * No atomics on the fields; pad columns of every slot stay zero; equal inputs give equal bits.  Refused before anything
 * is written -- FWI_EINVAL, naming the argument: a slot that does not exist (wall_slot and b0_slot: other than -1); two
 * arguments naming one slot; n_init < 0; with n_init == 0 a start that holds, outside the wall, a NaN, a negative entry
 * or no finite entry; with n_init > 0 a bad list as in fwi_eikonal; an unknown wrt; a beta that is not finite.
 * FWI_ESTATE: no model set.  The values of the wall, dm, b0 and in are not validated.  No sweep state of the context is
 * touched.  Out of scope: the reflector's depth as an unknown, a sub-cell reflector position, head waves, multiples and
 * transmitted conversions as separate arrivals.  No reference counterpart. */
int fwi_eikonal_stage(fwi_ctx *ctx, int32_t t_slot, int32_t scratch_slot, int32_t wall_slot /* -1: none */,
                      int32_t n_init /* 0: t_slot holds T_init */, const int32_t *init_idx, const double *init_dist,
                      const int32_t *ref_idx, int32_t max_sweeps, int32_t *launches_out);
int fwi_eikonal_handover(fwi_ctx *ctx, int32_t t_slot, int32_t in_slot, int32_t out_slot, double beta);
int fwi_eikonal_gradient_field(fwi_ctx *ctx, int32_t wrt, int32_t t_slot, int32_t lam_slot, int32_t out_slot,
                               double beta);
int fwi_eikonal_tangent_stage(fwi_ctx *ctx, int32_t wrt, int32_t t_slot, int32_t dm_slot,
                              int32_t b0_slot /* -1: none */, int32_t out_slot, int32_t scratch_slot,
                              int32_t n_init /* 0: no list */, const int32_t *init_idx, const double *init_dist,
                              const int32_t *ref_idx, int32_t max_sweeps, int32_t *launches_out);

/* Born (linearised) modelling dd = J dm: the exact derivative of the discrete fwi_forward along a model perturbation,
 * whose exact transpose is fwi_adjoint(image) + fwi_gradient.  With C = dt^2 c^2 and q^n the forward term the store of
 * fwi_forward(save != 0) holds for every step (q^n = C (L u^n + PML terms + src^n)):
 *     w        = dC / C = 2 dc / c  (FWI_WRT_VELOCITY: dm is dc)   or   -c^2 dm  (FWI_WRT_SLOWNESS2: dm perturbs 1 / c^2)
 *     dq^n     = C (L du^n + the CPML terms of du^n) + w q^n        (no point source)
 *     du^{n+1} = A (2 du^n - B du^{n-1} + dq^n),   du^0 = du^{-1} = 0;   dd^n = R du^{n+1},  n = 0 .. nt - 1
 * (increment form: dv' = A (B dv + dq), du' = du + dv'; the CPML memory variables of du start at zero and follow the
 * forward recursion).  The Born field obeys the wavefield's own recursion with the distributed source w q^n, so J costs
 * one more sweep over data already on the device: the ordinary one-step launches, each followed by du^{n+1} += A w q^n.
 *  - Needs a preceding fwi_forward / fwi_forward_spread with save != 0 on this context (else FWI_ESTATE); uses that
 *    call's nt and receivers and returns (nt, nrec) -- per point after fwi_forward_spread, as that call does.
 *  - Reads the store, never writes it: it may be called any number of times after one forward, and a following
 *    fwi_adjoint(..., image = 1) accumulates bit for bit what it would have without the Born call in between.
 *  - Runs in the context's wavefield buffers (free once the forward sweep has ended) plus one model-shaped compact array for w, allocated by the first call and
 *    freed by fwi_destroy.
 *  - Leaves dd on the device as the residual of the next fwi_adjoint(ctx, NULL, ...): the Gauss-Newton product
 *    H v = J^T J v is fwi_forward(save), fwi_born_vec, fwi_adjoint(NULL, image = 1), fwi_gradient_vec with no model- or
 *    data-sized PCIe transfer (seis_out == NULL skips the download).  The forward's synthetics are gone for
 *    fwi_misfit_l2 afterwards (FWI_ESTATE, the rule that holds after an adjoint).
 *  - Contexts whose store does not hold every q^n in the field's type cannot serve the EXACT derivative: on
 *    image_stride > 1, store_dtype = bf16 and ckpt_interval > 0 fwi_born / fwi_born_vec return FWI_EINVAL.
 *    fwi_born_imaging (below) runs on every context.
 *  - mode: FWI_BORN_SCATTER is the path above, available on every context.  FWI_BORN_FUSED carries w q^n inside the step
 *    kernel (no second pass: 24 instead of 32 B per point and step, 28 instead of 44 in increment form); it exists for
 *    3-D fp32 O(8) contexts on the stream kernel without the CPML and returns FWI_EINVAL on any other.  FWI_BORN_AUTO takes
 *    FUSED where it exists (measured at 0.58 - 0.74 of SCATTER's time per step), SCATTER elsewhere.  The
 *    selector is an argument, not an environment switch.  The two paths agree to round-off, not bit for bit.
 *  - The time loop is timed like the others (fwi_last_loop_ms, fwi_last_host_ms) and honours launch_mode.
 * No reference counterpart. */
enum { FWI_BORN_AUTO = 0, FWI_BORN_SCATTER = 1, FWI_BORN_FUSED = 2 };
int fwi_born(fwi_ctx *ctx, int32_t wrt, const void *dm_host, int32_t mode, void *seis_out /* (nt, nrec) or NULL */);
int fwi_born_vec(fwi_ctx *ctx, int32_t wrt, int32_t slot, int32_t mode, void *seis_out); /* dm from a device vector */
/* The IMAGING Born operator J_img: the operator whose exact transpose fwi_adjoint(image) + fwi_gradient are ON THIS
 * CONTEXT'S STORE, so that H = J_img^T J_img is symmetric positive semi-definite under every store mode (conjugate
 * gradients needs that; the exact J paired with a decimated J^T is not symmetric).  The recursion of fwi_born with the
 * scattering source taken from what the store holds, q~:
 *     dq^n = C (L du^n + the CPML terms of du^n) + [n % S == 0] S w q~^n,    S = image_stride
 *  - plain store (S = 1, native type): q~^n = q^n, J_img = J; the call takes fwi_born's code path, bit for bit.
 *  - image_stride S > 1: q~^n is slot n / S; the source acts on the stored steps only, with the quadrature weight S
 *    (folded into w once per call).  The steps in between are plain step launches: no scatter pass, no Born variant.
 *  - store_dtype = bf16: q~^n = bf16(C L u^n) + C src^n, the split the imaging side uses: the store's part is read as
 *    bf16 (FUSED: 22 instead of 24 B per point and step; SCATTER: 14 instead of 16 B in its second pass), the source's
 *    exact share w(x_s) C src^n(x_s) joins du^{n+1} at the source nodes (entries that share a node are summed first).
 *  - ckpt_interval K > 0: J_img = J (a recomputed q^n is the stored q^n).  Segment by segment in ascending order the
 *    forward state is restored from its snapshot, the segment's q^n are recomputed into the slot buffer and the Born
 *    field sweeps them: one forward sweep's work more than a store-all Born sweep.  The snapshots are read, never
 *    written.
 * State rules, mode, the residual left for fwi_adjoint(ctx, NULL, ...), timing, launch_mode and fwi_born_path are those
 * of fwi_born; FWI_BORN_FUSED exists on the same contexts (the bf16 store included).  No reference counterpart. */
int fwi_born_imaging(fwi_ctx *ctx, int32_t wrt, const void *dm_host, int32_t mode, void *seis_out /* (nt, nrec) or NULL */);
int fwi_born_imaging_vec(fwi_ctx *ctx, int32_t wrt, int32_t slot, int32_t mode, void *seis_out);
const char *fwi_born_path(const fwi_ctx *ctx);  /* static name of the path the last Born sweep took: "scatter", "fused";
                                                   "none" before the first */

/* Born and extended Born modelling on the Fourier store (fwi_set_fourier_store), whose fwi_born* stay FWI_ESTATE: the
 * recursion of fwi_born_imaging with the scattering source synthesised, batch by batch in forward time order, from the
 * coefficients the store holds.  theta_kj, w_k, Q_k, M_k, S as above; a_k = freq_weights[k] (NULL: ones), folded into
 * the synthesis table on the host.
 * fwi_fourier_born[_vec]:
 *     dq^n = C (L du^n + the CPML terms of du^n) + [n % S == 0] S w q~_a^n
 *     q~_a^{jS}(x) = sum_k a_k w_k (Re Q_k(x) cos theta_kj - Im Q_k(x) sin theta_kj),   w as for fwi_born
 * With a = 1 this is the exact transpose of fwi_adjoint(image != 0) + fwi_gradient on this context, with any a that of
 * fwi_adjoint_spectral + fwi_fourier_gradient(freq_weights = a): H_a = J_a^T J_a is symmetric positive semi-definite.
 * It reads Q_k and never writes it; M_k and the gradient accumulator are not touched, and a following adjoint of either
 * kind returns the bits it would have returned without the call in between.
 * fwi_fourier_born_extended[_vec]: extended Born modelling (demigration), the exact transpose of
 * fwi_fourier_offset_image / fwi_fourier_lag_image: for a gather (E_l), l = 0 .. nlag - 1, in the units of those calls,
 * and every residual r,   <J_ext E, r> = sum_l <E_l, offset_image_{h_l}(r)>   (or lag_image_{tau_l}(r)).
 * `kind`: FWI_EXT_OFFSET with `offsets` (nlag integers h_l in cells along grid axis `axis`, of either sign and any size;
 * `taus` is ignored) or FWI_EXT_TIMELAG with `taus` (nlag finite tau_l in seconds; `offsets` and `axis` are ignored).
 * `images_host`: nlag model-shaped arrays of the context dtype, one behind the other; `slots`: nlag vector slots.  The
 * extended scattering spectrum is formed one lag per launch,
 *     offset   P_k(y) = sum_l E_l(y - h_l e_a) Q_k(y - 2 h_l e_a)    over the l whose y - h_l e_a and y - 2 h_l e_a are
 *                                                                    cells of the grid (a lag that has none adds nothing)
 *     lag      P_k(y) = sum_l E_l(y) Q_k(y) exp(-i 2 pi f_k tau_l)
 * (fp64 between the loads and one rounding to the context dtype per lag), and the Born sweep above runs with the source
 *     [n = jS]  S (-c(y)^2) sum_k a_k w_k (Re P_k(y) cos theta_kj - Im P_k(y) sin theta_kj):
 * the factor -c^2 sits at the injection cell y.  With the single lag h = 0 (or tau = 0) and E_0 = dm the call equals
 * fwi_fourier_born(FWI_WRT_SLOWNESS2, dm) to round-off, not bit for bit.
 * P_k IS WRITTEN INTO THE 2 F ARRAYS THAT HOLD M_k (allocated here if no fwi_adjoint_spectral has run yet;
 * fwi_store_bytes counts them): the extended call destroys M_k, and fwi_fourier_gradient*, fwi_fourier_image,
 * fwi_fourier_offset_image*, fwi_fourier_lag_image* and fwi_fourier_adjoint_spectrum are FWI_ESTATE until the next
 * fwi_adjoint_spectral -- the call a Gauss-Newton loop makes next anyway.  Q_k is read only.
 * All four: the state rules, `mode` (FWI_BORN_FUSED on the same contexts), fwi_born_path, timing and launch_mode of
 * fwi_born_imaging; one time step per launch, the fused path too; dd stays on the device as the residual of the next
 * fwi_adjoint(ctx, NULL, ...) or fwi_adjoint_spectral(ctx, NULL, ...), and the forward's synthetics are gone for
 * fwi_misfit_* afterwards.  FWI_ESTATE: the store is off, or no fwi_forward(save != 0) since it was set.  FWI_EINVAL,
 * naming the argument and touching nothing: an unknown wrt, kind or mode; axis outside [0, ndim); nlag < 1; a null
 * pointer; a slot that does not exist; a tau or weight that is not finite; a repeated lag.  No reference counterpart. */
enum { FWI_EXT_OFFSET = 0, FWI_EXT_TIMELAG = 1 };
int fwi_fourier_born(fwi_ctx *ctx, int32_t wrt, const void *dm_host, const double *freq_weights, int32_t mode,
                     void *seis_out /* (nt, nrec) or NULL */);
int fwi_fourier_born_vec(fwi_ctx *ctx, int32_t wrt, int32_t slot, const double *freq_weights, int32_t mode,
                         void *seis_out);
int fwi_fourier_born_extended(fwi_ctx *ctx, int32_t kind, int32_t axis, int32_t nlag, const int32_t *offsets,
                              const double *taus, const void *images_host, const double *freq_weights, int32_t mode,
                              void *seis_out);
int fwi_fourier_born_extended_vec(fwi_ctx *ctx, int32_t kind, int32_t axis, int32_t nlag, const int32_t *offsets,
                                  const double *taus, const int32_t *slots, const double *freq_weights, int32_t mode,
                                  void *seis_out);

/* Shot-parallel exchange: one RCCL communicator per context, sum of the
 * gradient accumulators over ranks (in place, on device).  The reference's
 * only counterpart is the gather-by-concatenation of Monte Carlo samples,
 * full_waveform_inversion.py:816-848.  [SURVEY s.8e] */
#define FWI_UNIQUE_ID_BYTES 128
int fwi_comm_unique_id(void *id_out /* FWI_UNIQUE_ID_BYTES */);
int fwi_comm_init(fwi_ctx *ctx, int32_t rank, int32_t nranks, const void *id);
/* What RCCL itself says about the communicator (ncclCommCount / ncclCommUserRank): the evidence that
 * the N ranks of a job really share one communicator, echoed by bench.py as config.rccl_ranks. */
int fwi_comm_info(fwi_ctx *ctx, int32_t *nranks_out, int32_t *rank_out);
/* Tear the communicator down without waiting for peers (ncclCommAbort): the clean-up of a rank whose
 * job is being abandoned because another rank failed to join. */
int fwi_comm_abort(fwi_ctx *ctx);
int fwi_allreduce_gradient(fwi_ctx *ctx);
/* In-place sum / max over ranks of n <= 8 doubles (misfit values; the slowest rank's elapsed time). */
int fwi_allreduce_f64(fwi_ctx *ctx, double *vals, int32_t n);
int fwi_allreduce_f64_max(fwi_ctx *ctx, double *vals, int32_t n);

/* Measurement hooks (bench.py): device time of the last time loop, from HIP
 * events on the context's stream, and the synchronising fence. */
int fwi_last_loop_ms(fwi_ctx *ctx, double *ms_out);
/* Host side of the last time loop: wall time the calling thread spent forming and submitting its launches
 * (FWI_LAUNCH_GRAPH: capture + instantiation + the one graph launch), and of that the graph's capture + instantiation
 * alone (0 in stream mode).  Compared with fwi_last_loop_ms it tells whether a loop is bound by the host's launch rate. */
int fwi_last_host_ms(fwi_ctx *ctx, double *submit_ms_out, double *graph_build_ms_out);
/* Placement search (3-D fp32 stream contexts with the convolutional PML or in increment form, past the cache-resident
 * sizes): fwi_create times a few steps with some of the context's arrays at different offsets inside padded
 * allocations and keeps the fastest; results never depend on it.  Time per step before and after the search in
 * microseconds (0 = no search ran for this context) and, into shift_bytes_out[8], the chosen offsets in bytes of the
 * movable arrays in search order (CPML: ty, zeta_x, tz, psi_x, then v in increment form; increment form without CPML:
 * v, C; unused entries 0).  Under FWI_PLACEMENT_TUNE=fixed:... (fwi_create) the offsets are the requested ones and both
 * times are 0: no search ran.  Any out pointer may be NULL.  No reference counterpart. */
int fwi_placement_info(fwi_ctx *ctx, double *us_before_out, double *us_after_out, int64_t *shift_bytes_out);
/* Change fwi_config.launch_mode of a live context (takes effect with the next sweep): the A/B of stream launches against
 * hipGraph launches on ONE context, the same buffers and the same cache state (tools/graph_probe.py). */
int fwi_set_launch_mode(fwi_ctx *ctx, int32_t mode);
int fwi_synchronize(fwi_ctx *ctx);
/* Layout invariant check (tests): the number of cells of the context's padded fields (wavefields, dt^2 c^2, the increment
 * field, the spare / recomputation pairs) that lie OUTSIDE the grid's interior -- halo planes and rows, the x halo a
 * row shares with the next, the look-ahead planes, the tail -- and are not exactly zero.  Every kernel relies on those
 * cells being zero and never writes them; anything but 0 here is a bug. */
int fwi_check_padding(fwi_ctx *ctx, int64_t *dirty_out);
/* Name of the stencil kernel the context dispatches to (static string). */
const char *fwi_kernel_name(const fwi_ctx *ctx);
/* Device count / name without creating a context (returns FWI_EHIP if none). */
int fwi_device_count(int32_t *n_out);

/* ---------------------------------------------------------------------------
 * the reference's REAL hot loop, batched over N source samples.
 * Steps 4-7 of PARALLEL_worker_mc_inv (full_waveform_inversion.py:713-774) for
 * given samples: forward_model (:253-264), compare_synth_to_real_waveforms
 * (:584-684) with one of the five similarity metrics (:512-582), the likelihood
 * map exp(-(1-s)/2) (:774) and the posterior normalisation (:847-848).  fp64 like
 * the reference; the samples are the caller's (fwi_mc_invert draws them on the device).
 *   green   (k, n, t)   Green's functions        data (k, t)   observed traces
 *   samples (n, nsamp)  source vectors, the reference's MTs[:, i] layout
 * Stateless: buffers are uploaded, scored and freed inside the call.
 * ------------------------------------------------------------------------- */
enum { FWI_MC_VR = 0, FWI_MC_CC = 1, FWI_MC_PCC = 2, FWI_MC_CCSHIFT = 3, FWI_MC_GAU = 4 };

int fwi_mc_score(int32_t device, int32_t k, int32_t n, int32_t t, int64_t nsamp, const double *green,
                 const double *data, const double *samples, int32_t metric, int32_t normalise,
                 int32_t all_at_once, double *similarity_out /* nsamp */,
                 double *likelihood_out /* nsamp or NULL */, double *posterior_out /* nsamp or NULL */,
                 double *kernel_ms_out /* or NULL */);

/* The whole loop body of PARALLEL_worker_mc_inv (:713-774) on the device, samplers included:
 * sample i = first_sample .. first_sample + nsamp - 1 of `inversion_type` is drawn by the
 * reference's generate_random_* map (:282-510) from counter-based deviates (Philox4x32-10 keyed by
 * `seed`, counter = sample index; a pure function of (seed, i), so ranks / calls can split a
 * run by index ranges), scaled by `amplitude` (M_amplitude, :741-760) and scored like
 * fwi_mc_score.  n must be the type's component count (6, 3 or 9).  samples_out (n, nsamp) and
 * frac_out (nsamp; the sampler's amplitude fraction, 0 for the uncoupled types) may be NULL when
 * only the scores are wanted -- then no sample ever crosses PCIe. */
enum {
    FWI_MC_FULL_MT = 0,                        /* generate_random_MT                              :282 */
    FWI_MC_DC = 1,                             /* generate_random_DC_MT                           :295 */
    FWI_MC_SINGLE_FORCE = 2,                   /* generate_random_single_force_vector             :320 */
    FWI_MC_DC_SINGLE_FORCE_COUPLE = 3,         /* generate_random_DC_single_force_coupled_tensor  :333 */
    FWI_MC_DC_SINGLE_FORCE_NO_COUPLING = 4,    /* generate_random_DC_single_force_uncoupled_tensor :369 */
    FWI_MC_DC_CRACK_COUPLE = 5,                /* generate_random_DC_crack_coupled_tensor         :384 */
    FWI_MC_SINGLE_FORCE_CRACK_NO_COUPLING = 6  /* generate_random_single_force_crack_uncoupled_tensor :448 */
};

int fwi_mc_invert(int32_t device, int32_t inversion_type, uint64_t seed, int64_t first_sample, int64_t nsamp,
                  double amplitude, int32_t k, int32_t n, int32_t t, const double *green, const double *data,
                  int32_t metric, int32_t normalise, int32_t all_at_once,
                  double *samples_out /* (n, nsamp) or NULL */, double *frac_out /* nsamp or NULL */,
                  double *similarity_out /* nsamp */, double *likelihood_out /* nsamp or NULL */,
                  double *posterior_out /* nsamp or NULL */, double *kernel_ms_out /* or NULL */);

/* A run in many blocks (N beyond one call's memory, or streamed): the plan keeps the Green's
 * functions, the data and every work buffer on the device, so each block costs its kernels and its
 * downloads only.  Blocks hold at most max_samples samples.  *like_sum_out receives the block's
 * sum of likelihoods; the posterior over the whole run is likelihood / (sum of the blocks'
 * like_sum) (:847-848), formed by the caller.  One plan per GPU, one host thread at a time. */
typedef struct fwi_mc_plan fwi_mc_plan;
int fwi_mc_plan_create(int32_t device, int32_t k, int32_t n, int32_t t, const double *green, const double *data,
                       int64_t max_samples, fwi_mc_plan **out);
void fwi_mc_plan_destroy(fwi_mc_plan *plan);
int fwi_mc_plan_invert(fwi_mc_plan *plan, int32_t inversion_type, uint64_t seed, int64_t first_sample,
                       int64_t nsamp, double amplitude, int32_t metric, int32_t normalise, int32_t all_at_once,
                       double *samples_out /* (n, nsamp) or NULL */, double *frac_out /* nsamp or NULL */,
                       double *similarity_out /* nsamp */, double *likelihood_out /* nsamp or NULL */,
                       double *like_sum_out /* or NULL */, double *kernel_ms_out /* or NULL */);
int fwi_mc_plan_score(fwi_mc_plan *plan, int64_t nsamp, const double *samples /* (n, nsamp) */, int32_t metric,
                      int32_t normalise, int32_t all_at_once, double *similarity_out, double *likelihood_out,
                      double *like_sum_out, double *kernel_ms_out);

/* The device sampler alone: samples_out (n, nsamp), frac_out (nsamp) or NULL. */
int fwi_mc_sample(int32_t device, int32_t inversion_type, uint64_t seed, int64_t first_sample, int64_t nsamp,
                  double amplitude, double *samples_out, double *frac_out);

/* forward_model for a batch: synth_out (nsamp, k, t).  [full_waveform_inversion.py:253-264] */
int fwi_mc_forward(int32_t device, int32_t k, int32_t n, int32_t t, int64_t nsamp, const double *green,
                   const double *samples, double *synth_out);

#ifdef __cplusplus
}
#endif
#endif /* FWI_H */
