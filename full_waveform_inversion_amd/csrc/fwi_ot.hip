// Trace-by-trace optimal-transport (W2) misfit of (nt, ntr) trace gathers (fwi_ot.h): densities, normalised CDFs, the
// sorted searches behind the integer potentials, the dual sums and the adjoint source.  Its own object: the step / tile /
// point / smoothing / regularisation / data / matching / envelope / correlation / traveltime objects keep their pinned
// kernel counts.
//
// Everything here runs along the time axis of one trace, which is sequential by nature: a prefix sum and a search in a
// sorted array.  Lane = trace as in the shared gather tile (fwi_gather_tile.h), so every access of a wave to a gather at
// a common row is one run of consecutive addresses; what a thread owns besides its trace is one slice of consecutive
// times (fwi_ot.h ot_slice_len), which it walks in ascending order, a wave per slice and four slices per block.  The
// two prefix sums (the masses; the integer increments of the potentials) are each two-level: slice sums, their exclusive
// prefixes over ascending slices (ot_offsets), and a second walk that starts from the offset.  The search exploits that
// m+(n) and m-(n) do not decrease with n: one binary search per (slice, trace) and then a walk, nt + slices log2(nt)
// comparisons per trace instead of nt log2(nt).  Its loads follow the lane's own position in the other CDF and are the one
// access here that is not lane-contiguous; the lanes of a wave stay within a few rows of each other wherever neighbouring
// traces resemble each other.  No atomics and no LDS: every sum is added over ascending time within a slice and over the
// slices in ascending order, equal inputs give equal bits.  All arithmetic between the loads and the one rounding of g
// to T is fp64; the potentials are integers of magnitude <= 2 nt^2 carried in fp64, exactly.
#include <hip/hip_runtime.h>

#include "fwi_gather_tile.h"
#include "fwi_kernels.h"
#include "fwi_ot.h"

namespace fwi {

namespace {

constexpr int OT_BLOCK = GT_LANES * OT_BS;
constexpr int OT_PBLOCK = 256;
// the (slices, ntr) arrays of slice sums and the per-trace arrays of `work`, in the order of ot_work_doubles
enum { OT_P_P = 0, OT_P_Q, OT_P_BAD, OT_P_A, OT_P_B, OT_P_PHIF, OT_P_PSIG, OT_NPART };
enum { OT_T_SS = 0, OT_T_SD, OT_T_BAD, OT_T_A, OT_T_B, OT_T_COEF, OT_T_PHIBAR, OT_T_W, OT_NTRACE };
static_assert(OT_NPART == 7 && OT_NTRACE == 8, "ot_work_doubles counts them");

struct OtCell {
    int gx, sl;      // this thread's trace and slice
    int n_lo, n_hi;  // the slice's rows
    bool on;         // both exist
};

__device__ __forceinline__ OtCell ot_cell(int nt, int ntr, int slen, int slices) {
    OtCell c;
    c.gx = (int)blockIdx.x * GT_LANES + (int)(threadIdx.x & 63);
    c.sl = (int)blockIdx.y * OT_BS + (int)(threadIdx.x >> 6);
    c.on = c.gx < ntr && c.sl < slices;
    c.n_lo = c.sl * slen;
    c.n_hi = c.n_lo + slen < nt ? c.n_lo + slen : nt;
    return c;
}

__device__ __forceinline__ bool ot_proper(double v) { return v >= 0.0 && v < __builtin_huge_val(); }  // false for NaN

__device__ __forceinline__ double ot_positive(double x, int transform, double param) {
    if (transform == OT_LINEAR) return x + param;
    const double z = param * x;
    return (fmax(z, 0.0) + log1p(exp(-fabs(z)))) / param;
}

__device__ __forceinline__ double ot_slope(double x, int transform, double param) {
    if (transform == OT_LINEAR) return 1.0;
    const double e = exp(-fabs(param * x));
    return x >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
}

template <typename T>
__global__ __launch_bounds__(OT_BLOCK) void ot_density(double *p, double *q, double *part, const T *s, const T *d,
                                                       const T *w, int transform, double param, int nt, int ntr,
                                                       int slen, int slices) {
    const OtCell c = ot_cell(nt, ntr, slen, slices);
    if (!c.on) return;
    double sp = 0.0, sq = 0.0;
    int bad = 0;
    for (int n = c.n_lo; n < c.n_hi; ++n) {
        const int64_t at = (int64_t)n * ntr + c.gx;
        const double m = w ? (double)w[at] : 1.0;
        const double pv = ot_positive(m * (double)s[at], transform, param);
        const double qv = ot_positive(m * (double)d[at], transform, param);
        p[at] = pv, q[at] = qv;
        sp += pv, sq += qv;
        bad += !(ot_proper(pv) && ot_proper(qv));
    }
    const int64_t at = (int64_t)c.sl * ntr + c.gx, np = (int64_t)slices * ntr;
    part[OT_P_P * np + at] = sp;
    part[OT_P_Q * np + at] = sq;
    part[OT_P_BAD * np + at] = (double)bad;
}

// arrays blockIdx.y of part: the slice sums of a trace -> their exclusive prefixes over ascending slices; the total -> tot
__global__ __launch_bounds__(OT_PBLOCK) void ot_offsets(double *part, double *tot, int slices, int ntr) {
    const int j = (int)blockIdx.x * OT_PBLOCK + (int)threadIdx.x;
    if (j >= ntr) return;
    double *a = part + (int64_t)blockIdx.y * slices * ntr + j;
    double run = 0.0;
    for (int sl = 0; sl < slices; ++sl) {
        const double v = a[(int64_t)sl * ntr];
        a[(int64_t)sl * ntr] = run;
        run += v;
    }
    tot[(int64_t)blockIdx.y * ntr + j] = run;
}

// blockIdx.z = 0: F from p, 1: G from q
__global__ __launch_bounds__(OT_BLOCK) void ot_cdf(double *F, double *G, const double *p, const double *q,
                                                   const double *part, const double *tot, int nt, int ntr, int slen,
                                                   int slices) {
    const OtCell c = ot_cell(nt, ntr, slen, slices);
    if (!c.on) return;
    const int z = (int)blockIdx.z;
    const double *src = z ? q : p;
    double *dst = z ? G : F;
    const double off = part[((int64_t)z * slices + c.sl) * ntr + c.gx], S = tot[(int64_t)z * ntr + c.gx];
    double run = 0.0;
    for (int n = c.n_lo; n < c.n_hi; ++n) {
        const int64_t at = (int64_t)n * ntr + c.gx;
        run += src[at];
        dst[at] = (off + run) / S;
    }
}

// blockIdx.z = 0: a from the levels of F among G, 1: b from the levels of G among F.  Every loop is bounded by the
// index, whatever the values compare like (a trace that does not count may hold NaN).
__global__ __launch_bounds__(OT_BLOCK) void ot_search(double *a, double *b, double *part, const double *F,
                                                      const double *G, int nt, int ntr, int slen, int slices) {
    const OtCell c = ot_cell(nt, ntr, slen, slices);
    if (!c.on) return;
    const int z = (int)blockIdx.z, L = nt - 1;
    const double *X = (z ? G : F) + c.gx, *Y = (z ? F : G) + c.gx;
    double *out = (z ? b : a) + c.gx;
    double sum = 0.0;
    if (c.n_lo == 0) out[0] = 0.0;
    const int n0 = c.n_lo > 1 ? c.n_lo : 1;
    if (n0 < c.n_hi) {
        double y = X[(int64_t)(n0 - 1) * ntr];
        int lo = 0, hi = L;
        while (lo < hi) {  // m+: the first m in [0, L) with Y_m > y
            const int mid = (lo + hi) >> 1;
            if (Y[(int64_t)mid * ntr] <= y) lo = mid + 1; else hi = mid;
        }
        int mp = lo;
        lo = 0, hi = L;
        while (lo < hi) {  // m-: the first m in [0, L) with Y_m >= y
            const int mid = (lo + hi) >> 1;
            if (Y[(int64_t)mid * ntr] < y) lo = mid + 1; else hi = mid;
        }
        int mm = lo;
        for (int n = n0; n < c.n_hi; ++n) {
            if (n > n0) y = X[(int64_t)(n - 1) * ntr];
            while (mp < L && Y[(int64_t)mp * ntr] <= y) ++mp;
            while (mm < L && Y[(int64_t)mm * ntr] < y) ++mm;
            const double av = (double)(2 * n - 1 - mp - mm);
            out[(int64_t)n * ntr] = av;
            sum += av;
        }
    }
    part[((int64_t)(OT_P_A + z) * slices + c.sl) * ntr + c.gx] = sum;
}

// blockIdx.z = 0: phi (written over a) and the slice sums of phi f, 1: psi (not kept) and the slice sums of psi g
__global__ __launch_bounds__(OT_BLOCK) void ot_dual(double *a, const double *b, const double *p, const double *q,
                                                    double *part, const double *tot, int nt, int ntr, int slen,
                                                    int slices) {
    const OtCell c = ot_cell(nt, ntr, slen, slices);
    if (!c.on) return;
    const int z = (int)blockIdx.z;
    const double *inc = z ? b : a, *dens = z ? q : p;
    const double S = tot[(int64_t)(OT_T_SS + z) * ntr + c.gx];
    double run = part[((int64_t)(OT_P_A + z) * slices + c.sl) * ntr + c.gx], sum = 0.0;
    for (int n = c.n_lo; n < c.n_hi; ++n) {
        const int64_t at = (int64_t)n * ntr + c.gx;
        run += inc[at];
        if (!z) a[at] = run;
        sum = fma(run, dens[at] / S, sum);
    }
    part[((int64_t)(OT_P_PHIF + z) * slices + c.sl) * ntr + c.gx] = sum;
}

__global__ __launch_bounds__(OT_PBLOCK) void ot_finish(double *tot, int32_t *counts, double *jterm, const double *part,
                                                       const double *tw, double dt, int slices, int ntr) {
    const int j = (int)blockIdx.x * OT_PBLOCK + (int)threadIdx.x;
    if (j >= ntr) return;
    const int64_t np = (int64_t)slices * ntr;
    double sphi = 0.0, spsi = 0.0;
    for (int sl = 0; sl < slices; ++sl) {
        sphi += part[OT_P_PHIF * np + (int64_t)sl * ntr + j];
        spsi += part[OT_P_PSIG * np + (int64_t)sl * ntr + j];
    }
    const double Ss = tot[(int64_t)OT_T_SS * ntr + j], Sd = tot[(int64_t)OT_T_SD * ntr + j];
    const bool ok = tot[(int64_t)OT_T_BAD * ntr + j] == 0.0 && Ss > 0.0 && ot_proper(Ss) && Sd > 0.0 && ot_proper(Sd);
    const double wj = tw ? tw[j] : 1.0, dt2 = dt * dt;
    const double W = ok ? dt2 * (sphi + spsi) : 0.0;
    tot[(int64_t)OT_T_COEF * ntr + j] = ok ? 0.5 * wj * dt2 / Ss : 0.0;
    tot[(int64_t)OT_T_PHIBAR * ntr + j] = ok ? sphi : 0.0;
    tot[(int64_t)OT_T_W * ntr + j] = W;
    jterm[j] = 0.5 * wj * W;
    counts[j] = ok ? 1 : 0;
}

template <typename T>
__global__ __launch_bounds__(OT_BLOCK) void ot_source(T *g, const T *s, const T *w, const double *phi,
                                                      const double *tot, int transform, double param, int nt, int ntr,
                                                      int slen, int slices) {
    const OtCell c = ot_cell(nt, ntr, slen, slices);
    if (!c.on) return;
    const double coef = tot[(int64_t)OT_T_COEF * ntr + c.gx], phibar = tot[(int64_t)OT_T_PHIBAR * ntr + c.gx];
    for (int n = c.n_lo; n < c.n_hi; ++n) {
        const int64_t at = (int64_t)n * ntr + c.gx;
        const double m = w ? (double)w[at] : 1.0;
        double v = 0.0;  // a trace that does not count (or weighs nothing): whatever its samples are
        if (coef != 0.0) v = m * (coef * (phi[at] - phibar) * ot_slope(m * (double)s[at], transform, param));
        g[at] = (T)v;
    }
}

}  // namespace

template <typename T>
hipError_t launch_ot_misfit(double *work, int32_t *counts, T *g, const T *s, const T *d, const T *w, const double *tw,
                            int transform, double param, double dt, int nt, int ntr, hipStream_t st) {
    if (!work || !counts || !g || !s || !d || nt < 1 || ntr < 1 || g == w ||
        (transform != OT_LINEAR && transform != OT_SOFTPLUS))
        return hipErrorInvalidValue;
    const int slen = ot_slice_len(nt, ntr), slices = ot_slices(nt, ntr);
    const size_t n = (size_t)nt * ntr, np = (size_t)slices * ntr;
    double *p = work, *q = p + n, *F = q + n, *G = F + n, *a = G + n, *b = a + n;
    double *part = b + n, *tot = part + OT_NPART * np, *jterm = tot + (size_t)OT_NTRACE * ntr;
    const unsigned xt = (unsigned)gather_xtiles(ntr), yb = (unsigned)((slices + OT_BS - 1) / OT_BS);
    const unsigned pb = (unsigned)((ntr + OT_PBLOCK - 1) / OT_PBLOCK);
    const dim3 one(xt, yb, 1), two(xt, yb, 2), blk(OT_BLOCK);
    hipError_t e;
    hipLaunchKernelGGL(ot_density<T>, one, blk, 0, st, p, q, part, s, d, w, transform, param, nt, ntr, slen, slices);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(ot_offsets, dim3(pb, 3), dim3(OT_PBLOCK), 0, st, part, tot, slices, ntr);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(ot_cdf, two, blk, 0, st, F, G, p, q, part, tot, nt, ntr, slen, slices);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(ot_search, two, blk, 0, st, a, b, part, F, G, nt, ntr, slen, slices);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(ot_offsets, dim3(pb, 2), dim3(OT_PBLOCK), 0, st, part + OT_P_A * np, tot + (size_t)OT_T_A * ntr,
                       slices, ntr);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(ot_dual, two, blk, 0, st, a, b, p, q, part, tot, nt, ntr, slen, slices);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(ot_finish, dim3(pb), dim3(OT_PBLOCK), 0, st, tot, counts, jterm, part, tw, dt, slices, ntr);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = launch_sum_partials(jterm, ntr, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(ot_source<T>, one, blk, 0, st, g, s, w, a, tot, transform, param, nt, ntr, slen, slices);
    return hipGetLastError();
}

template hipError_t launch_ot_misfit<float>(double *, int32_t *, float *, const float *, const float *, const float *,
                                            const double *, int, double, double, int, int, hipStream_t);
template hipError_t launch_ot_misfit<double>(double *, int32_t *, double *, const double *, const double *,
                                             const double *, const double *, int, double, double, int, int, hipStream_t);

}  // namespace fwi
