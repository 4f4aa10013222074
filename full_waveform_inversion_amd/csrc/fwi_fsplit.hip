// The kernels of the tomographic / migration split on the Fourier store (fwi_fsplit.h).  Its own object: fwi_fimage.o,
// fwi_feximage.o, fwi_fourier.o and the step / tile / point objects keep their pinned kernel counts.
//
// The layout is that of fwi_fimage.hip: a thread owns 16 bytes of every compact volume (4 fp32 or 2 fp64 cells; a compact
// volume holds a multiple of 4 cells and starts 16-byte aligned), nothing is atomic, the frequencies are walked in
// ascending order with one fp64 sum per cell, and the weights and the taps sit at addresses that are the same in every
// lane, so they arrive through the scalar data cache.  Equal inputs give equal bits.
//
// The sum over k is kept in registers, so k is the outer loop and every (k, Re | Im) is one step: the workgroup stages
// the cells of Q and of M that its outputs need in LDS (its own cells and `R` halo cells on either side along the axis,
// zeros where the halo leaves the grid), forms HQ and HM of its cells from LDS, and meanwhile holds the next step's
// vectors in flight in registers.  Sum order, per cell, all in fp64 on the converted coefficients:
//   for k = 0 .. F - 1:
//     for c in (Re, Im):  hq = 0; hm = 0;
//                         for r = 1 .. R, t_r != 0:  hq = fma(t_r, Q_c(i - r) - Q_c(i + r), hq);   (hm likewise)
//                         Re: p = hq * hm; t = Q_c * M_c;     Im: p = fma(hq, hm, p); t = fma(Q_c, M_c, t);
//     s = fma(a_k, fma(beta, p, alpha * t), s)
//   dst = T(s)
// With alpha = 1/2 and beta = +-1/2 the inner fma is exactly (t +- p) / 2; with every tap zero p = 0 and both are t / 2.
//
// z and y (fsplit_march): a tap shift is a whole number of planes or rows, so every read is an aligned vector.  A
// workgroup of 8 x 32 threads owns 8 vectors (128 B) of the contiguous run by FSPLIT_CHUNK = 64 cells along the axis,
// two cells per thread; the LDS image is (CHUNK + 2 R) rows of 128 B for Q and for M, and a wave reads 8 consecutive
// rows, 1 KiB, per instruction.  Rows outside [0, n) are never addressed in memory: their LDS rows are zeros.
// x (fsplit_row): the filter crosses lanes.  A wave owns 64 vectors of one row; its LDS image is those cells with R
// cells on either side, the halo by element reads.  Every cell, halo cells included, is tested against 0 <= x < nx of
// the GRID in 64-bit arithmetic before an address is formed from it (the row pitch cx is nx rounded up to 4: the pad
// columns, and the cells of the neighbouring row behind them, are no cells of this row).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fwi_fsplit.h"
#include "fwi_fstore_device.h"

namespace fwi {

namespace {

constexpr int FSPLIT_BLOCK = 256;
constexpr int FSPLIT_LANES = 8;                                   // vectors of the contiguous run per staged row
constexpr int FSPLIT_PHASES = FSPLIT_BLOCK / FSPLIT_LANES;        // threads along the axis
constexpr int FSPLIT_CPT = FSPLIT_CHUNK / FSPLIT_PHASES;          // cells along the axis per thread
constexpr int FSPLIT_RPT = (FSPLIT_CHUNK + 2 * FSPLIT_RMAX + FSPLIT_PHASES - 1) / FSPLIT_PHASES;  // staged rows per thread
constexpr int FSPLIT_WAVES = FSPLIT_BLOCK / 64;
static_assert(FSPLIT_CHUNK % FSPLIT_PHASES == 0 && FSPLIT_RMAX <= 64, "tiling of fsplit_march / halo of fsplit_row");

using fstore::Pack;
using fstore::zero_pack;

// The per-step sums of one cell's V elements from its filtered (hq, hm) and own (qc, mc) coefficients.
template <typename T, int V>
__device__ __forceinline__ void fsplit_pair(bool im, const double *hq, const double *hm, const Pack<T, V> &qc,
                                            const Pack<T, V> &mc, double *p, double *t) {
#pragma unroll
    for (int e = 0; e < V; ++e) {
        const double qd = (double)qc.e[e], md = (double)mc.e[e];
        p[e] = im ? fma(hq[e], hm[e], p[e]) : hq[e] * hm[e];
        t[e] = im ? fma(qd, md, t[e]) : qd * md;
    }
}

// The volume as (outer, n, stride) elements: the filter runs along n, `stride` (ny cx along z, cx along y) is both the
// distance of two cells of the axis and the length of the contiguous run.  Workgroup b: chunk b % nchunk of the axis,
// tile (b / nchunk) % ntile of the run, outer index b / (nchunk ntile).
template <typename T, int V>
__global__ __launch_bounds__(FSPLIT_BLOCK) void fsplit_march(T *__restrict__ dst, const T *__restrict__ q,
                                                             const T *__restrict__ m, const double *__restrict__ a,
                                                             const double *__restrict__ taps, int64_t npts, int F, int n,
                                                             int64_t stride, int cx, int nx, int nchunk, int ntile, int R,
                                                             double alpha, double beta) {
    using P = Pack<T, V>;
    extern __shared__ __attribute__((aligned(16))) unsigned char fsplit_lds[];
    const int nrows = FSPLIT_CHUNK + 2 * R;
    P *lq = (P *)fsplit_lds, *lm = lq + nrows * FSPLIT_LANES;

    const int lane = threadIdx.x % FSPLIT_LANES, phase = threadIdx.x / FSPLIT_LANES;
    const int64_t b = blockIdx.x;
    const int chunk = (int)(b % nchunk), tile = (int)(b / nchunk % ntile);
    const int64_t outer = b / nchunk / ntile;
    const int64_t col = ((int64_t)tile * FSPLIT_LANES + lane) * V;  // first element of this thread's vector in the run
    const bool live = col < stride;                                 // (stride is a multiple of 4: whole vectors)
    const int64_t i0 = (int64_t)chunk * FSPLIT_CHUNK;               // first cell of the chunk along the axis
    const int64_t base = outer * n * stride + col;

    // staged row j of this thread: cell i0 - R + phase + j PHASES of the axis; bit j: it is a cell of the grid
    unsigned rows = 0;
    if (live) {
#pragma unroll
        for (int j = 0; j < FSPLIT_RPT; ++j) {
            const int64_t i = i0 - R + phase + (int64_t)j * FSPLIT_PHASES;
            if (phase + j * FSPLIT_PHASES < nrows && i >= 0 && i < n) rows |= 1u << j;
        }
    }
    P pq[FSPLIT_RPT], pm[FSPLIT_RPT];  // the next step's vectors, in flight under this step's sums
    const T *qs = q + base + (i0 - R + phase) * stride, *ms = m + base + (i0 - R + phase) * stride;
#pragma unroll
    for (int j = 0; j < FSPLIT_RPT; ++j) {
        pq[j] = pm[j] = zero_pack<T, V>();
        if (rows >> j & 1u) {
            pq[j] = *(const P *)(qs + (int64_t)j * FSPLIT_PHASES * stride);
            pm[j] = *(const P *)(ms + (int64_t)j * FSPLIT_PHASES * stride);
        }
    }

    double s[FSPLIT_CPT][V], p[FSPLIT_CPT][V], t[FSPLIT_CPT][V];
#pragma unroll
    for (int c = 0; c < FSPLIT_CPT; ++c)
#pragma unroll
        for (int e = 0; e < V; ++e) s[c][e] = p[c][e] = t[c][e] = 0.0;

#pragma unroll 1
    for (int step = 0; step < 2 * F; ++step) {  // step = 2 k + (0: Re, 1: Im)
        __syncthreads();                         // the sums of the step before have left LDS
#pragma unroll
        for (int j = 0; j < FSPLIT_RPT; ++j) {
            const int row = phase + j * FSPLIT_PHASES;
            if (row < nrows) {
                lq[row * FSPLIT_LANES + lane] = pq[j];
                lm[row * FSPLIT_LANES + lane] = pm[j];
            }
        }
        __syncthreads();
        if (step + 1 < 2 * F) {
            qs += npts;
            ms += npts;
#pragma unroll
            for (int j = 0; j < FSPLIT_RPT; ++j) {
                if (rows >> j & 1u) {
                    pq[j] = *(const P *)(qs + (int64_t)j * FSPLIT_PHASES * stride);
                    pm[j] = *(const P *)(ms + (int64_t)j * FSPLIT_PHASES * stride);
                }
            }
        }
        double hq[FSPLIT_CPT][V], hm[FSPLIT_CPT][V];
#pragma unroll
        for (int c = 0; c < FSPLIT_CPT; ++c)
#pragma unroll
            for (int e = 0; e < V; ++e) hq[c][e] = hm[c][e] = 0.0;
        const P *cq = lq + (R + phase) * FSPLIT_LANES + lane, *cm = lm + (R + phase) * FSPLIT_LANES + lane;
#pragma unroll 1
        for (int r = 1; r <= R; ++r) {
            const double tr = taps[r - 1];
            if (tr == 0.0) continue;
#pragma unroll
            for (int c = 0; c < FSPLIT_CPT; ++c) {
                const int lo = (c * FSPLIT_PHASES - r) * FSPLIT_LANES, hi = (c * FSPLIT_PHASES + r) * FSPLIT_LANES;
                const P ql = cq[lo], qh = cq[hi], ml = cm[lo], mh = cm[hi];
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    hq[c][e] = fma(tr, (double)ql.e[e] - (double)qh.e[e], hq[c][e]);
                    hm[c][e] = fma(tr, (double)ml.e[e] - (double)mh.e[e], hm[c][e]);
                }
            }
        }
        const bool im = step & 1;
#pragma unroll
        for (int c = 0; c < FSPLIT_CPT; ++c)
            fsplit_pair<T, V>(im, hq[c], hm[c], cq[c * FSPLIT_PHASES * FSPLIT_LANES], cm[c * FSPLIT_PHASES * FSPLIT_LANES],
                              p[c], t[c]);
        if (im) {
            const double ak = a[step >> 1];
#pragma unroll
            for (int c = 0; c < FSPLIT_CPT; ++c)
#pragma unroll
                for (int e = 0; e < V; ++e) s[c][e] = fma(ak, fma(beta, p[c][e], alpha * t[c][e]), s[c][e]);
        }
    }

    if (!live) return;
    const int x = (int)(col % cx);
#pragma unroll
    for (int c = 0; c < FSPLIT_CPT; ++c) {
        const int64_t i = i0 + phase + (int64_t)c * FSPLIT_PHASES;
        if (i >= n) continue;
        P d;
#pragma unroll
        for (int e = 0; e < V; ++e) d.e[e] = x + e < nx ? (T)s[c][e] : T(0);
        *(P *)(dst + base + i * stride) = d;
    }
}

// Wave w of workgroup b: work item b WAVES + w = row (item / nseg) of the nz ny compact rows, segment (item % nseg) of
// 64 V cells of it.
template <typename T, int V>
__global__ __launch_bounds__(FSPLIT_BLOCK) void fsplit_row(T *__restrict__ dst, const T *__restrict__ q,
                                                           const T *__restrict__ m, const double *__restrict__ a,
                                                           const double *__restrict__ taps, int64_t npts, int F, int cx,
                                                           int nx, int nseg, int64_t nitem, int R, double alpha,
                                                           double beta) {
    using P = Pack<T, V>;
    constexpr int SEG = 64 * V, LEN = SEG + 2 * FSPLIT_RMAX;  // (RMAX is a multiple of V: the own vectors stay aligned)
    __shared__ __attribute__((aligned(16))) T lq_all[FSPLIT_WAVES][LEN];
    __shared__ __attribute__((aligned(16))) T lm_all[FSPLIT_WAVES][LEN];
    const int lane = threadIdx.x % 64, wave = threadIdx.x / 64;
    T *lq = lq_all[wave], *lm = lm_all[wave];

    const int64_t item = (int64_t)blockIdx.x * FSPLIT_WAVES + wave;
    const bool work = item < nitem;
    const int64_t row = work ? item / nseg : 0;
    const int64_t x0 = work ? (item - row * nseg) * SEG : 0, x = x0 + (int64_t)lane * V;
    const bool live = work && x < cx;  // this thread's vector lies in the row pitch
    // the halo cells of this lane: x0 - 1 - lane on the left, x0 + SEG + lane on the right
    const int64_t xl = x0 - 1 - lane, xr = x0 + SEG + lane;
    const bool left = work && lane < R && xl >= 0 && xl < nx, right = work && lane < R && xr >= 0 && xr < nx;
    unsigned mask = 0;  // bit e: x + e is a cell of the grid
#pragma unroll
    for (int e = 0; e < V; ++e)
        if (live && x + e < nx) mask |= 1u << e;

    const T *qs = q + row * cx, *ms = m + row * cx;
    P pq = zero_pack<T, V>(), pm = pq;  // the next step's cells, in flight under this step's sums
    T pql = T(0), pqr = T(0), pml = T(0), pmr = T(0);
    if (mask) {
        pq = *(const P *)(qs + x);
        pm = *(const P *)(ms + x);
    }
    if (left) pql = qs[xl], pml = ms[xl];
    if (right) pqr = qs[xr], pmr = ms[xr];

    double s[V], p[V], t[V];
#pragma unroll
    for (int e = 0; e < V; ++e) s[e] = p[e] = t[e] = 0.0;

#pragma unroll 1
    for (int step = 0; step < 2 * F; ++step) {  // step = 2 k + (0: Re, 1: Im)
        __syncthreads();                         // the sums of the step before have left LDS
#pragma unroll
        for (int e = 0; e < V; ++e) {
            if (!(mask >> e & 1u)) pq.e[e] = pm.e[e] = T(0);  // pad columns count as outside the grid
        }
        *(P *)(lq + FSPLIT_RMAX + lane * V) = pq;
        *(P *)(lm + FSPLIT_RMAX + lane * V) = pm;
        if (lane < R) {
            lq[FSPLIT_RMAX - 1 - lane] = pql;
            lm[FSPLIT_RMAX - 1 - lane] = pml;
            lq[FSPLIT_RMAX + SEG + lane] = pqr;
            lm[FSPLIT_RMAX + SEG + lane] = pmr;
        }
        __syncthreads();
        if (step + 1 < 2 * F) {
            qs += npts;
            ms += npts;
            if (mask) {
                pq = *(const P *)(qs + x);
                pm = *(const P *)(ms + x);
            }
            if (left) pql = qs[xl], pml = ms[xl];
            if (right) pqr = qs[xr], pmr = ms[xr];
        }
        double hq[V], hm[V];
#pragma unroll
        for (int e = 0; e < V; ++e) hq[e] = hm[e] = 0.0;
        const T *cq = lq + FSPLIT_RMAX + lane * V, *cm = lm + FSPLIT_RMAX + lane * V;
#pragma unroll 1
        for (int r = 1; r <= R; ++r) {
            const double tr = taps[r - 1];
            if (tr == 0.0) continue;
#pragma unroll
            for (int e = 0; e < V; ++e) {
                hq[e] = fma(tr, (double)cq[e - r] - (double)cq[e + r], hq[e]);
                hm[e] = fma(tr, (double)cm[e - r] - (double)cm[e + r], hm[e]);
            }
        }
        const bool im = step & 1;
        fsplit_pair<T, V>(im, hq, hm, *(const P *)cq, *(const P *)cm, p, t);
        if (im) {
            const double ak = a[step >> 1];
#pragma unroll
            for (int e = 0; e < V; ++e) s[e] = fma(ak, fma(beta, p[e], alpha * t[e]), s[e]);
        }
    }

    if (!live) return;
    P d;
#pragma unroll
    for (int e = 0; e < V; ++e) d.e[e] = (mask >> e & 1u) ? (T)s[e] : T(0);
    *(P *)(dst + row * cx + x) = d;
}

}  // namespace

template <typename T>
hipError_t launch_fsplit(const GridDesc &g, T *dst, const T *q, const T *m, const double *a, int F, int axis,
                         const double *taps, int ntaps, double alpha, double beta, hipStream_t s) {
    constexpr int V = 16 / (int)sizeof(T);
    if (!fstore::volumes_ok<T>(g.npts, F, dst, q, m) || !a || !taps || g.cx % 4 != 0 || g.nx > g.cx || axis < 0 ||
        axis > 2 || g.npts != (int64_t)g.nz * g.ny * g.cx || ntaps < 0 || ntaps > FSPLIT_RMAX)
        return hipErrorInvalidValue;
    const int n = axis == 0 ? g.nz : axis == 1 ? g.ny : g.nx;
    if (ntaps >= std::max(n, 1)) return hipErrorInvalidValue;  // the caller drops the taps that touch nothing
    if (axis == 2) {
        const int nseg = (g.cx + 64 * V - 1) / (64 * V);
        const int64_t nitem = (int64_t)g.nz * g.ny * nseg, nblock = (nitem + FSPLIT_WAVES - 1) / FSPLIT_WAVES;
        if (nblock > INT32_MAX) return hipErrorInvalidValue;
        hipLaunchKernelGGL((fsplit_row<T, V>), dim3((unsigned)nblock), dim3(FSPLIT_BLOCK), 0, s, dst, q, m, a, taps, g.npts,
                           F, g.cx, g.nx, nseg, nitem, ntaps, alpha, beta);
        return hipGetLastError();
    }
    const int64_t stride = axis == 0 ? (int64_t)g.ny * g.cx : (int64_t)g.cx, outer = axis == 0 ? 1 : g.nz;
    const int64_t ntile = (stride / V + FSPLIT_LANES - 1) / FSPLIT_LANES;
    const int nchunk = (n + FSPLIT_CHUNK - 1) / FSPLIT_CHUNK;
    const int64_t nblock = outer * ntile * nchunk;
    if (ntile > INT32_MAX || nblock > INT32_MAX) return hipErrorInvalidValue;
    const size_t lds = (size_t)2 * (FSPLIT_CHUNK + 2 * ntaps) * FSPLIT_LANES * 16;
    hipLaunchKernelGGL((fsplit_march<T, V>), dim3((unsigned)nblock), dim3(FSPLIT_BLOCK), lds, s, dst, q, m, a, taps, g.npts,
                       F, n, stride, g.cx, g.nx, nchunk, (int)ntile, ntaps, alpha, beta);
    return hipGetLastError();
}

#define FWI_FSPLIT_INSTANTIATE(T)                                                                                    \
    template hipError_t launch_fsplit<T>(const GridDesc &, T *, const T *, const T *, const double *, int, int,      \
                                         const double *, int, double, double, hipStream_t);
FWI_FSPLIT_INSTANTIATE(float)
FWI_FSPLIT_INSTANTIATE(double)

}  // namespace fwi
