// The kernels of the extended images on the Fourier store (fwi_feximage.h).  Its own object: fwi_fimage.o, fwi_fourier.o
// and the step / tile / point objects keep their pinned kernel counts.
//
// One launch per lag, each a pure streaming pass in the layout of fwi_fimage.hip: a thread owns 16 bytes of every compact
// volume (4 fp32 or 2 fp64 cells; a compact volume holds a multiple of 4 cells and starts 16-byte aligned), nothing is
// shared and nothing is atomic, so equal inputs give equal bits.  The frequencies are walked one at a time in ascending
// order with one fp64 sum per cell, the next frequency's vectors in flight under the products of the current one; the
// weights sit at addresses that are the same in every lane, so they arrive through the scalar data cache and cost no
// vector register.  Sum order, per cell:
//   offset  s = 0; for k = 0 .. F - 1: t = Re Q_k(x-) * Re M_k(x+); t = fma(Im Q_k(x-), Im M_k(x+), t); s = fma(a_k, t, s);
//   lag     s = 0; for k = 0 .. F - 1: pr = fma(Im Q_k, Im M_k, Re Q_k * Re M_k);
//                                      pi = fma(Im Q_k, Re M_k, -(Re Q_k * Im M_k));
//                                      s = fma(C_k, pr, s); s = fma(D_k, pi, s);
//   then    dst = T(s)
// With h = 0, and with tau = 0 (C_k = a_k, D_k = 0), this is the image sum of fwi_fimage.hip operation for operation.
//
// The offset pass reads Q_k at x- = x - h e and M_k at x+ = x + h e.  A shift along z or y moves both reads by a whole
// number of compact rows or planes, a shift along x by a multiple of the thread's cells moves them by whole vectors: the
// reads stay aligned 16-byte vectors.  Any other shift along x takes element reads, which neighbouring lanes coalesce.
// The row end: the compact row pitch cx is nx rounded up to 4, so x - h or x + h can pass nx, and even cx, and land in the
// next row.  Every cell is therefore tested against the GRID's extent (0 <= x -+ h < n of the axis) before any address
// is formed from it; a thread none of whose cells passes reads nothing and writes zeros, and so do the pad columns.
#include <hip/hip_runtime.h>

#include "fwi_feximage.h"
#include "fwi_fstore_device.h"

namespace fwi {

namespace {

using namespace fstore;

// axis: 0 = z, 1 = y, 2 = x.  ELEM = false: h e is a whole number of vectors (any h along z or y, h % V == 0 along x).
template <typename T, int V, bool ELEM>
__global__ __launch_bounds__(BLOCK) void feximage_offset(GridDesc g, T *__restrict__ dst, const T *__restrict__ q,
                                                         const T *__restrict__ m, const double *__restrict__ a, int F,
                                                         int axis, int64_t h) {
    using P = Pack<T, V>;
    const int64_t npts = g.npts, sh = shift_elems(g, axis, h);
    const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = tid; i < npts / V; i += nthr) {
        const int64_t i0 = i * V, row = i0 / g.cx;  // row = z * ny + y
        const int x = (int)(i0 - row * g.cx);
        const unsigned mask = shift_mask<V>(g, row, x, axis, -h, h);
        if (mask == 0) {
            *(P *)(dst + i0) = zero_pack<T, V>();
            continue;
        }
        // (|h| < n from here on: sh is the shift in elements, and both shifted vectors lie inside the volume)
        double s[V];
#pragma unroll
        for (int e = 0; e < V; ++e) s[e] = 0.0;
        Walk<T, V, ELEM, true> w(q + i0 - sh, m + i0 + sh, npts, mask);
#pragma unroll 1
        for (int k = 0; k < F; ++k) {
            w.prefetch(k + 1 < F);
            const double ak = a[k];
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const double t = re_qconjm((double)w.qr.e[e], (double)w.qi.e[e], (double)w.mr.e[e], (double)w.mi.e[e]);
                s[e] = fma(ak, t, s[e]);
            }
            w.next();
        }
        P d;
#pragma unroll
        for (int e = 0; e < V; ++e) d.e[e] = (mask >> e & 1u) ? (T)s[e] : T(0);
        *(P *)(dst + i0) = d;
    }
}

template <typename T, int V>
__global__ __launch_bounds__(BLOCK) void feximage_lag(T *__restrict__ dst, const T *__restrict__ q,
                                                      const T *__restrict__ m, const double *__restrict__ cd,
                                                      int64_t npts, int F) {
    using P = Pack<T, V>;
    const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = tid; i < npts / V; i += nthr) {
        const int64_t i0 = i * V;
        double s[V];
#pragma unroll
        for (int e = 0; e < V; ++e) s[e] = 0.0;
        Walk<T, V, false, true> w(q + i0, m + i0, npts, 0u);
#pragma unroll 1
        for (int k = 0; k < F; ++k) {
            w.prefetch(k + 1 < F);
            const double ck = cd[k], dk = cd[F + k];
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const double qr = (double)w.qr.e[e], qi = (double)w.qi.e[e];
                const double mr = (double)w.mr.e[e], mi = (double)w.mi.e[e];
                const double pr = re_qconjm(qr, qi, mr, mi);
                const double pi = fma(qi, mr, -(qr * mi));
                s[e] = fma(ck, pr, s[e]);
                s[e] = fma(dk, pi, s[e]);
            }
            w.next();
        }
        P d;
#pragma unroll
        for (int e = 0; e < V; ++e) d.e[e] = (T)s[e];
        *(P *)(dst + i0) = d;
    }
}

}  // namespace

template <typename T>
hipError_t launch_feximage_offset(const GridDesc &g, T *dst, const T *q, const T *m, const double *a, int F, int axis,
                                  int64_t h, hipStream_t s) {
    constexpr int VEC = 16 / (int)sizeof(T);
    if (!volumes_ok<T>(g.npts, F, dst, q, m) || !a || g.cx % 4 != 0 || g.nx > g.cx || axis < 0 || axis > 2 ||
        g.npts != (int64_t)g.nz * g.ny * g.cx)
        return hipErrorInvalidValue;
    const dim3 grid(blocks(g.npts / VEC)), block(BLOCK);
    if (axis == 2 && h % VEC != 0)
        hipLaunchKernelGGL((feximage_offset<T, VEC, true>), grid, block, 0, s, g, dst, q, m, a, F, axis, h);
    else
        hipLaunchKernelGGL((feximage_offset<T, VEC, false>), grid, block, 0, s, g, dst, q, m, a, F, axis, h);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_feximage_lag(T *dst, const T *q, const T *m, const double *cd, int64_t npts, int F, hipStream_t s) {
    constexpr int VEC = 16 / (int)sizeof(T);
    if (!volumes_ok<T>(npts, F, dst, q, m) || !cd) return hipErrorInvalidValue;
    hipLaunchKernelGGL((feximage_lag<T, VEC>), dim3(blocks(npts / VEC)), dim3(BLOCK), 0, s, dst, q, m, cd, npts, F);
    return hipGetLastError();
}

#define FWI_FEXIMAGE_INSTANTIATE(T)                                                                                  \
    template hipError_t launch_feximage_offset<T>(const GridDesc &, T *, const T *, const T *, const double *, int, int, \
                                                  int64_t, hipStream_t);                                            \
    template hipError_t launch_feximage_lag<T>(T *, const T *, const T *, const double *, int64_t, int, hipStream_t);
FWI_FEXIMAGE_INSTANTIATE(float)
FWI_FEXIMAGE_INSTANTIATE(double)

}  // namespace fwi
