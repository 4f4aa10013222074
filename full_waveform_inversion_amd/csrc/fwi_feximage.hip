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

#include <algorithm>

#include "fwi_feximage.h"

namespace fwi {

namespace {

constexpr int FEX_BLOCK = 256;

template <typename T, int V>
struct alignas(sizeof(T) * V) Pack {
    T e[V];
};

// the V cells at p: one vector read, or (ELEM) the cells of `mask` one by one, the others 0 and never addressed
template <typename T, int V, bool ELEM>
__device__ __forceinline__ Pack<T, V> fex_load(const T *__restrict__ p, unsigned mask) {
    using P = Pack<T, V>;
    if (!ELEM) return *(const P *)p;
    P r;
#pragma unroll
    for (int e = 0; e < V; ++e) r.e[e] = (mask >> e & 1u) ? p[e] : T(0);
    return r;
}

// axis: 0 = z, 1 = y, 2 = x.  ELEM = false: h e is a whole number of vectors (any h along z or y, h % V == 0 along x).
template <typename T, int V, bool ELEM>
__global__ __launch_bounds__(FEX_BLOCK) void feximage_offset(GridDesc g, T *__restrict__ dst, const T *__restrict__ q,
                                                             const T *__restrict__ m, const double *__restrict__ a,
                                                             int F, int axis, int64_t h) {
    using P = Pack<T, V>;
    const int64_t npts = g.npts;
    const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = tid; i < npts / V; i += nthr) {
        const int64_t i0 = i * V, row = i0 / g.cx;  // row = z * ny + y
        const int x = (int)(i0 - row * g.cx);
        unsigned mask = 0;  // bit e: cell x + e and both of its shifted cells lie in the grid
        if (axis == 2) {
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const int64_t lo = x + e - h, hi = x + e + h;
                if (lo >= 0 && lo < g.nx && hi >= 0 && hi < g.nx) mask |= 1u << e;
            }
        } else {
            const int64_t c = axis == 0 ? row / g.ny : row % g.ny, n = axis == 0 ? g.nz : g.ny;
            if (c - h >= 0 && c - h < n && c + h >= 0 && c + h < n) {
#pragma unroll
                for (int e = 0; e < V; ++e)
                    if (x + e < g.nx) mask |= 1u << e;
            }
        }
        P d;
        if (mask == 0) {
#pragma unroll
            for (int e = 0; e < V; ++e) d.e[e] = T(0);
            *(P *)(dst + i0) = d;
            continue;
        }
        // (|h| < n from here on: the shift in elements fits, and both shifted vectors lie inside the volume)
        const int64_t sh = h * (axis == 2 ? 1 : axis == 1 ? (int64_t)g.cx : (int64_t)g.ny * g.cx);
        const T *qk = q + i0 - sh, *mk = m + i0 + sh;  // Re, Im of frequency k: qk, qk + npts
        P qr0 = fex_load<T, V, ELEM>(qk, mask), qi0 = fex_load<T, V, ELEM>(qk + npts, mask);
        P mr0 = fex_load<T, V, ELEM>(mk, mask), mi0 = fex_load<T, V, ELEM>(mk + npts, mask);
        double s[V];
#pragma unroll
        for (int e = 0; e < V; ++e) s[e] = 0.0;
#pragma unroll 1
        for (int k = 0; k < F; ++k) {
            P qr1 = qr0, qi1 = qi0, mr1 = mr0, mi1 = mi0;  // the next frequency's vectors, in flight under this one's sums
            if (k + 1 < F) {
                qr1 = fex_load<T, V, ELEM>(qk + 2 * npts, mask);
                qi1 = fex_load<T, V, ELEM>(qk + 3 * npts, mask);
                mr1 = fex_load<T, V, ELEM>(mk + 2 * npts, mask);
                mi1 = fex_load<T, V, ELEM>(mk + 3 * npts, mask);
            }
            const double ak = a[k];
#pragma unroll
            for (int e = 0; e < V; ++e) {
                double t = (double)qr0.e[e] * (double)mr0.e[e];
                t = fma((double)qi0.e[e], (double)mi0.e[e], t);
                s[e] = fma(ak, t, s[e]);
            }
            qr0 = qr1;
            qi0 = qi1;
            mr0 = mr1;
            mi0 = mi1;
            qk += 2 * npts;
            mk += 2 * npts;
        }
#pragma unroll
        for (int e = 0; e < V; ++e) d.e[e] = (mask >> e & 1u) ? (T)s[e] : T(0);
        *(P *)(dst + i0) = d;
    }
}

template <typename T, int V>
__global__ __launch_bounds__(FEX_BLOCK) void feximage_lag(T *__restrict__ dst, const T *__restrict__ q,
                                                          const T *__restrict__ m, const double *__restrict__ cd,
                                                          int64_t npts, int F) {
    using P = Pack<T, V>;
    const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = tid; i < npts / V; i += nthr) {
        const int64_t i0 = i * V;
        const T *qk = q + i0, *mk = m + i0;  // Re, Im of frequency k: qk, qk + npts
        P qr0 = *(const P *)qk, qi0 = *(const P *)(qk + npts), mr0 = *(const P *)mk, mi0 = *(const P *)(mk + npts);
        double s[V];
#pragma unroll
        for (int e = 0; e < V; ++e) s[e] = 0.0;
#pragma unroll 1
        for (int k = 0; k < F; ++k) {
            P qr1 = qr0, qi1 = qi0, mr1 = mr0, mi1 = mi0;  // the next frequency's vectors, in flight under this one's sums
            if (k + 1 < F) {
                qr1 = *(const P *)(qk + 2 * npts);
                qi1 = *(const P *)(qk + 3 * npts);
                mr1 = *(const P *)(mk + 2 * npts);
                mi1 = *(const P *)(mk + 3 * npts);
            }
            const double ck = cd[k], dk = cd[F + k];
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const double qr = (double)qr0.e[e], qi = (double)qi0.e[e], mr = (double)mr0.e[e], mi = (double)mi0.e[e];
                const double pr = fma(qi, mi, qr * mr);
                const double pi = fma(qi, mr, -(qr * mi));
                s[e] = fma(ck, pr, s[e]);
                s[e] = fma(dk, pi, s[e]);
            }
            qr0 = qr1;
            qi0 = qi1;
            mr0 = mr1;
            mi0 = mi1;
            qk += 2 * npts;
            mk += 2 * npts;
        }
        P d;
#pragma unroll
        for (int e = 0; e < V; ++e) d.e[e] = (T)s[e];
        *(P *)(dst + i0) = d;
    }
}

int fex_blocks(int64_t work) {
    return (int)std::max<int64_t>(1, std::min<int64_t>(1 << 20, (work + FEX_BLOCK - 1) / FEX_BLOCK));
}

template <typename T>
bool fex_volumes_ok(const T *dst, const T *q, const T *m, const double *w, int64_t npts, int F) {
    constexpr int VEC = 16 / (int)sizeof(T);
    return npts > 0 && npts % VEC == 0 && F >= 1 && dst && q && m && w &&
           ((uintptr_t)dst | (uintptr_t)q | (uintptr_t)m) % 16 == 0;
}

}  // namespace

template <typename T>
hipError_t launch_feximage_offset(const GridDesc &g, T *dst, const T *q, const T *m, const double *a, int F, int axis,
                                  int64_t h, hipStream_t s) {
    constexpr int VEC = 16 / (int)sizeof(T);
    if (!fex_volumes_ok(dst, q, m, a, g.npts, F) || g.cx % 4 != 0 || g.nx > g.cx || axis < 0 || axis > 2 ||
        g.npts != (int64_t)g.nz * g.ny * g.cx)
        return hipErrorInvalidValue;
    const dim3 grid(fex_blocks(g.npts / VEC)), block(FEX_BLOCK);
    if (axis == 2 && h % VEC != 0)
        hipLaunchKernelGGL((feximage_offset<T, VEC, true>), grid, block, 0, s, g, dst, q, m, a, F, axis, h);
    else
        hipLaunchKernelGGL((feximage_offset<T, VEC, false>), grid, block, 0, s, g, dst, q, m, a, F, axis, h);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_feximage_lag(T *dst, const T *q, const T *m, const double *cd, int64_t npts, int F, hipStream_t s) {
    constexpr int VEC = 16 / (int)sizeof(T);
    if (!fex_volumes_ok(dst, q, m, cd, npts, F)) return hipErrorInvalidValue;
    hipLaunchKernelGGL((feximage_lag<T, VEC>), dim3(fex_blocks(npts / VEC)), dim3(FEX_BLOCK), 0, s, dst, q, m, cd, npts,
                       F);
    return hipGetLastError();
}

#define FWI_FEXIMAGE_INSTANTIATE(T)                                                                                  \
    template hipError_t launch_feximage_offset<T>(const GridDesc &, T *, const T *, const T *, const double *, int, int, \
                                                  int64_t, hipStream_t);                                            \
    template hipError_t launch_feximage_lag<T>(T *, const T *, const T *, const double *, int64_t, int, hipStream_t);
FWI_FEXIMAGE_INSTANTIATE(float)
FWI_FEXIMAGE_INSTANTIATE(double)

}  // namespace fwi
