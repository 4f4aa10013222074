// The kernels of spectral imaging on the Fourier store (fwi_fimage.h).  Its own object: fwi_fourier.o and the step / tile
// / point objects keep their pinned kernel counts.
//
// All three are pure streaming passes in the layout of the two transforms (fwi_fourier.hip): a thread owns 16 bytes of
// every compact volume (4 fp32 or 2 fp64 cells; a compact volume holds a multiple of 4 cells and starts 16-byte aligned),
// nothing is shared and nothing is atomic, so equal inputs give equal bits.  The image and the illumination walk the
// frequencies one at a time in ascending order with one fp64 sum per cell, the next frequency's vectors in flight under
// the products of the current one; the weight a_k sits at an address that is the same in every lane, so it arrives
// through the scalar data cache and costs no vector register.  Sum order, per cell:
//   image       s = 0; for k = 0 .. F - 1: t = Re Q_k * Re M_k; t = fma(Im Q_k, Im M_k, t); s = fma(a_k, t, s);
//   illuminate  s = 0; for k = 0 .. F - 1: t = Re Q_k * Re Q_k; t = fma(Im Q_k, Im Q_k, t); s = fma(a_k, t, s);
//   then        dst = T(s) (beta = 0) or T(double(dst) + s) (beta = 1)
#include <hip/hip_runtime.h>

#include "fwi_fimage.h"
#include "fwi_fstore_device.h"

namespace fwi {

namespace {

using namespace fstore;

// The V cells from compact element i0 on lie in one row (the row stride cx is a multiple of 4).  Where they are all grid
// cells and their padded address is 16-byte aligned they come in one vector read, else in V scalar reads, which
// neighbouring lanes coalesce.
template <typename T, int V>
__global__ __launch_bounds__(BLOCK) void fimage_pack(GridDesc g, const T *__restrict__ u, T *__restrict__ slot) {
    using P = Pack<T, V>;
    const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = tid; i < g.npts / V; i += nthr) {
        const int64_t i0 = i * V, row = i0 / g.cx;  // row = z * ny + y
        const int x = (int)(i0 - row * g.cx);
        const int z = (int)(row / g.ny), y = (int)(row % g.ny);
        const T *src = u + g.off0 + (int64_t)z * g.sz + (int64_t)y * g.sy + x;
        P p;
        if (x + V <= g.nx && (uintptr_t)src % sizeof(P) == 0) {
            p = *(const P *)src;  // (the padded row pitch is a multiple of 4 cells: most rows start aligned)
        } else {
#pragma unroll
            for (int e = 0; e < V; ++e) p.e[e] = x + e < g.nx ? src[e] : T(0);  // pad column of the compact layout
        }
        *(P *)(slot + i0) = p;
    }
}

// MODE 0: image (q and m), MODE 1: illuminate (q alone; m is not read)
template <typename T, int V, int MODE>
__global__ __launch_bounds__(BLOCK) void fimage_sum(T *__restrict__ dst, const T *__restrict__ q,
                                                    const T *__restrict__ m, const double *__restrict__ a, int64_t npts,
                                                    int F, int beta) {
    using P = Pack<T, V>;
    const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = tid; i < npts / V; i += nthr) {
        const int64_t i0 = i * V;
        double s[V];
#pragma unroll
        for (int e = 0; e < V; ++e) s[e] = 0.0;
        Walk<T, V, false, MODE == 0> w(q + i0, m + i0, npts, 0u);
#pragma unroll 1
        for (int k = 0; k < F; ++k) {
            w.prefetch(k + 1 < F);
            const P &mr = MODE == 0 ? w.mr : w.qr, &mi = MODE == 0 ? w.mi : w.qi;  // illuminate: M_k is Q_k
            const double ak = a[k];
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const double t = re_qconjm((double)w.qr.e[e], (double)w.qi.e[e], (double)mr.e[e], (double)mi.e[e]);
                s[e] = fma(ak, t, s[e]);
            }
            w.next();
        }
        P d;
        if (beta) {
            d = *(const P *)(dst + i0);
#pragma unroll
            for (int e = 0; e < V; ++e) d.e[e] = (T)((double)d.e[e] + s[e]);
        } else {
#pragma unroll
            for (int e = 0; e < V; ++e) d.e[e] = (T)s[e];
        }
        *(P *)(dst + i0) = d;
    }
}

template <typename T, int MODE>
hipError_t launch_sum(T *dst, const T *q, const T *m, const double *a, int64_t npts, int F, int beta, hipStream_t s) {
    constexpr int VEC = 16 / (int)sizeof(T);
    if (!volumes_ok<T>(npts, F, dst, q, m) || (beta != 0 && beta != 1) || !a) return hipErrorInvalidValue;
    hipLaunchKernelGGL((fimage_sum<T, VEC, MODE>), dim3(blocks(npts / VEC)), dim3(BLOCK), 0, s, dst, q, m, a, npts, F,
                       beta);
    return hipGetLastError();
}

}  // namespace

template <typename T>
hipError_t launch_fimage_pack(const GridDesc &g, const T *u, T *slot, hipStream_t s) {
    constexpr int VEC = 16 / (int)sizeof(T);
    if (g.npts <= 0 || g.cx % 4 != 0 || !u || !slot || (uintptr_t)slot % 16 != 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL((fimage_pack<T, VEC>), dim3(blocks(g.npts / VEC)), dim3(BLOCK), 0, s, g, u, slot);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_fimage_image(T *dst, const T *q, const T *m, const double *a, int64_t npts, int F, int beta,
                               hipStream_t s) {
    return launch_sum<T, 0>(dst, q, m, a, npts, F, beta, s);
}

template <typename T>
hipError_t launch_fimage_illuminate(T *dst, const T *q, const double *a, int64_t npts, int F, int beta, hipStream_t s) {
    return launch_sum<T, 1>(dst, q, q, a, npts, F, beta, s);
}

#define FWI_FIMAGE_INSTANTIATE(T)                                                                                  \
    template hipError_t launch_fimage_pack<T>(const GridDesc &, const T *, T *, hipStream_t);                       \
    template hipError_t launch_fimage_image<T>(T *, const T *, const T *, const double *, int64_t, int, int,        \
                                               hipStream_t);                                                        \
    template hipError_t launch_fimage_illuminate<T>(T *, const T *, const double *, int64_t, int, int, hipStream_t);
FWI_FIMAGE_INSTANTIATE(float)
FWI_FIMAGE_INSTANTIATE(double)

}  // namespace fwi
