// The kernels of extended Born modelling on the Fourier store (fwi_fbornx.h).  Its own object: fwi_feximage.o,
// fwi_fimage.o, fwi_fourier.o and the step / tile / point objects keep their pinned kernel counts.
//
// One launch per lag, each a pure streaming pass in the layout of fwi_feximage.hip: a thread owns 16 bytes of every
// compact volume (4 fp32 or 2 fp64 cells), nothing is shared and nothing is atomic, so equal inputs give equal bits.  The
// thread reads its cells of the image once and walks the frequencies in ascending order; the phases of the time-lag pass
// sit at addresses that are the same in every lane and arrive through the scalar data cache.
//
// The offset pass writes P_k(y) from E at y - h e and Q_k at y - 2 h e.  A shift along z or y moves a read by a whole
// number of compact rows or planes; along x, 2 h cells are a whole number of vectors whenever 2 h % V == 0 (every even h
// in fp32, every h in fp64), and then Q_k is read in aligned vectors, else cell by cell (neighbouring lanes coalesce).
// The single image volume is read in vectors where h % V == 0 and cell by cell otherwise.  The row end: the compact row
// pitch cx is nx rounded up to 4, so a shifted cell can pass nx, and even cx, and land in the next row.  Every cell is
// therefore tested against the GRID's extent in 64-bit arithmetic before any address is formed from it; a thread none of
// whose cells passes reads nothing and (first lag) writes zeros.
#include <hip/hip_runtime.h>

#include "fwi_fbornx.h"
#include "fwi_fstore_device.h"

namespace fwi {

namespace {

using namespace fstore;

// axis: 0 = z, 1 = y, 2 = x.  ELEM = false: 2 h e is a whole number of vectors (any h along z or y, 2 h % V == 0 along x).
template <typename T, int V, bool ELEM>
__global__ __launch_bounds__(BLOCK) void fbornx_offset(GridDesc g, T *__restrict__ p, const T *__restrict__ q,
                                                       const T *__restrict__ img, int F, int axis, int64_t h,
                                                       int beta) {
    using P = Pack<T, V>;
    const int64_t npts = g.npts, sh = shift_elems(g, axis, h);
    const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = tid; i < npts / V; i += nthr) {
        const int64_t i0 = i * V, row = i0 / g.cx;  // row = z * ny + y
        const int x = (int)(i0 - row * g.cx);
        const unsigned mask = shift_mask<V>(g, row, x, axis, -h, -2 * h);  // of the cells y = x + e: y - h, y - 2 h
        T *pk = p + i0;  // Re, Im of frequency k: pk, pk + npts
        if (mask == 0) {
            if (!beta)
                for (int k = 0; k < 2 * F; ++k) *(P *)(pk + k * npts) = zero_pack<T, V>();
            continue;
        }
        // (|2 h| < n from here on: sh and 2 sh are the shifts in elements, and the shifted vectors lie in the volume)
        const T *ek = img + i0 - sh, *qk = q + i0 - 2 * sh;
        const P ev = axis == 2 && h % V != 0 ? load<T, V, true>(ek, mask) : load<T, V, false>(ek, mask);
        for (int k = 0; k < F; ++k) {
            const P qr = load<T, V, ELEM>(qk, mask), qi = load<T, V, ELEM>(qk + npts, mask);
            P pr = zero_pack<T, V>(), pi = pr;
            if (beta) {
                pr = *(const P *)pk;
                pi = *(const P *)(pk + npts);
            }
#pragma unroll
            for (int e = 0; e < V; ++e) {
                if (!(mask >> e & 1u)) continue;
                const double ee = (double)ev.e[e];
                pr.e[e] = (T)fma(ee, (double)qr.e[e], (double)pr.e[e]);
                pi.e[e] = (T)fma(ee, (double)qi.e[e], (double)pi.e[e]);
            }
            *(P *)pk = pr;
            *(P *)(pk + npts) = pi;
            qk += 2 * npts;
            pk += 2 * npts;
        }
    }
}

template <typename T, int V>
__global__ __launch_bounds__(BLOCK) void fbornx_lag(T *__restrict__ p, const T *__restrict__ q,
                                                    const T *__restrict__ img, const double *__restrict__ cs,
                                                    int64_t npts, int F, int beta) {
    using P = Pack<T, V>;
    const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = tid; i < npts / V; i += nthr) {
        const int64_t i0 = i * V;
        const P ev = *(const P *)(img + i0);
        const T *qk = q + i0;  // Re, Im of frequency k: qk, qk + npts
        T *pk = p + i0;
        for (int k = 0; k < F; ++k) {
            const P qr = *(const P *)qk, qi = *(const P *)(qk + npts);
            P pr = zero_pack<T, V>(), pi = pr;
            if (beta) {
                pr = *(const P *)pk;
                pi = *(const P *)(pk + npts);
            }
            const double ck = cs[k], sk = cs[F + k];
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const double ee = (double)ev.e[e], r = (double)qr.e[e], m = (double)qi.e[e];
                pr.e[e] = (T)fma(ee, fma(m, sk, r * ck), (double)pr.e[e]);
                pi.e[e] = (T)fma(ee, fma(-r, sk, m * ck), (double)pi.e[e]);
            }
            *(P *)pk = pr;
            *(P *)(pk + npts) = pi;
            qk += 2 * npts;
            pk += 2 * npts;
        }
    }
}

}  // namespace

template <typename T>
hipError_t launch_fbornx_offset(const GridDesc &g, T *p, const T *q, const T *img, int F, int axis, int64_t h, int beta,
                                hipStream_t s) {
    constexpr int VEC = 16 / (int)sizeof(T);
    if (!volumes_ok<T>(g.npts, F, p, q, img) || p == q || g.cx % 4 != 0 || g.nx > g.cx || axis < 0 || axis > 2 ||
        g.npts != (int64_t)g.nz * g.ny * g.cx || h > INT32_MAX || h < INT32_MIN)
        return hipErrorInvalidValue;
    const dim3 grid(blocks(g.npts / VEC)), block(BLOCK);
    if (axis == 2 && (2 * h) % VEC != 0)
        hipLaunchKernelGGL((fbornx_offset<T, VEC, true>), grid, block, 0, s, g, p, q, img, F, axis, h, beta);
    else
        hipLaunchKernelGGL((fbornx_offset<T, VEC, false>), grid, block, 0, s, g, p, q, img, F, axis, h, beta);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_fbornx_lag(T *p, const T *q, const T *img, const double *cs, int64_t npts, int F, int beta,
                             hipStream_t s) {
    constexpr int VEC = 16 / (int)sizeof(T);
    if (!volumes_ok<T>(npts, F, p, q, img) || p == q || !cs) return hipErrorInvalidValue;
    hipLaunchKernelGGL((fbornx_lag<T, VEC>), dim3(blocks(npts / VEC)), dim3(BLOCK), 0, s, p, q, img, cs, npts, F, beta);
    return hipGetLastError();
}

#define FWI_FBORNX_INSTANTIATE(T)                                                                                     \
    template hipError_t launch_fbornx_offset<T>(const GridDesc &, T *, const T *, const T *, int, int, int64_t, int,  \
                                                hipStream_t);                                                         \
    template hipError_t launch_fbornx_lag<T>(T *, const T *, const T *, const double *, int64_t, int, int, hipStream_t);
FWI_FBORNX_INSTANTIATE(float)
FWI_FBORNX_INSTANTIATE(double)

}  // namespace fwi
