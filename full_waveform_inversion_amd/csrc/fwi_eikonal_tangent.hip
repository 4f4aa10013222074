// The tangent of the first-arrival traveltimes on the device (fwi_eikonal_tangent.h; the definition is the NumPy twin,
// full_waveform_inversion_amd/eikonal.py).  A unit of its own: fwi_eikonal.o keeps its kernels, and both take the local
// solver from fwi_eikonal_device.h.  Nothing here touches the stepping kernels or their buffers.
#include "fwi_eikonal_tangent.h"

#include <math.h>

namespace fwi {

namespace {

#include "fwi_eikonal_device.h"

template <typename T>
__global__ __launch_bounds__(256) void eikonal_tangent_zero(T *x0, T *x1, int64_t npts) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npts) return;
    x0[i] = (T)0;
    x1[i] = (T)0;
}

// the source-determined listed nodes, by one thread in list order: x = dist[k] * ds[ref] in both arrays
template <typename T, int ND>
__global__ void eikonal_tangent_list(GridDesc g, const T *__restrict__ tim, const T *__restrict__ dm,
                                     const T *__restrict__ c, T *x0, T *x1, T h, int wrt_velocity, const int64_t *idx,
                                     const T *dist, int64_t ref, int cnt) {
#pragma clang fp contract(off)
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    int n[ND], p[ND];
    int64_t st[ND];
    eik_dims<ND>(g, n, st);
    const T dsr = eik_dslowness<T>(dm[ref], c[ref], wrt_velocity);
    for (int k = 0; k < cnt; ++k) {
        const int64_t gi = idx[k];
        int64_t r = gi;
        for (int d = 0; d < ND; ++d) {
            p[d] = (int)(r / st[d]);
            r -= (int64_t)p[d] * st[d];
        }
        T t[ND];
        bool lower[ND];
        eik_fetch<T, ND>(tim, n, st, p, gi, t, lower);
        if (tim[gi] < eik_local<T, ND>(t, ((T)1 / c[gi]) * h)) {
            const T v = dist[k] * dsr;
            x0[gi] = v;
            x1[gi] = v;
        }
    }
}

template <typename T, int ND>
__global__ __launch_bounds__(Eik<ND>::NT) void eikonal_tangent_sweep(GridDesc g, const T *__restrict__ tim,
                                                                     const T *__restrict__ dm,
                                                                     const T *__restrict__ in, T *__restrict__ out,
                                                                     const T *__restrict__ c, T h, int wrt_velocity,
                                                                     int K, int *flag) {
    eik_tangent_tile<T, ND, false>(g, tim, dm, nullptr, in, out, c, h, wrt_velocity, K, flag);
}

}  // namespace

template <typename T>
hipError_t launch_eikonal_tangent_init(const GridDesc &g, const T *t, const T *dm, const T *c, T *x0, T *x1, double h,
                                       int wrt_velocity, const int64_t *idx, const T *dist, int64_t ref, int n,
                                       hipStream_t s) {
    if (n <= 0 || x0 == x1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(eikonal_tangent_zero<T>, dim3(blocks256(g.npts)), dim3(256), 0, s, x0, x1, g.npts);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (g.ndim == 2)
        hipLaunchKernelGGL((eikonal_tangent_list<T, 2>), dim3(1), dim3(64), 0, s, g, t, dm, c, x0, x1, (T)h,
                           wrt_velocity, idx, dist, ref, n);
    else
        hipLaunchKernelGGL((eikonal_tangent_list<T, 3>), dim3(1), dim3(64), 0, s, g, t, dm, c, x0, x1, (T)h,
                           wrt_velocity, idx, dist, ref, n);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_eikonal_tangent_sweep(const GridDesc &g, const T *t, const T *dm, const T *in, T *out, const T *c,
                                        double h, int wrt_velocity, int K, int *flag, hipStream_t s) {
    if (K < 1 || K > EIK_KMAX || in == out) return hipErrorInvalidValue;
    if (g.ndim == 2)
        hipLaunchKernelGGL((eikonal_tangent_sweep<T, 2>), eik_grid<2>(g), dim3(Eik<2>::NT), 0, s, g, t, dm, in, out, c,
                           (T)h, wrt_velocity, K, flag);
    else
        hipLaunchKernelGGL((eikonal_tangent_sweep<T, 3>), eik_grid<3>(g), dim3(Eik<3>::NT), 0, s, g, t, dm, in, out, c,
                           (T)h, wrt_velocity, K, flag);
    return hipGetLastError();
}

#define EIK_INSTANTIATE(T)                                                                                            \
    template hipError_t launch_eikonal_tangent_init<T>(const GridDesc &, const T *, const T *, const T *, T *, T *,   \
                                                       double, int, const int64_t *, const T *, int64_t, int,         \
                                                       hipStream_t);                                                  \
    template hipError_t launch_eikonal_tangent_sweep<T>(const GridDesc &, const T *, const T *, const T *, T *,       \
                                                        const T *, double, int, int, int *, hipStream_t);
EIK_INSTANTIATE(float)
EIK_INSTANTIATE(double)
#undef EIK_INSTANTIATE

}  // namespace fwi
