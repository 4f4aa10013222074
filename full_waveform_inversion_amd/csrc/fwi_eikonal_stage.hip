// Walled, slot-started eikonal solves, the handover between two stages and the stage tangent on the device
// (fwi_eikonal_stage.h; the definition is the NumPy twin, full_waveform_inversion_amd/eikonal.py).  A unit of its own:
// fwi_eikonal.o and fwi_eikonal_tangent.o keep their kernels, and all three take the local solver and the sweep bodies
// from fwi_eikonal_device.h.  Nothing here touches the stepping kernels or their buffers.
#include "fwi_eikonal_stage.h"

#include <math.h>

namespace fwi {

namespace {

#include "fwi_eikonal_device.h"

template <typename T>
__global__ __launch_bounds__(256) void eikonal_stage_check(GridDesc g, const T *__restrict__ t,
                                                           const T *__restrict__ wall, int *flags) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool bad = false, finite = false;
    if (i < g.npts && (int)(i % g.cx) < g.nx && !(wall && wall[i] != (T)0)) {
        const T v = t[i];
        bad = !(v >= (T)0);  // a NaN, a negative entry, -inf
        finite = v >= (T)0 && v < eik_inf<T>();
    }
    const int anybad = __syncthreads_or(bad), anyfinite = __syncthreads_or(finite);
    if (threadIdx.x == 0) {
        if (anybad) atomicMax(flags, 1);
        if (anyfinite) atomicMax(flags + 1, 1);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void eikonal_stage_start(GridDesc g, T *t0, T *t1, const T *__restrict__ wall) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= g.npts) return;
    T v = (T)0;
    if ((int)(i % g.cx) < g.nx) v = (wall && wall[i] != (T)0) ? eik_inf<T>() : t0[i];
    t0[i] = v;
    t1[i] = v;
}

template <typename T, int ND>
__global__ __launch_bounds__(Eik<ND>::NT) void eikonal_stage_sweep(GridDesc g, const T *__restrict__ in,
                                                                   T *__restrict__ out, const T *__restrict__ c,
                                                                   const T *__restrict__ wall, T h, int K, int *flag) {
    eik_sweep_tile<T, ND, true>(g, in, out, c, wall, h, K, flag);
}

// position of the compact index gi; false in a pad column
template <int ND>
__device__ __forceinline__ bool eik_position(const GridDesc &g, int64_t gi, const int64_t (&st)[ND], int (&p)[ND]) {
    int64_t r = gi;
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        p[d] = (int)(r / st[d]);
        r -= (int64_t)p[d] * st[d];
    }
    return p[ND - 1] < g.nx;
}

template <typename T, int ND>
__global__ __launch_bounds__(256) void eikonal_handover(GridDesc g, const T *__restrict__ tim, const T *__restrict__ in,
                                                        const T *__restrict__ c, T *out, T h, T beta) {
#pragma clang fp contract(off)
    const int64_t gi = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gi >= g.npts) return;
    int n[ND], p[ND];
    int64_t st[ND];
    eik_dims<ND>(g, n, st);
    if (!eik_position<ND>(g, gi, st, p)) {  // pad column
        out[gi] = (T)0;
        return;
    }
    T t[ND];
    bool lower[ND];
    eik_fetch<T, ND>(tim, n, st, p, gi, t, lower);
    const T Ti = tim[gi];
    const bool sd = Ti < eik_inf<T>() && Ti < eik_local<T, ND>(t, ((T)1 / c[gi]) * h);
    const T v = sd ? in[gi] : (T)0;
    out[gi] = beta == (T)0 ? v : beta * out[gi] + v;
}

template <typename T, int ND>
__global__ __launch_bounds__(256) void eikonal_stage_tangent_start(GridDesc g, const T *__restrict__ tim,
                                                                   const T *__restrict__ b0, const T *__restrict__ c,
                                                                   T *x0, T *x1, T h) {
#pragma clang fp contract(off)
    const int64_t gi = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gi >= g.npts) return;
    int n[ND], p[ND];
    int64_t st[ND];
    eik_dims<ND>(g, n, st);
    T v = (T)0;
    if (b0 && eik_position<ND>(g, gi, st, p)) {
        T t[ND], w[ND], den;
        bool lower[ND], live;
        eik_fetch<T, ND>(tim, n, st, p, gi, t, lower);
        eik_weights<T, ND>(tim[gi], t, ((T)1 / c[gi]) * h, w, den, live);
        if (!live) v = (T)0 + b0[gi];  // b_i = 0 there
    }
    x0[gi] = v;
    x1[gi] = v;
}

// the source-determined listed nodes, by one thread in list order: x = dist[k] * ds[ref] (+ b0) in both arrays
template <typename T, int ND>
__global__ void eikonal_stage_tangent_list(GridDesc g, const T *__restrict__ tim, const T *__restrict__ dm,
                                           const T *__restrict__ b0, const T *__restrict__ c, T *x0, T *x1, T h,
                                           int wrt_velocity, const int64_t *idx, const T *dist, int64_t ref, int cnt) {
#pragma clang fp contract(off)
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    int n[ND], p[ND];
    int64_t st[ND];
    eik_dims<ND>(g, n, st);
    const T dsr = eik_dslowness<T>(dm[ref], c[ref], wrt_velocity);
    for (int k = 0; k < cnt; ++k) {
        const int64_t gi = idx[k];
        eik_position<ND>(g, gi, st, p);
        T t[ND];
        bool lower[ND];
        eik_fetch<T, ND>(tim, n, st, p, gi, t, lower);
        if (tim[gi] < eik_local<T, ND>(t, ((T)1 / c[gi]) * h)) {
            T v = dist[k] * dsr;
            if (b0) v = v + b0[gi];
            x0[gi] = v;
            x1[gi] = v;
        }
    }
}

template <typename T, int ND>
__global__ __launch_bounds__(Eik<ND>::NT) void eikonal_stage_tangent_sweep(GridDesc g, const T *__restrict__ tim,
                                                                           const T *__restrict__ dm,
                                                                           const T *__restrict__ b0,
                                                                           const T *__restrict__ in,
                                                                           T *__restrict__ out, const T *__restrict__ c,
                                                                           T h, int wrt_velocity, int K, int *flag) {
    eik_tangent_tile<T, ND, true>(g, tim, dm, b0, in, out, c, h, wrt_velocity, K, flag);
}

}  // namespace

template <typename T>
hipError_t launch_eikonal_stage_check(const GridDesc &g, const T *t, const T *wall, int *flags, hipStream_t s) {
    hipLaunchKernelGGL(eikonal_stage_check<T>, dim3(blocks256(g.npts)), dim3(256), 0, s, g, t, wall, flags);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_eikonal_stage_start(const GridDesc &g, T *t0, T *t1, const T *wall, hipStream_t s) {
    if (t0 == t1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(eikonal_stage_start<T>, dim3(blocks256(g.npts)), dim3(256), 0, s, g, t0, t1, wall);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_eikonal_stage_sweep(const GridDesc &g, const T *in, T *out, const T *c, const T *wall, double h, int K,
                                      int *flag, hipStream_t s) {
    if (K < 1 || K > EIK_KMAX || in == out || !wall) return hipErrorInvalidValue;
    if (g.ndim == 2)
        hipLaunchKernelGGL((eikonal_stage_sweep<T, 2>), eik_grid<2>(g), dim3(Eik<2>::NT), 0, s, g, in, out, c, wall,
                           (T)h, K, flag);
    else
        hipLaunchKernelGGL((eikonal_stage_sweep<T, 3>), eik_grid<3>(g), dim3(Eik<3>::NT), 0, s, g, in, out, c, wall,
                           (T)h, K, flag);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_eikonal_handover(const GridDesc &g, const T *t, const T *in, const T *c, T *out, double h, double beta,
                                   hipStream_t s) {
    if (g.ndim == 2)
        hipLaunchKernelGGL((eikonal_handover<T, 2>), dim3(blocks256(g.npts)), dim3(256), 0, s, g, t, in, c, out, (T)h,
                           (T)beta);
    else
        hipLaunchKernelGGL((eikonal_handover<T, 3>), dim3(blocks256(g.npts)), dim3(256), 0, s, g, t, in, c, out, (T)h,
                           (T)beta);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_eikonal_stage_tangent_init(const GridDesc &g, const T *t, const T *dm, const T *b0, const T *c, T *x0,
                                             T *x1, double h, int wrt_velocity, const int64_t *idx, const T *dist,
                                             int64_t ref, int n, hipStream_t s) {
    if (x0 == x1) return hipErrorInvalidValue;
    if (g.ndim == 2)
        hipLaunchKernelGGL((eikonal_stage_tangent_start<T, 2>), dim3(blocks256(g.npts)), dim3(256), 0, s, g, t, b0, c,
                           x0, x1, (T)h);
    else
        hipLaunchKernelGGL((eikonal_stage_tangent_start<T, 3>), dim3(blocks256(g.npts)), dim3(256), 0, s, g, t, b0, c,
                           x0, x1, (T)h);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || n <= 0) return e;
    if (g.ndim == 2)
        hipLaunchKernelGGL((eikonal_stage_tangent_list<T, 2>), dim3(1), dim3(64), 0, s, g, t, dm, b0, c, x0, x1, (T)h,
                           wrt_velocity, idx, dist, ref, n);
    else
        hipLaunchKernelGGL((eikonal_stage_tangent_list<T, 3>), dim3(1), dim3(64), 0, s, g, t, dm, b0, c, x0, x1, (T)h,
                           wrt_velocity, idx, dist, ref, n);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_eikonal_stage_tangent_sweep(const GridDesc &g, const T *t, const T *dm, const T *b0, const T *in,
                                              T *out, const T *c, double h, int wrt_velocity, int K, int *flag,
                                              hipStream_t s) {
    if (K < 1 || K > EIK_KMAX || in == out || !b0) return hipErrorInvalidValue;
    if (g.ndim == 2)
        hipLaunchKernelGGL((eikonal_stage_tangent_sweep<T, 2>), eik_grid<2>(g), dim3(Eik<2>::NT), 0, s, g, t, dm, b0, in,
                           out, c, (T)h, wrt_velocity, K, flag);
    else
        hipLaunchKernelGGL((eikonal_stage_tangent_sweep<T, 3>), eik_grid<3>(g), dim3(Eik<3>::NT), 0, s, g, t, dm, b0, in,
                           out, c, (T)h, wrt_velocity, K, flag);
    return hipGetLastError();
}

#define EIK_INSTANTIATE(T)                                                                                            \
    template hipError_t launch_eikonal_stage_check<T>(const GridDesc &, const T *, const T *, int *, hipStream_t);    \
    template hipError_t launch_eikonal_stage_start<T>(const GridDesc &, T *, T *, const T *, hipStream_t);            \
    template hipError_t launch_eikonal_stage_sweep<T>(const GridDesc &, const T *, T *, const T *, const T *, double, \
                                                      int, int *, hipStream_t);                                       \
    template hipError_t launch_eikonal_handover<T>(const GridDesc &, const T *, const T *, const T *, T *, double,    \
                                                   double, hipStream_t);                                              \
    template hipError_t launch_eikonal_stage_tangent_init<T>(const GridDesc &, const T *, const T *, const T *,       \
                                                             const T *, T *, T *, double, int, const int64_t *,       \
                                                             const T *, int64_t, int, hipStream_t);                   \
    template hipError_t launch_eikonal_stage_tangent_sweep<T>(const GridDesc &, const T *, const T *, const T *,      \
                                                              const T *, T *, const T *, double, int, int, int *,     \
                                                              hipStream_t);
EIK_INSTANTIATE(float)
EIK_INSTANTIATE(double)
#undef EIK_INSTANTIATE

}  // namespace fwi
