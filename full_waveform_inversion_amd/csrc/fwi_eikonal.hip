// First-arrival traveltimes and their discrete adjoint on the device (fwi_eikonal.h; the definition is the NumPy twin,
// full_waveform_inversion_amd/eikonal.py).  Nothing here touches the stepping kernels or their buffers.
#include "fwi_eikonal.h"

#include <math.h>

namespace fwi {

namespace {

#include "fwi_eikonal_device.h"

template <typename T>
__global__ __launch_bounds__(256) void eikonal_fill(GridDesc g, T *t) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= g.npts) return;
    t[i] = (int)(i % g.cx) < g.nx ? eik_inf<T>() : (T)0;
}

template <typename T>
__global__ __launch_bounds__(256) void eikonal_init(T *t0, T *t1, const T *c, const int64_t *idx, const T *dist,
                                                    int64_t ref, int n) {
#pragma clang fp contract(off)
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const T v = ((T)1 / c[ref]) * dist[k];
    t0[idx[k]] = v;
    t1[idx[k]] = v;
}

template <typename T, int ND>
__global__ __launch_bounds__(Eik<ND>::NT) void eikonal_sweep(GridDesc g, const T *__restrict__ in, T *__restrict__ out,
                                                             const T *__restrict__ c, T h, int K, int *flag) {
    eik_sweep_tile<T, ND, false>(g, in, out, c, nullptr, h, K, flag);
}

template <typename T, int ND>
__global__ __launch_bounds__(Eik<ND>::NT) void eikonal_adjoint_sweep(GridDesc g, const T *__restrict__ tim,
                                                                     const T *__restrict__ rhs,
                                                                     const T *__restrict__ in, T *__restrict__ out,
                                                                     const T *__restrict__ c, T h, int K, int *flag) {
#pragma clang fp contract(off)
    constexpr int TL = Eik<ND>::TL, NT = Eik<ND>::NT, P = TL + 2, PT = TL + 4;
    constexpr int NP = ND == 2 ? P * P : P * P * P, NPT = ND == 2 ? PT * PT : PT * PT * PT;
    __shared__ T sT[NPT];      // times, two cells around the tile
    __shared__ T sW[ND][NP];   // dG/dt_d of the tile and one cell around it, signed: > 0 the upwind neighbour is the
                               // lower one, < 0 the upper one, 0 the axis hands nothing on
    __shared__ T sL[NP];       // lambda, one frozen cell around the tile
    int n[ND], o[ND], l[ND];
    int64_t st[ND], gi;
    eik_dims<ND>(g, n, st);
    eik_origin<ND>(o);
    for (int i = threadIdx.x; i < NPT; i += NT) {
        eik_decode<ND>(i, PT, l);
        sT[i] = eik_cell<ND>(n, st, o, l, 2, gi) ? tim[gi] : eik_inf<T>();
    }
    __syncthreads();
    for (int i = threadIdx.x; i < NP; i += NT) {  // the local solver once per tile cell and halo cell
        eik_decode<ND>(i, P, l);
        const bool ok = eik_cell<ND>(n, st, o, l, 1, gi);
        T w[ND];
        bool lower[ND];
#pragma unroll
        for (int d = 0; d < ND; ++d) w[d] = (T)0, lower[d] = true;
        if (ok) {
            int lt = 0, s = 1, lts[ND];
            for (int d = ND - 1; d >= 0; --d) {
                lts[d] = s;
                lt += (l[d] + 1) * s;
                s *= PT;
            }
            T t[ND], den;
#pragma unroll
            for (int d = 0; d < ND; ++d) {
                const T lo = sT[lt - lts[d]], hi = sT[lt + lts[d]];
                t[d] = eik_min(lo, hi);
                lower[d] = lo <= hi;
            }
            eik_weights<T, ND>(sT[lt], t, ((T)1 / c[gi]) * h, w, den);
        }
#pragma unroll
        for (int d = 0; d < ND; ++d) sW[d][i] = lower[d] ? w[d] : -w[d];
        sL[i] = ok ? in[gi] : (T)0;
    }
    eik_decode<ND>(threadIdx.x, TL, l);
    const bool valid = eik_cell<ND>(n, st, o, l, 0, gi);
    int li = 0, ls[ND];
    {
        int s = 1;
        for (int d = ND - 1; d >= 0; --d) {
            ls[d] = s;
            li += (l[d] + 1) * s;
            s *= P;
        }
    }
    const T b = valid ? rhs[gi] : (T)0;
    __syncthreads();
    const T orig = sL[li];
    T cur = orig;
    for (int k = 0; k < K; ++k) {
        T acc = b;  // gather form, the terms in a fixed order: axis by axis, the lower neighbour first
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            const T wl = sW[d][li - ls[d]], wu = sW[d][li + ls[d]];
            if (wl < (T)0) acc = acc + (-wl) * sL[li - ls[d]];
            if (wu > (T)0) acc = acc + wu * sL[li + ls[d]];
        }
        __syncthreads();
        if (valid) sL[li] = acc, cur = acc;
        __syncthreads();
    }
    if (valid) out[gi] = cur;
    if (__syncthreads_or(valid && cur != orig) && threadIdx.x == 0) atomicMax(flag, 1);
}

template <typename T>
__device__ __forceinline__ T eik_convert(T gs, T cv, int wrt_velocity) {
#pragma clang fp contract(off)
    return wrt_velocity ? -gs / (cv * cv) : gs * cv / (T)2;
}

template <typename T, int ND>
__global__ __launch_bounds__(256) void eikonal_gradient(GridDesc g, const T *__restrict__ tim, const T *__restrict__ lam,
                                                        const T *__restrict__ c, T *out, T h, T beta, int wrt_velocity) {
#pragma clang fp contract(off)
    const int64_t gi = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gi >= g.npts) return;
    int n[ND], p[ND];
    int64_t st[ND];
    eik_dims<ND>(g, n, st);
    int64_t r = gi;
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        p[d] = (int)(r / st[d]);
        r -= (int64_t)p[d] * st[d];
    }
    if (p[ND - 1] >= g.nx) {  // pad column
        out[gi] = (T)0;
        return;
    }
    T t[ND], w[ND], den;
    bool lower[ND];
    eik_fetch<T, ND>(tim, n, st, p, gi, t, lower);
    const T cv = c[gi], s = (T)1 / cv;
    eik_weights<T, ND>(tim[gi], t, s * h, w, den);
    const T dGds = den > (T)0 ? s * h * h / den : (T)0;
    const T gm = eik_convert<T>(dGds * lam[gi], cv, wrt_velocity);
    out[gi] = beta == (T)0 ? gm : beta * out[gi] + gm;
}

// the source term, by one thread in list order
template <typename T, int ND>
__global__ void eikonal_source_term(GridDesc g, const T *__restrict__ tim, const T *__restrict__ lam,
                                    const T *__restrict__ c, T *out, T h, int wrt_velocity, const int64_t *idx,
                                    const T *dist, int64_t ref, int cnt) {
#pragma clang fp contract(off)
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    int n[ND], p[ND];
    int64_t st[ND];
    eik_dims<ND>(g, n, st);
    T acc = (T)0;
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
        if (tim[gi] < eik_local<T, ND>(t, ((T)1 / c[gi]) * h)) acc = acc + dist[k] * lam[gi];
    }
    out[ref] = out[ref] + eik_convert<T>(acc, c[ref], wrt_velocity);
}

template <typename T>
__global__ __launch_bounds__(256) void points_scale(T *x, int64_t npts, T beta) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < npts) x[i] = beta == (T)0 ? (T)0 : beta * x[i];
}

template <typename T>
__global__ __launch_bounds__(256) void points_add(T *x, const int64_t *idx, const T *v, int n) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k < n) x[idx[k]] = x[idx[k]] + v[k];
}

template <typename T>
__global__ __launch_bounds__(256) void points_gather(const T *x, const int64_t *idx, double *out, int n) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k < n) out[k] = (double)x[idx[k]];
}

}  // namespace

template <typename T>
hipError_t launch_eikonal_fill(const GridDesc &g, T *t, hipStream_t s) {
    hipLaunchKernelGGL(eikonal_fill<T>, dim3(blocks256(g.npts)), dim3(256), 0, s, g, t);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_eikonal_init(T *t0, T *t1, const T *c, const int64_t *idx, const T *dist, int64_t ref, int n,
                               hipStream_t s) {
    if (n <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(eikonal_init<T>, dim3(blocks256(n)), dim3(256), 0, s, t0, t1, c, idx, dist, ref, n);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_eikonal_sweep(const GridDesc &g, const T *in, T *out, const T *c, double h, int K, int *flag,
                                hipStream_t s) {
    if (K < 1 || K > EIK_KMAX || in == out) return hipErrorInvalidValue;
    if (g.ndim == 2)
        hipLaunchKernelGGL((eikonal_sweep<T, 2>), eik_grid<2>(g), dim3(Eik<2>::NT), 0, s, g, in, out, c, (T)h, K, flag);
    else
        hipLaunchKernelGGL((eikonal_sweep<T, 3>), eik_grid<3>(g), dim3(Eik<3>::NT), 0, s, g, in, out, c, (T)h, K, flag);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_eikonal_adjoint_sweep(const GridDesc &g, const T *t, const T *b, const T *in, T *out, const T *c,
                                        double h, int K, int *flag, hipStream_t s) {
    if (K < 1 || K > EIK_KMAX || in == out) return hipErrorInvalidValue;
    if (g.ndim == 2)
        hipLaunchKernelGGL((eikonal_adjoint_sweep<T, 2>), eik_grid<2>(g), dim3(Eik<2>::NT), 0, s, g, t, b, in, out, c,
                           (T)h, K, flag);
    else
        hipLaunchKernelGGL((eikonal_adjoint_sweep<T, 3>), eik_grid<3>(g), dim3(Eik<3>::NT), 0, s, g, t, b, in, out, c,
                           (T)h, K, flag);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_eikonal_gradient(const GridDesc &g, const T *t, const T *lam, const T *c, T *out, double h,
                                   double beta, int wrt_velocity, const int64_t *idx, const T *dist, int64_t ref, int n,
                                   hipStream_t s) {
    if (g.ndim == 2)
        hipLaunchKernelGGL((eikonal_gradient<T, 2>), dim3(blocks256(g.npts)), dim3(256), 0, s, g, t, lam, c, out, (T)h,
                           (T)beta, wrt_velocity);
    else
        hipLaunchKernelGGL((eikonal_gradient<T, 3>), dim3(blocks256(g.npts)), dim3(256), 0, s, g, t, lam, c, out, (T)h,
                           (T)beta, wrt_velocity);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || n <= 0) return e;
    if (g.ndim == 2)
        hipLaunchKernelGGL((eikonal_source_term<T, 2>), dim3(1), dim3(64), 0, s, g, t, lam, c, out, (T)h, wrt_velocity,
                           idx, dist, ref, n);
    else
        hipLaunchKernelGGL((eikonal_source_term<T, 3>), dim3(1), dim3(64), 0, s, g, t, lam, c, out, (T)h, wrt_velocity,
                           idx, dist, ref, n);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_scatter_points(T *x, int64_t npts, double beta, const int64_t *idx, const T *v, int n, hipStream_t s) {
    hipLaunchKernelGGL(points_scale<T>, dim3(blocks256(npts)), dim3(256), 0, s, x, npts, (T)beta);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || n <= 0) return e;
    hipLaunchKernelGGL(points_add<T>, dim3(blocks256(n)), dim3(256), 0, s, x, idx, v, n);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_gather_points(const T *x, const int64_t *idx, double *out, int n, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(points_gather<T>, dim3(blocks256(n)), dim3(256), 0, s, x, idx, out, n);
    return hipGetLastError();
}

#define EIK_INSTANTIATE(T)                                                                                           \
    template hipError_t launch_eikonal_fill<T>(const GridDesc &, T *, hipStream_t);                                  \
    template hipError_t launch_eikonal_init<T>(T *, T *, const T *, const int64_t *, const T *, int64_t, int,        \
                                               hipStream_t);                                                         \
    template hipError_t launch_eikonal_sweep<T>(const GridDesc &, const T *, T *, const T *, double, int, int *,     \
                                                hipStream_t);                                                        \
    template hipError_t launch_eikonal_adjoint_sweep<T>(const GridDesc &, const T *, const T *, const T *, T *,      \
                                                        const T *, double, int, int *, hipStream_t);                 \
    template hipError_t launch_eikonal_gradient<T>(const GridDesc &, const T *, const T *, const T *, T *, double,   \
                                                   double, int, const int64_t *, const T *, int64_t, int,            \
                                                   hipStream_t);                                                     \
    template hipError_t launch_scatter_points<T>(T *, int64_t, double, const int64_t *, const T *, int, hipStream_t); \
    template hipError_t launch_gather_points<T>(const T *, const int64_t *, double *, int, hipStream_t);
EIK_INSTANTIATE(float)
EIK_INSTANTIATE(double)
#undef EIK_INSTANTIATE

}  // namespace fwi
