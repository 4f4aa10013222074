// Born modelling, generic path (fwi_born.h): the scattering source w q^n added to the Born field after each ordinary
// one-step launch.  Its own object: the step / tile / point objects keep their pinned kernel counts.
//
// Both kernels are bandwidth-bound element-wise passes, 16 bytes per lane: the scatter reads q^n (compact, once per
// sweep: streaming load, it must not evict the fields), w (compact, re-read every step) and read-modify-writes the
// padded field -- 16 B per point and step in fp32 (24 B in increment form, which updates v as well).
#include <algorithm>

#include "fwi_born.h"
#include "fwi_device.h"

namespace fwi {

namespace {

constexpr int BORN_BLOCK = 256;

template <typename T>
__global__ __launch_bounds__(BORN_BLOCK) void born_weight(const T *dm, const T *c, T *w, int wrt_velocity, int64_t n,
                                                          int nx, int cx) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        double v = 0.0;  // pad column (c = 0 there)
        if (cx == nx || (int)(i % cx) < nx) {
            const double cc = (double)c[i], d = (double)dm[i];
            v = wrt_velocity ? 2.0 * d / cc : -(cc * cc) * d;
        }
        w[i] = (T)v;
    }
}

// One thread per 16-byte vector of the compact layout (rows of cx elements, cx % 4 == 0: vectors never straddle rows,
// and the padded rows they map to start 16-byte aligned as well).
template <typename T, bool INC>
__global__ __launch_bounds__(BORN_BLOCK) void born_scatter(T *u, T *v, const T *q, const T *w, const T *dz, const T *dy,
                                                           const T *dx, int damp, GridDesc g, int nvec) {
    constexpr int VL = VecOf<T>::VL;
    const int i = blockIdx.x * BORN_BLOCK + threadIdx.x;
    if (i >= nvec) return;
    const int cxv = g.cx / VL;
    const int row = i / cxv, x0 = (i - row * cxv) * VL;
    const int z = row / g.ny, y = row - z * g.ny;
    const int64_t ci = (int64_t)row * g.cx + x0;
    const int64_t p = g.off0 + (int64_t)z * g.sz + (int64_t)y * g.sy + x0;
    // (q^n by streaming load: 100.7 against 101.7 us/step at 256^3 with a plain load, 120.4 against 122.6 in increment
    // form, profiles/r05_born_loads_ab.json; FWI_BORN_Q_PLAIN builds the plain form for the A/B)
#ifdef FWI_BORN_Q_PLAIN
    const vec<T> qv = ldv<T>(q + ci);
#else
    const vec<T> qv = ldv_stream<T>(q + ci);
#endif
    const vec<T> wv = ldv<T>(w + ci);
    vec<T> uv = ldv<T>(u + p);
    vec<T> vv;
    if (INC) vv = ldv<T>(v + p);
    T dzy = T(0);
    if (damp) dzy = dz[z];
#pragma unroll
    for (int j = 0; j < VL; ++j) {
        const int x = x0 + j;
        if (x >= g.nx) continue;  // pad column: a halo cell of the padded field, stays zero
        T add = wv.v[j] * qv.v[j];
        if (damp) {
            T d = dzy + dx[x];
            if (g.ndim == 3) d += dy[y];
            add = add / (T(1) + d);
        }
        uv.v[j] += add;
        if (INC) vv.v[j] += add;
    }
    stv<T>(u + p, uv);
    if (INC) stv<T>(v + p, vv);
}

}  // namespace

template <typename T>
hipError_t launch_born_weight(const GridDesc &g, const T *dm, const T *c, T *w, int wrt_velocity, hipStream_t s) {
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(2048, (g.npts + BORN_BLOCK - 1) / BORN_BLOCK));
    hipLaunchKernelGGL(born_weight<T>, dim3(blocks), dim3(BORN_BLOCK), 0, s, dm, c, w, wrt_velocity, g.npts, g.nx, g.cx);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_born_scatter(const GridDesc &g, T *u, T *v, const T *q, const T *w, const T *dz, const T *dy,
                               const T *dx, int damp, hipStream_t s) {
    const int64_t nvec = g.npts / VecOf<T>::VL;
    if (nvec <= 0) return hipSuccess;
    if (nvec > (int64_t)0x7fffffff - BORN_BLOCK) return hipErrorInvalidValue;
    const int blocks = (int)((nvec + BORN_BLOCK - 1) / BORN_BLOCK);
    if (v)
        hipLaunchKernelGGL((born_scatter<T, true>), dim3(blocks), dim3(BORN_BLOCK), 0, s, u, v, q, w, dz, dy, dx, damp, g,
                           (int)nvec);
    else
        hipLaunchKernelGGL((born_scatter<T, false>), dim3(blocks), dim3(BORN_BLOCK), 0, s, u, v, q, w, dz, dy, dx, damp, g,
                           (int)nvec);
    return hipGetLastError();
}

#define FWI_BORN_INSTANTIATE(T)                                                                                      \
    template hipError_t launch_born_weight<T>(const GridDesc &, const T *, const T *, T *, int, hipStream_t);        \
    template hipError_t launch_born_scatter<T>(const GridDesc &, T *, T *, const T *, const T *, const T *, const T *, \
                                               const T *, int, hipStream_t);
FWI_BORN_INSTANTIATE(float)
FWI_BORN_INSTANTIATE(double)

}  // namespace fwi
