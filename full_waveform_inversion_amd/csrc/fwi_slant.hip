// The kernel of the slant stack over vector slots (fwi_slant.h).  Its own object: every other object keeps its pinned
// kernel count.
//
// One streaming pass in the layout of the Fourier-store kernels (fwi_fstore_device.h): a thread owns 16 bytes of every
// compact volume (4 fp32 or 2 fp64 cells), nothing is shared and nothing is atomic, so equal inputs give equal bits.  A
// shift along z is a whole number of compact planes (rows in 2-D), so every read stays an aligned 16-byte vector and the
// two taps of a source are the same vector of two neighbouring planes.  The sources are separate allocations: their
// pointers, whole shifts and coefficients come by value in the kernel arguments and are read at addresses that are the
// same in every lane, through the scalar data cache.  The next source's two vectors are in flight under the sums of the
// current one.  Sum order, per cell, with one fp64 sum in registers:
//   s = 0; for i = 0 .. nsrc - 1:  s = fma(c0_i, src_i(z + n_i), s)        where 0 <= z + n_i < nz
//                                  s = fma(c1_i, src_i(z + n_i + 1), s)    where 0 <= z + n_i + 1 < nz and c1_i != 0
//   dst = T(beta == 0 ? s : fma(beta, dst, s))
// The row end of DESIGN.md s.4q, along z: a tap is tested against the GRID's extent, in 64-bit arithmetic, before any
// address is formed from it; one that fails is neither read nor counted.  The pad columns of dst are written as zeros.
#include <hip/hip_runtime.h>

#include "fwi_fstore_device.h"
#include "fwi_slant.h"

namespace fwi {

namespace {

using namespace fstore;

// the two taps of source k on the V cells from element i0 of plane z: read where the tap's plane is one of the grid
template <typename T, int V>
__device__ __forceinline__ void slant_taps(const SlantTable &t, int k, int64_t i0, int64_t z, int nz, int64_t plane,
                                           Pack<T, V> &a, Pack<T, V> &b, bool &va, bool &vb) {
    using P = Pack<T, V>;
    const int64_t za = z + t.n[k];
    va = za >= 0 && za < nz;
    vb = t.c1[k] != 0.0 && za + 1 >= 0 && za + 1 < nz;
    const T *p = (const T *)t.src[k] + i0;
    a = b = zero_pack<T, V>();
    if (va) a = *(const P *)(p + t.n[k] * plane);
    if (vb) b = *(const P *)(p + (t.n[k] + 1) * plane);
}

template <typename T, int V>
__global__ __launch_bounds__(BLOCK) void slant_sum(GridDesc g, T *__restrict__ dst, const SlantTable t, int nsrc,
                                                   double beta) {
    using P = Pack<T, V>;
    const int64_t npts = g.npts, plane = (int64_t)g.ny * g.cx;
    const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = tid; i < npts / V; i += nthr) {
        const int64_t i0 = i * V, row = i0 / g.cx, z = row / g.ny;  // row = z * ny + y
        const int x = (int)(i0 - row * g.cx);
        double s[V];
#pragma unroll
        for (int e = 0; e < V; ++e) s[e] = 0.0;
        P a, b, a1, b1;
        bool va = false, vb = false, va1, vb1;
        if (nsrc > 0) slant_taps<T, V>(t, 0, i0, z, g.nz, plane, a, b, va, vb);
#pragma unroll 1
        for (int k = 0; k < nsrc; ++k) {
            a1 = a, b1 = b, va1 = va, vb1 = vb;
            if (k + 1 < nsrc) slant_taps<T, V>(t, k + 1, i0, z, g.nz, plane, a1, b1, va1, vb1);
            const double c0 = t.c0[k], c1 = t.c1[k];
            if (va) {
#pragma unroll
                for (int e = 0; e < V; ++e) s[e] = fma(c0, (double)a.e[e], s[e]);
            }
            if (vb) {
#pragma unroll
                for (int e = 0; e < V; ++e) s[e] = fma(c1, (double)b.e[e], s[e]);
            }
            a = a1, b = b1, va = va1, vb = vb1;
        }
        P d;
        if (beta != 0.0) {
            const P old = *(const P *)(dst + i0);
#pragma unroll
            for (int e = 0; e < V; ++e) s[e] = fma(beta, (double)old.e[e], s[e]);
        }
#pragma unroll
        for (int e = 0; e < V; ++e) d.e[e] = x + e < g.nx ? (T)s[e] : T(0);
        *(P *)(dst + i0) = d;
    }
}

}  // namespace

template <typename T>
hipError_t launch_slant_sum(const GridDesc &g, T *dst, const SlantTable &t, int nsrc, double beta, hipStream_t s) {
    constexpr int VEC = 16 / (int)sizeof(T);
    if (!volumes_ok<T>(g.npts, 1, dst) || g.cx % 4 != 0 || g.nx > g.cx || nsrc < 0 || nsrc > SLANT_MAX ||
        g.npts != (int64_t)g.nz * g.ny * g.cx)
        return hipErrorInvalidValue;
    for (int k = 0; k < nsrc; ++k)
        if (!t.src[k] || (uintptr_t)t.src[k] % 16 != 0 || t.src[k] == (const void *)dst || t.n[k] < -(int64_t)g.nz - 1 ||
            t.n[k] > (int64_t)g.nz + 1)
            return hipErrorInvalidValue;
    hipLaunchKernelGGL((slant_sum<T, VEC>), dim3(blocks(g.npts / VEC)), dim3(BLOCK), 0, s, g, dst, t, nsrc, beta);
    return hipGetLastError();
}

template hipError_t launch_slant_sum<float>(const GridDesc &, float *, const SlantTable &, int, double, hipStream_t);
template hipError_t launch_slant_sum<double>(const GridDesc &, double *, const SlantTable &, int, double, hipStream_t);

}  // namespace fwi
