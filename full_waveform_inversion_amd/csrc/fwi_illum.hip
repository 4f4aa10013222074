// Source-side illumination: a time-axis reduction of the stored forward term, and the vector operations of its
// preconditioner (fwi_illum.h).  Its own object: the step / tile / point objects keep their pinned kernel counts.
//
// The store already holds q^n = C (L u^n + src^n) ~ dt^2 d2u/dt2 for every imaging step (it is what the imaging
// condition correlates with), so H = (S / dt^4) sum_n (q^n)^2 costs one streaming pass over device-resident data and
// no extra wave propagation.  That pass is bandwidth-bound: 16 B per lane per slot, several slots in flight per
// thread, the sum of squares kept in fp64 registers, one read-modify-write of the accumulator per launch.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fwi_illum.h"

namespace fwi {

namespace {

constexpr int ILLUM_BLOCK = 256;
constexpr int ILLUM_INFLIGHT = 4;  // store slots loaded ahead of their use, per thread

// the 16-byte vector of one slot, squared into sum[0 .. 16 / element bytes)
template <typename T, bool QB>
struct Sq;

template <>
struct Sq<float, false> {
    static constexpr int VEC = 4;
    __device__ static void add(double *sum, uint4 v) {
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const double q = (double)__uint_as_float(w[e]);
            sum[e] = fma(q, q, sum[e]);
        }
    }
    __device__ static double elem(const void *p, int64_t i) { return (double)((const float *)p)[i]; }
};

template <>
struct Sq<float, true> {  // bf16: the upper half of an fp32 (q_elem in fwi_kernels.hip), element 2w in the low half
    static constexpr int VEC = 8;
    __device__ static void add(double *sum, uint4 v) {
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const double lo = (double)__uint_as_float(w[e] << 16), hi = (double)__uint_as_float(w[e] & 0xffff0000u);
            sum[2 * e] = fma(lo, lo, sum[2 * e]);
            sum[2 * e + 1] = fma(hi, hi, sum[2 * e + 1]);
        }
    }
    __device__ static double elem(const void *p, int64_t i) {
        return (double)__uint_as_float((unsigned)((const unsigned short *)p)[i] << 16);
    }
};

template <>
struct Sq<double, false> {
    static constexpr int VEC = 2;
    __device__ static void add(double *sum, uint4 v) {
        const double a = __hiloint2double((int)v.y, (int)v.x), b = __hiloint2double((int)v.w, (int)v.z);
        sum[0] = fma(a, a, sum[0]);
        sum[1] = fma(b, b, sum[1]);
    }
    __device__ static double elem(const void *p, int64_t i) { return ((const double *)p)[i]; }
};

template <typename T, bool QB>
__global__ __launch_bounds__(ILLUM_BLOCK) void illum_accumulate(T *acc, const char *store, int64_t npts, int nslots) {
    using S = Sq<T, QB>;
    constexpr int VEC = S::VEC;
    const size_t slot_bytes = (size_t)npts * (16 / VEC);
    const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
    if (npts % VEC == 0) {  // every slot starts 16-byte aligned
        for (int64_t i = tid; i < npts / VEC; i += nthr) {
            double sum[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) sum[e] = 0.0;
            const char *p = store + i * 16;
            int k = 0;
            for (; k + ILLUM_INFLIGHT <= nslots; k += ILLUM_INFLIGHT) {
                uint4 v[ILLUM_INFLIGHT];
#pragma unroll
                for (int j = 0; j < ILLUM_INFLIGHT; ++j) v[j] = *(const uint4 *)(p + (size_t)(k + j) * slot_bytes);
#pragma unroll
                for (int j = 0; j < ILLUM_INFLIGHT; ++j) S::add(sum, v[j]);
            }
            for (; k < nslots; ++k) S::add(sum, *(const uint4 *)(p + (size_t)k * slot_bytes));
            T *a = acc + i * VEC;
#pragma unroll
            for (int e = 0; e < VEC; ++e) a[e] = (T)((double)a[e] + sum[e]);
        }
    } else {  // (bf16 store of a grid with npts % 8 == 4: slots are only 8-byte aligned) one element per thread
        for (int64_t i = tid; i < npts; i += nthr) {
            double sum = 0.0;
            for (int k = 0; k < nslots; ++k) {
                const double q = S::elem(store + (size_t)k * slot_bytes, i);
                sum = fma(q, q, sum);
            }
            acc[i] = (T)((double)acc[i] + sum);
        }
    }
}

// One thread per grid node that carries a source entry (the first entry of that node does the work: entries of
// off-grid sources and duplicates share nodes, and (b + c)^2 is not linear in the entries).
__global__ void illum_source_bf16(float *acc, const unsigned short *store, int64_t npts, const float *wav,
                                  const int64_t *cidx, const float *cq, int nt, int nsrc, int stride) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nsrc) return;
    const int64_t node = cidx[i];
    for (int j = 0; j < i; ++j)
        if (cidx[j] == node) return;  // not the node's first entry
    double sum = 0.0;
    for (int n = 0; n < nt; n += stride) {
        double c = 0.0;
        for (int j = i; j < nsrc; ++j)
            if (cidx[j] == node) c += (double)cq[j] * (double)wav[(int64_t)n * nsrc + j];
        const double b = (double)__uint_as_float((unsigned)store[(size_t)(n / stride) * npts + node] << 16);
        sum += 2.0 * b * c + c * c;
    }
    acc[node] = (float)((double)acc[node] + sum);
}

template <typename T>
__global__ void illum_finalize(const T *acc, const T *c, T *out, double scale, int wrt_velocity, int64_t n, int nx,
                               int cx) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        double v = (double)acc[i] * scale;
        if (cx != nx && (int)(i % cx) >= nx) {
            v = 0.0;  // pad column (c = 0 there)
        } else if (wrt_velocity) {
            const double cc = (double)c[i], d = 2.0 / (cc * cc * cc);
            v *= d * d;
        }
        out[i] = (T)v;
    }
}

template <typename T>
__global__ void vec_mul_kernel(T *y, const T *x, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        y[i] = (T)((double)x[i] * (double)y[i]);
}

template <typename T>
__global__ void vec_recip_kernel(T *y, double a, double b, int64_t n, int nx, int cx) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        y[i] = (cx == nx || (int)(i % cx) < nx) ? (T)(a / ((double)y[i] + b)) : T(0);
}

int blocks_for(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(2048, (n + 255) / 256)); }

}  // namespace

template <typename T>
hipError_t launch_illum_accumulate(T *acc, const void *store, int64_t npts, int nslots, int q_bf16, hipStream_t s) {
    if (nslots <= 0 || npts <= 0) return hipSuccess;
    auto go = [&](auto kern, int vec) {
        const int64_t work = (npts % vec == 0) ? npts / vec : npts;
        const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(1 << 20, (work + ILLUM_BLOCK - 1) / ILLUM_BLOCK));
        hipLaunchKernelGGL(kern, dim3(blocks), dim3(ILLUM_BLOCK), 0, s, acc, (const char *)store, npts, nslots);
    };
    if constexpr (std::is_same<T, float>::value) {
        if (q_bf16)
            go(illum_accumulate<float, true>, 8);
        else
            go(illum_accumulate<float, false>, 4);
    } else {
        if (q_bf16) return hipErrorInvalidValue;
        go(illum_accumulate<double, false>, 2);
    }
    return hipGetLastError();
}

hipError_t launch_illum_source_bf16(float *acc, const void *store, int64_t npts, const float *wav, const int64_t *cidx,
                                    const float *cq, int nt, int nsrc, int stride, hipStream_t s) {
    if (nsrc <= 0 || nt <= 0) return hipSuccess;
    hipLaunchKernelGGL(illum_source_bf16, dim3((nsrc + 63) / 64), dim3(64), 0, s, acc, (const unsigned short *)store,
                       npts, wav, cidx, cq, nt, nsrc, stride < 1 ? 1 : stride);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_illum_finalize(const GridDesc &g, const T *acc, const T *c, T *out, double scale, int wrt_velocity,
                                 hipStream_t s) {
    hipLaunchKernelGGL(illum_finalize<T>, dim3(blocks_for(g.npts)), dim3(256), 0, s, acc, c, out, scale, wrt_velocity,
                       g.npts, g.nx, g.cx);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_vec_mul(const GridDesc &g, T *y, const T *x, hipStream_t s) {
    hipLaunchKernelGGL(vec_mul_kernel<T>, dim3(blocks_for(g.npts)), dim3(256), 0, s, y, x, g.npts);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_vec_recip(const GridDesc &g, T *y, double a, double b, hipStream_t s) {
    hipLaunchKernelGGL(vec_recip_kernel<T>, dim3(blocks_for(g.npts)), dim3(256), 0, s, y, a, b, g.npts, g.nx, g.cx);
    return hipGetLastError();
}

#define FWI_ILLUM_INSTANTIATE(T)                                                                                  \
    template hipError_t launch_illum_accumulate<T>(T *, const void *, int64_t, int, int, hipStream_t);            \
    template hipError_t launch_illum_finalize<T>(const GridDesc &, const T *, const T *, T *, double, int,         \
                                                 hipStream_t);                                                    \
    template hipError_t launch_vec_mul<T>(const GridDesc &, T *, const T *, hipStream_t);                         \
    template hipError_t launch_vec_recip<T>(const GridDesc &, T *, double, double, hipStream_t);
FWI_ILLUM_INSTANTIATE(float)
FWI_ILLUM_INSTANTIATE(double)

}  // namespace fwi
