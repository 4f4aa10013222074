// The transforms of the Fourier-compressed forward-term store (fwi_fourier.h).  Its own object: the step / tile / point
// objects keep their pinned kernel counts.
//
// Both kernels are pure streaming passes over compact volumes: every cell belongs to one thread, nothing is shared and
// nothing is atomic, so equal inputs give equal bits.  A thread owns 16 bytes of every volume (4 fp32 or 2 fp64 cells;
// the <T, 1> variants, one cell per thread, serve a cell count that would leave the volumes unaligned).  It keeps one
// fp64 register set per sample of the batch (FOURIER_BMAX of them) and walks the frequencies one at a time, the next
// frequency's pair of accumulator vectors in flight under the sums of the current one: the 2 x FOURIER_BMAX twiddles of
// one frequency fill 32 scalar registers, and more than one frequency's worth of them spills.  The twiddles come from
// the table the host uploaded before the sweep: their address is the same in every lane, so they arrive through the
// scalar data cache (two 64-byte scalar loads per frequency) and cost no vector register.  Sum order, per cell:
//   analysis   s = 0; for b = 0 .. 7: s = fma(q_b, t_b, s) (q_b = 0 from nb on); then acc = T(double(acc) + s) for Re,
//              T(double(acc) - s) for Im, per k
//   synthesis  o_b = 0; for k = 0 .. F - 1: o_b = fma(Re_k, c_bk, o_b); o_b = fma(-Im_k, s_bk, o_b); then slot_b = T(o_b)
#include <hip/hip_runtime.h>

#include "fwi_fourier.h"
#include "fwi_fstore_device.h"

namespace fwi {

namespace {

using namespace fstore;

// slot of sample j0 + b, from j = slot0 + b with slot0 = j0 % ring_slots and b < ring_slots
__device__ __forceinline__ int ring_slot(int j, int ring_slots) { return j < ring_slots ? j : j - ring_slots; }

// the V cells from element i0 on
template <typename T, int V>
__device__ __forceinline__ void analyse_cells(T *__restrict__ acc, const T *__restrict__ ring, int64_t npts, int64_t i0,
                                              int ring_slots, int slot0, int j0, int nb, const double *__restrict__ tw,
                                              int tw_rows, int F) {
    using P = Pack<T, V>;
    double q[FOURIER_BMAX][V];
#pragma unroll
    for (int b = 0; b < FOURIER_BMAX; ++b) {
        P p = {};
        if (b < nb) p = *(const P *)(ring + (size_t)ring_slot(slot0 + b, ring_slots) * npts + i0);
#pragma unroll
        for (int e = 0; e < V; ++e) q[b][e] = (double)p.e[e];
    }
    T *a = acc + i0;  // Re Q_k, Im Q_k of frequency k: a, a + npts
    P re0 = *(const P *)a, im0 = *(const P *)(a + npts);
    const double *t = tw + (size_t)j0 * 2;  // frequency k: the rows j0 .. of its table, (cos, sin) pairs
#pragma unroll 1
    for (int k = 0; k < F; ++k, t += (size_t)tw_rows * 2) {
        P re1 = re0, im1 = im0;  // the next frequency's pair, in flight under this one's sums
        if (k + 1 < F) {
            re1 = *(const P *)(a + 2 * npts);
            im1 = *(const P *)(a + 3 * npts);
        }
        double re[V], im[V];
#pragma unroll
        for (int e = 0; e < V; ++e) re[e] = im[e] = 0.0;
#pragma unroll
        for (int b = 0; b < FOURIER_BMAX; ++b) {  // (b >= nb: q_b = 0, and the table has FOURIER_BMAX rows to spare)
            const double cs = t[2 * b], sn = t[2 * b + 1];
#pragma unroll
            for (int e = 0; e < V; ++e) {
                re[e] = fma(q[b][e], cs, re[e]);
                im[e] = fma(q[b][e], sn, im[e]);
            }
        }
#pragma unroll
        for (int e = 0; e < V; ++e) {
            re0.e[e] = (T)((double)re0.e[e] + re[e]);
            im0.e[e] = (T)((double)im0.e[e] - im[e]);
        }
        *(P *)a = re0;
        *(P *)(a + npts) = im0;
        re0 = re1;
        im0 = im1;
        a += 2 * npts;
    }
}

template <typename T, int V>
__device__ __forceinline__ void synthesise_cells(T *__restrict__ ring, const T *__restrict__ acc, int64_t npts,
                                                 int64_t i0, int ring_slots, int slot0, int j0, int nb,
                                                 const double *__restrict__ tw, int tw_rows, int F) {
    using P = Pack<T, V>;
    double o[FOURIER_BMAX][V];
#pragma unroll
    for (int b = 0; b < FOURIER_BMAX; ++b)
#pragma unroll
        for (int e = 0; e < V; ++e) o[b][e] = 0.0;
    const T *a = acc + i0;
    P re0 = *(const P *)a, im0 = *(const P *)(a + npts);
    const double *t = tw + (size_t)j0 * 2;  // frequency k: the rows j0 .. of its table, (cos, sin) pairs
#pragma unroll 1
    for (int k = 0; k < F; ++k, t += (size_t)tw_rows * 2) {
        P re1 = re0, im1 = im0;
        if (k + 1 < F) {
            re1 = *(const P *)(a + 2 * npts);
            im1 = *(const P *)(a + 3 * npts);
        }
        double re[V], im[V];
#pragma unroll
        for (int e = 0; e < V; ++e) {
            re[e] = (double)re0.e[e];
            im[e] = -(double)im0.e[e];
        }
#pragma unroll
        for (int b = 0; b < FOURIER_BMAX; ++b) {  // (b >= nb: formed from the table's spare rows, never stored)
            const double cs = t[2 * b], sn = t[2 * b + 1];
#pragma unroll
            for (int e = 0; e < V; ++e) {
                o[b][e] = fma(re[e], cs, o[b][e]);
                o[b][e] = fma(im[e], sn, o[b][e]);
            }
        }
        re0 = re1;
        im0 = im1;
        a += 2 * npts;
    }
#pragma unroll
    for (int b = 0; b < FOURIER_BMAX; ++b)
        if (b < nb) {
            P p;
#pragma unroll
            for (int e = 0; e < V; ++e) p.e[e] = (T)o[b][e];
            *(P *)(ring + (size_t)ring_slot(slot0 + b, ring_slots) * npts + i0) = p;
        }
}

// V cells per thread: 16 / sizeof(T) where every volume starts 16-byte aligned (npts % V == 0), else 1
template <typename T, int V>
__global__ __launch_bounds__(BLOCK) void fourier_analyse(T *acc, const T *ring, int64_t npts, int ring_slots, int slot0,
                                                         int j0, int nb, const double *tw, int tw_rows, int F) {
    const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = tid; i < npts / V; i += nthr)
        analyse_cells<T, V>(acc, ring, npts, i * V, ring_slots, slot0, j0, nb, tw, tw_rows, F);
}

template <typename T, int V>
__global__ __launch_bounds__(BLOCK) void fourier_synthesise(T *ring, const T *acc, int64_t npts, int ring_slots,
                                                            int slot0, int j0, int nb, const double *tw, int tw_rows,
                                                            int F) {
    const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = tid; i < npts / V; i += nthr)
        synthesise_cells<T, V>(ring, acc, npts, i * V, ring_slots, slot0, j0, nb, tw, tw_rows, F);
}

// either transform: `wide` with 16 / sizeof(T) cells per thread where npts allows it, else `one`; `out` is the volume
// set it writes (acc of the analysis, ring of the synthesis), `in` the one it reads
template <typename T>
using Transform = void (*)(T *, const T *, int64_t, int, int, int, int, const double *, int, int);

template <typename T>
hipError_t launch_transform(Transform<T> wide, Transform<T> one, T *out, const T *in, int64_t npts, int ring_slots,
                            int slot0, int j0, int nb, const double *tw, int tw_rows, int F, hipStream_t s) {
    constexpr int VEC = 16 / (int)sizeof(T);
    if (npts <= 0 || ring_slots < 1 || j0 < 0 || nb < 1 || nb > FOURIER_BMAX || nb > ring_slots || F < 1 ||
        j0 + FOURIER_BMAX > tw_rows || !out || !in || !tw)
        return hipErrorInvalidValue;
    const bool vec = npts % VEC == 0;
    hipLaunchKernelGGL(vec ? wide : one, dim3(blocks(vec ? npts / VEC : npts)), dim3(BLOCK), 0, s, out, in, npts,
                       ring_slots, slot0, j0, nb, tw, tw_rows, F);
    return hipGetLastError();
}

}  // namespace

template <typename T>
hipError_t launch_fourier_analyse(T *acc, const T *ring, int64_t npts, int ring_slots, int slot0, int j0, int nb,
                                  const double *tw, int tw_rows, int F, hipStream_t s) {
    return launch_transform<T>(fourier_analyse<T, 16 / (int)sizeof(T)>, fourier_analyse<T, 1>, acc, ring, npts, ring_slots,
                               slot0, j0, nb, tw, tw_rows, F, s);
}

template <typename T>
hipError_t launch_fourier_synthesise(T *ring, const T *acc, int64_t npts, int ring_slots, int slot0, int j0, int nb,
                                     const double *tw, int tw_rows, int F, hipStream_t s) {
    return launch_transform<T>(fourier_synthesise<T, 16 / (int)sizeof(T)>, fourier_synthesise<T, 1>, ring, acc, npts,
                               ring_slots, slot0, j0, nb, tw, tw_rows, F, s);
}

#define FWI_FOURIER_INSTANTIATE(T)                                                                                  \
    template hipError_t launch_fourier_analyse<T>(T *, const T *, int64_t, int, int, int, int, const double *, int,   \
                                                  int, hipStream_t);                                              \
    template hipError_t launch_fourier_synthesise<T>(T *, const T *, int64_t, int, int, int, int, const double *,     \
                                                     int, int, hipStream_t);
FWI_FOURIER_INSTANTIATE(float)
FWI_FOURIER_INSTANTIATE(double)

}  // namespace fwi
