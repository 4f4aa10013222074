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

#include <algorithm>

#include "fwi_fbornx.h"

namespace fwi {

namespace {

constexpr int FBX_BLOCK = 256;

template <typename T, int V>
struct alignas(sizeof(T) * V) Pack {
    T e[V];
};

// the V cells at p: one vector read, or (`elem`) the cells of `mask` one by one, the others 0 and never addressed
template <typename T, int V>
__device__ __forceinline__ Pack<T, V> fbx_load(const T *__restrict__ p, unsigned mask, bool elem) {
    using P = Pack<T, V>;
    if (!elem) return *(const P *)p;
    P r;
#pragma unroll
    for (int e = 0; e < V; ++e) r.e[e] = (mask >> e & 1u) ? p[e] : T(0);
    return r;
}

// axis: 0 = z, 1 = y, 2 = x.  ELEM = false: 2 h e is a whole number of vectors (any h along z or y, 2 h % V == 0 along x).
template <typename T, int V, bool ELEM>
__global__ __launch_bounds__(FBX_BLOCK) void fbornx_offset(GridDesc g, T *__restrict__ p, const T *__restrict__ q,
                                                           const T *__restrict__ img, int F, int axis, int64_t h,
                                                           int beta) {
    using P = Pack<T, V>;
    const int64_t npts = g.npts;
    const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = tid; i < npts / V; i += nthr) {
        const int64_t i0 = i * V, row = i0 / g.cx;  // row = z * ny + y
        const int x = (int)(i0 - row * g.cx);
        unsigned mask = 0;  // bit e: cell y = x + e and its shifted cells y - h, y - 2 h lie in the grid
        if (axis == 2) {
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const int64_t c1 = x + e - h, c2 = x + e - 2 * h;
                if (x + e < g.nx && c1 >= 0 && c1 < g.nx && c2 >= 0 && c2 < g.nx) mask |= 1u << e;
            }
        } else {
            const int64_t c = axis == 0 ? row / g.ny : row % g.ny, n = axis == 0 ? g.nz : g.ny;
            if (c - h >= 0 && c - h < n && c - 2 * h >= 0 && c - 2 * h < n) {
#pragma unroll
                for (int e = 0; e < V; ++e)
                    if (x + e < g.nx) mask |= 1u << e;
            }
        }
        T *pk = p + i0;  // Re, Im of frequency k: pk, pk + npts
        if (mask == 0) {
            if (!beta) {
                P z;
#pragma unroll
                for (int e = 0; e < V; ++e) z.e[e] = T(0);
                for (int k = 0; k < 2 * F; ++k) *(P *)(pk + k * npts) = z;
            }
            continue;
        }
        // (|2 h| < n from here on: the shifts in elements fit, and the shifted vectors lie inside the volume)
        const int64_t sh = h * (axis == 2 ? 1 : axis == 1 ? (int64_t)g.cx : (int64_t)g.ny * g.cx);
        const P ev = fbx_load<T, V>(img + i0 - sh, mask, axis == 2 && h % V != 0);
        const T *qk = q + i0 - 2 * sh;
        for (int k = 0; k < F; ++k) {
            const P qr = fbx_load<T, V>(qk, mask, ELEM), qi = fbx_load<T, V>(qk + npts, mask, ELEM);
            P pr, pi;
            if (beta) {
                pr = *(const P *)pk;
                pi = *(const P *)(pk + npts);
            } else {
#pragma unroll
                for (int e = 0; e < V; ++e) pr.e[e] = pi.e[e] = T(0);
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
__global__ __launch_bounds__(FBX_BLOCK) void fbornx_lag(T *__restrict__ p, const T *__restrict__ q,
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
            P pr, pi;
            if (beta) {
                pr = *(const P *)pk;
                pi = *(const P *)(pk + npts);
            } else {
#pragma unroll
                for (int e = 0; e < V; ++e) pr.e[e] = pi.e[e] = T(0);
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

int fbx_blocks(int64_t work) {
    return (int)std::max<int64_t>(1, std::min<int64_t>(1 << 20, (work + FBX_BLOCK - 1) / FBX_BLOCK));
}

template <typename T>
bool fbx_volumes_ok(const T *p, const T *q, const T *img, int64_t npts, int F) {
    constexpr int VEC = 16 / (int)sizeof(T);
    return npts > 0 && npts % VEC == 0 && F >= 1 && p && q && img && p != q &&
           ((uintptr_t)p | (uintptr_t)q | (uintptr_t)img) % 16 == 0;
}

}  // namespace

template <typename T>
hipError_t launch_fbornx_offset(const GridDesc &g, T *p, const T *q, const T *img, int F, int axis, int64_t h, int beta,
                                hipStream_t s) {
    constexpr int VEC = 16 / (int)sizeof(T);
    if (!fbx_volumes_ok(p, q, img, g.npts, F) || g.cx % 4 != 0 || g.nx > g.cx || axis < 0 || axis > 2 ||
        g.npts != (int64_t)g.nz * g.ny * g.cx || h > INT32_MAX || h < INT32_MIN)
        return hipErrorInvalidValue;
    const dim3 grid(fbx_blocks(g.npts / VEC)), block(FBX_BLOCK);
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
    if (!fbx_volumes_ok(p, q, img, npts, F) || !cs) return hipErrorInvalidValue;
    hipLaunchKernelGGL((fbornx_lag<T, VEC>), dim3(fbx_blocks(npts / VEC)), dim3(FBX_BLOCK), 0, s, p, q, img, cs, npts, F,
                       beta);
    return hipGetLastError();
}

#define FWI_FBORNX_INSTANTIATE(T)                                                                                     \
    template hipError_t launch_fbornx_offset<T>(const GridDesc &, T *, const T *, const T *, int, int, int64_t, int,  \
                                                hipStream_t);                                                         \
    template hipError_t launch_fbornx_lag<T>(T *, const T *, const T *, const double *, int64_t, int, int, hipStream_t);
FWI_FBORNX_INSTANTIATE(float)
FWI_FBORNX_INSTANTIATE(double)

}  // namespace fwi
