// What the kernels on the Fourier store share (fwi_fourier.hip, fwi_fimage.hip, fwi_feximage.hip, fwi_fbornx.hip and
// fwi_fsplit.hip; no other file includes this): the 16-byte pack a thread owns of every compact volume, the launch
// geometry, the masked read, the test of shifted cells against the grid, the walk over the frequencies of Q_k and M_k
// and the argument check of the launchers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "fwi_kernels.h"

namespace fwi {
namespace fstore {

constexpr int BLOCK = 256;

// workgroups of a grid-stride pass over `work` threads' worth of cells
inline int blocks(int64_t work) {
    return (int)std::max<int64_t>(1, std::min<int64_t>(1 << 20, (work + BLOCK - 1) / BLOCK));
}

// `npts` cells are whole 16-byte vectors, and every volume of `v` exists and starts on one
template <typename T, typename... U>
bool volumes_ok(int64_t npts, int F, const U *...v) {
    constexpr int VEC = 16 / (int)sizeof(T);
    return npts > 0 && npts % VEC == 0 && F >= 1 && (... && v) && (... | (uintptr_t)v) % 16 == 0;
}

template <typename T, int V>
struct alignas(sizeof(T) * V) Pack {
    T e[V];
};

template <typename T, int V>
__device__ __forceinline__ Pack<T, V> zero_pack() {
    Pack<T, V> p;
#pragma unroll
    for (int e = 0; e < V; ++e) p.e[e] = T(0);
    return p;
}

// the V cells at p: one vector read, or (ELEM) the cells of `mask` one by one, the others 0 and never addressed
template <typename T, int V, bool ELEM>
__device__ __forceinline__ Pack<T, V> load(const T *__restrict__ p, unsigned mask) {
    using P = Pack<T, V>;
    if (!ELEM) return *(const P *)p;
    P r;
#pragma unroll
    for (int e = 0; e < V; ++e) r.e[e] = (mask >> e & 1u) ? p[e] : T(0);
    return r;
}

// Bit e: cell x + e of compact row `row` (= z * ny + y) is a grid cell, and so are the two cells `s1` and `s2` cells
// from it along `axis` (0 = z, 1 = y, 2 = x).  The compact row pitch cx is nx rounded up to 4, so a shifted cell can
// pass nx, and even cx, and land in the next row: every cell is tested against the GRID's extent, in 64-bit arithmetic,
// before any address is formed from it.
template <int V>
__device__ __forceinline__ unsigned shift_mask(const GridDesc &g, int64_t row, int x, int axis, int64_t s1, int64_t s2) {
    unsigned mask = 0;
    if (axis == 2) {
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const int64_t c1 = x + e + s1, c2 = x + e + s2;
            if (x + e < g.nx && c1 >= 0 && c1 < g.nx && c2 >= 0 && c2 < g.nx) mask |= 1u << e;
        }
    } else {
        const int64_t c = axis == 0 ? row / g.ny : row % g.ny, n = axis == 0 ? g.nz : g.ny;
        if (c + s1 >= 0 && c + s1 < n && c + s2 >= 0 && c + s2 < n) {
#pragma unroll
            for (int e = 0; e < V; ++e)
                if (x + e < g.nx) mask |= 1u << e;
        }
    }
    return mask;
}

// A shift of `h` cells along `axis`, in elements of a compact volume.  It is the same in every thread: form it once,
// above the loop over the cells (formed inside it, hipcc keeps one address per volume in vector registers).  The product
// wraps where |h| is far past the grid; it is used only where shift_mask passed a cell, and there |h| < n of the axis
// and it fits.
__device__ __forceinline__ int64_t shift_elems(const GridDesc &g, int axis, int64_t h) {
    const int64_t stride = axis == 2 ? 1 : axis == 1 ? (int64_t)g.cx : (int64_t)g.ny * g.cx;
    return (int64_t)((uint64_t)h * (uint64_t)stride);
}

// Re(Q conj M) of one cell.  Every image sum forms it here, so h = 0 and tau = 0 are the plain image bit for bit.
__device__ __forceinline__ double re_qconjm(double qr, double qi, double mr, double mi) {
    double t = qr * mr;
    t = fma(qi, mi, t);
    return t;
}

// The walk over the frequencies of Q_k and M_k on the V cells from q and m on (Re, Im of frequency k: qk, qk + npts):
//   Walk w(q, m, npts, mask);
//   for k = 0 .. F - 1, ascending:  w.prefetch(k + 1 < F);  sums on w.qr, w.qi (Re, Im Q_k), w.mr, w.mi (M_k);  w.next();
// prefetch puts the next frequency's vectors in flight under the caller's sums of the current one.  PAIR = false: m is
// not read and mr, mi hold nothing (the caller's M_k is Q_k).  The loop itself stays in the kernel: handed over as a
// callable, the sums made hipcc wait for the first prefetched vector before it issued the last two.
template <typename T, int V, bool ELEM, bool PAIR>
struct Walk {
    using P = Pack<T, V>;
    P qr, qi, mr, mi, qr1, qi1, mr1, mi1;
    const T *qk, *mk;
    int64_t npts;
    unsigned mask;

    __device__ __forceinline__ Walk(const T *q, const T *m, int64_t n, unsigned msk) : qk(q), mk(m), npts(n), mask(msk) {
        qr = load<T, V, ELEM>(qk, mask);
        qi = load<T, V, ELEM>(qk + npts, mask);
        if (PAIR) {
            mr = load<T, V, ELEM>(mk, mask);
            mi = load<T, V, ELEM>(mk + npts, mask);
        }
    }
    __device__ __forceinline__ void prefetch(bool more) {
        qr1 = qr, qi1 = qi;
        if (PAIR) mr1 = mr, mi1 = mi;
        if (more) {
            qr1 = load<T, V, ELEM>(qk + 2 * npts, mask);
            qi1 = load<T, V, ELEM>(qk + 3 * npts, mask);
            if (PAIR) {
                mr1 = load<T, V, ELEM>(mk + 2 * npts, mask);
                mi1 = load<T, V, ELEM>(mk + 3 * npts, mask);
            }
        }
    }
    __device__ __forceinline__ void next() {
        qr = qr1, qi = qi1;
        if (PAIR) mr = mr1, mi = mi1;
        qk += 2 * npts;
        mk += 2 * npts;
    }
};

}  // namespace fstore
}  // namespace fwi
