// Separable Gaussian smoothing of compact model-sized vectors (fwi_smooth.h).  Its own object: the step / tile / point
// objects keep their pinned kernel counts.
//
// One launch is one axis.  Each pass reads its input from HBM once, apart from the halos of its tiles, and writes its
// output once, in 16-byte lanes along x:
//   x pass    one wave per row segment of 64 lanes; the segment and 2 R halo cells (mirrored against nx while they are
//             staged) sit in LDS, every lane reads its window of V + 2 R cells back as aligned 16-byte vectors.
//   y/z pass  a tile of 64 rows x 16 lanes (256 B of x) plus 2 R mirrored halo rows in LDS (32 KB at most, four blocks
//             per CU); a thread owns 4 consecutive rows of one lane and slides over its 4 + 2 R rows once.
// A block of 256 threads is 16 lanes x 16 row groups, so the four 16-lane groups a ds_read_b128 is served in each
// cover the 16 slots of one 256-byte LDS row: no bank conflicts without padding.
// The sum of every output cell runs over ascending source index in one fma chain: bit-reproducible whatever the launch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "fwi_smooth.h"

namespace fwi {

namespace {

constexpr int SM_BLOCK = 256;
constexpr int SM_XL = 16, SM_RG = 16, SM_ROWS = 4;  // y/z pass: lanes along x, row groups, rows per thread
constexpr int SM_TA = SM_RG * SM_ROWS;              // ... rows of a tile along the smoothed axis
constexpr int SM_STAGE = (SM_TA + 2 * SMOOTH_RMAX) / SM_RG;  // ... staged rows per thread at most

template <typename T>
struct alignas(16) Lane {
    T v[16 / sizeof(T)];
};

// w[|k|], zero beyond R (a window vector may reach up to V - 1 or SM_ROWS - 1 cells past R; those terms are skipped)
template <typename T>
struct SmoothW {
    T w[SMOOTH_RMAX + 8];
};

// rho(j); outside one reflection the result lies outside [0, n) and the cell is not read
__device__ inline int mirror(int j, int n) {
    j = j < 0 ? -1 - j : j;
    return j >= n ? 2 * n - 1 - j : j;
}

template <typename T>
__global__ __launch_bounds__(SM_BLOCK) void smooth_x(T *dst, const T *src, int nx, int cx, int64_t nrows, int xtiles,
                                                     int R, SmoothW<T> W) {
    constexpr int V = 16 / sizeof(T), XT = 64 * V, LROW = XT + 2 * SMOOTH_RMAX;
    __shared__ Lane<T> lds_[4 * LROW / V];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int xt = (int)(blockIdx.x % xtiles);
    const int64_t row = (int64_t)(blockIdx.x / xtiles) * 4 + wave;
    const int x0 = xt * XT, gx = x0 + lane * V;
    const bool live = row < nrows;
    T *L = (T *)lds_ + wave * LROW + SMOOTH_RMAX;  // L[i] is the cell x0 + i of this wave's row
    const int RV = (R + V - 1) / V * V;
    if (live) {
        const T *srow = src + row * cx;
        Lane<T> v;
        if (gx + V <= nx) {
            v = *(const Lane<T> *)(srow + gx);
        } else {  // the lane that straddles nx and the ones behind it: mirrored cells, not the pad columns
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const int m = mirror(gx + e, nx);
                v.v[e] = (m >= 0 && m < nx) ? srow[m] : T(0);
            }
        }
        *(Lane<T> *)(L + lane * V) = v;
        if (lane < 2 * RV) {  // halo: RV cells left of the segment, RV right of it
            const int i = lane < RV ? lane - RV : XT + lane - RV;
            const int m = mirror(x0 + i, nx);
            L[i] = (m >= 0 && m < nx) ? srow[m] : T(0);
        }
    }
    __syncthreads();
    if (!live || gx >= cx) return;
    T acc[V];
#pragma unroll
    for (int e = 0; e < V; ++e) acc[e] = T(0);
    for (int jj = -RV; jj <= RV; jj += V) {
        const Lane<T> v = *(const Lane<T> *)(L + lane * V + jj);
#pragma unroll
        for (int i = 0; i < V; ++i) {
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const int d = jj + i - e < 0 ? e - i - jj : jj + i - e;
                if (d <= R) acc[e] = fma(W.w[d], v.v[i], acc[e]);
            }
        }
    }
    Lane<T> out;
#pragma unroll
    for (int e = 0; e < V; ++e) out.v[e] = gx + e < nx ? acc[e] : T(0);
    *(Lane<T> *)(dst + row * cx + gx) = out;
}

// Smooths along an axis of length n whose consecutive cells lie `ls` elements apart; `os` separates the lines' planes
// (y pass: the z planes; z pass: the y rows).
template <typename T>
__global__ __launch_bounds__(SM_BLOCK) void smooth_line(T *dst, const T *src, int n, int64_t ls, int64_t os, int nx,
                                                        int cx, int xtiles, int atiles, int R, SmoothW<T> W) {
    constexpr int V = 16 / sizeof(T);
    __shared__ Lane<T> lds[(SM_TA + 2 * SMOOTH_RMAX) * SM_XL];
    const int xl = threadIdx.x & (SM_XL - 1), rg = threadIdx.x / SM_XL;
    int64_t b = blockIdx.x;
    const int xt = (int)(b % xtiles);
    b /= xtiles;
    const int at = (int)(b % atiles);
    const int64_t outer = b / atiles;
    const int gx = (xt * SM_XL + xl) * V, a0 = at * SM_TA;
    const bool inx = gx < cx;
    const T *sbase = src + outer * os + gx;
    const int nstage = (n - a0 < SM_TA ? n - a0 : SM_TA) + 2 * R;  // LDS row jr is the axis cell a0 - R + jr
    Lane<T> st[SM_STAGE];
#pragma unroll
    for (int k = 0; k < SM_STAGE; ++k) {
        const int jr = rg + k * SM_RG, m = mirror(a0 - R + jr, n);
        Lane<T> v;
#pragma unroll
        for (int i = 0; i < V; ++i) v.v[i] = T(0);
        if (inx && jr < nstage && m >= 0 && m < n) v = *(const Lane<T> *)(sbase + m * ls);
        st[k] = v;
    }
#pragma unroll
    for (int k = 0; k < SM_STAGE; ++k) {
        const int jr = rg + k * SM_RG;
        if (jr < nstage) lds[jr * SM_XL + xl] = st[k];
    }
    __syncthreads();
    const int r0 = rg * SM_ROWS;  // this thread's first row within the tile
    if (!inx || a0 + r0 >= n) return;
    T acc[SM_ROWS][V];
#pragma unroll
    for (int e = 0; e < SM_ROWS; ++e)
#pragma unroll
        for (int i = 0; i < V; ++i) acc[e][i] = T(0);
    // (a thread whose last rows lie behind n reads rows nobody staged, into accumulators it then drops)
    for (int j = 0; j < SM_ROWS + 2 * R; ++j) {
        const Lane<T> v = lds[(r0 + j) * SM_XL + xl];
#pragma unroll
        for (int e = 0; e < SM_ROWS; ++e) {
            const int d = j - R - e < 0 ? R + e - j : j - R - e;
            if (d <= R) {
#pragma unroll
                for (int i = 0; i < V; ++i) acc[e][i] = fma(W.w[d], v.v[i], acc[e][i]);
            }
        }
    }
    T *dbase = dst + outer * os + gx;
#pragma unroll
    for (int e = 0; e < SM_ROWS; ++e) {
        const int a = a0 + r0 + e;
        if (a >= n) break;
        Lane<T> out;
#pragma unroll
        for (int i = 0; i < V; ++i) out.v[i] = gx + i < nx ? acc[e][i] : T(0);
        *(Lane<T> *)(dbase + a * ls) = out;
    }
}

}  // namespace

void smooth_weights(double sigma, int R, double *w) {
    double sum = 0.0;
    for (int k = 0; k <= R; ++k) {
        w[k] = (k == 0) ? 1.0 : std::exp(-0.5 * (double)k * (double)k / (sigma * sigma));
        sum += (k == 0) ? w[k] : 2.0 * w[k];
    }
    for (int k = 0; k <= R; ++k) w[k] /= sum;
}

template <typename T>
hipError_t launch_smooth_axis(const GridDesc &g, T *dst, const T *src, int axis, int R, const T *w, hipStream_t s) {
    constexpr int V = 16 / sizeof(T);
    const int n = axis == 0 ? g.nz : axis == 1 ? g.ny : g.nx;
    if (axis < 0 || axis > 2 || (axis == 1 && g.ndim != 3) || R < 1 || R > SMOOTH_RMAX || R > n || !w || dst == src)
        return hipErrorInvalidValue;
    SmoothW<T> W;
    for (int k = 0; k < SMOOTH_RMAX + 8; ++k) W.w[k] = k <= R ? w[k] : T(0);
    if (axis == 2) {
        const int64_t nrows = (int64_t)g.nz * g.ny;
        const int xtiles = (g.cx + 64 * V - 1) / (64 * V);
        const int64_t blocks = (nrows + 3) / 4 * xtiles;
        if (blocks > 0x7fffffff) return hipErrorInvalidValue;
        hipLaunchKernelGGL(smooth_x<T>, dim3((unsigned)blocks), dim3(SM_BLOCK), 0, s, dst, src, g.nx, g.cx, nrows, xtiles,
                           R, W);
    } else {
        const int64_t plane = (int64_t)g.ny * g.cx;
        const int64_t ls = axis == 0 ? plane : g.cx, os = axis == 0 ? g.cx : plane;
        const int nouter = axis == 0 ? g.ny : g.nz;
        const int xtiles = (g.cx + SM_XL * V - 1) / (SM_XL * V), atiles = (n + SM_TA - 1) / SM_TA;
        const int64_t blocks = (int64_t)xtiles * atiles * nouter;
        if (blocks > 0x7fffffff) return hipErrorInvalidValue;
        hipLaunchKernelGGL(smooth_line<T>, dim3((unsigned)blocks), dim3(SM_BLOCK), 0, s, dst, src, n, ls, os, g.nx, g.cx,
                           xtiles, atiles, R, W);
    }
    return hipGetLastError();
}

template hipError_t launch_smooth_axis<float>(const GridDesc &, float *, const float *, int, int, const float *,
                                              hipStream_t);
template hipError_t launch_smooth_axis<double>(const GridDesc &, double *, const double *, int, int, const double *,
                                               hipStream_t);

}  // namespace fwi
