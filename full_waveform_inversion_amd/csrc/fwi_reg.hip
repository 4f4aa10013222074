// First-order Tikhonov / smoothed isotropic TV regularisation of compact model-sized vectors (fwi_reg.h).  Its own
// object: the step / tile / point / smoothing objects keep their pinned kernel counts.
//
// One launch reads x (x0, v) once, apart from the one-cell halos of its tiles, and writes out once, in 16-byte lanes
// along x.  A block of 256 threads is 16 rows x 16 lanes: a y-x tile of REG_TY rows by 64 (fp32) / 32 (fp64) columns,
// marched over REG_ZC planes.  Per plane z:
//   stage   d = x - x0 (and v) of the plane z + 1, tile plus a one-cell halo, into LDS as fp64 (the plane z is there
//           from the step before: two buffers, alternating);
//   k       every thread forms s and k = 1 / sqrt(s + eps^2) of its own cells and their fluxes F_a = w_a k (D_a v); the
//           k of the row below the tile and of the column left of it are formed once each (one wave's lanes apiece) and
//           all k go to LDS (TV only: Tikhonov has k = 1);
//   out     out_j = alpha (F_x(j - e_x) - F_x(j) + F_y(j - e_y) - F_y(j) + F_z(j - e_z) - F_z(j)) + beta out_j: the low x
//           and y fluxes from the neighbours' k in LDS, the low z flux carried over in registers from the plane before
//           (a chunk that does not start at z = 0 forms it from the plane z0 - 1 first, without output).
// Everything between the loads and the final rounding to T is fp64.  The value R is summed per thread over ascending z,
// then over the block by a fixed tree (fwi_gather_tile.h) into partial[block]; reg_final adds the partials in a fixed
// order.  No atomics.
#include <hip/hip_runtime.h>

#include "fwi_gather_tile.h"
#include "fwi_reg.h"

namespace fwi {

namespace {

constexpr int RG_BLOCK = 256;
static_assert(REG_TY * REG_XL == RG_BLOCK && RG_BLOCK == GT_BLOCK, "one thread per row and lane; the block sum's 256");

template <typename T>
struct alignas(16) Lane {
    T v[16 / sizeof(T)];
};

struct RegArgs {
    int nz, ny, nx, cx;  // the grid as (nz, ny, nx): a 2-D grid has nz = 1
    int xtiles, ytiles;
    double wz, wy, wx, eps, alpha, beta;
};

// Stages the tile of plane z with its halo: rows -1 .. REG_TY, columns -1 .. TX.  A cell outside the grid (the pad
// columns among them) takes the value of the nearest cell inside, so that every difference across an end of an axis is
// an exact zero: the no-flux ends need no masks, and no load leaves the logical array.
template <typename T>
__device__ inline void stage_plane(double *dst, const T *src, const T *src0, const RegArgs &a, int z, int y0, int x0) {
    constexpr int V = 16 / sizeof(T), TX = REG_XL * V, P = TX + 4;
    const int64_t plane = (int64_t)z * a.ny;
    for (int i = threadIdx.x; i < (REG_TY + 2) * REG_XL; i += RG_BLOCK) {
        const int r = i / REG_XL - 1, l = i % REG_XL;
        const int gy = min(max(y0 + r, 0), a.ny - 1), gx = x0 + l * V;
        const int64_t row = (plane + gy) * a.cx;
        double *d = dst + (r + 1) * P + l * V + 2;
        if (gx + V <= a.nx) {
            const Lane<T> p = *(const Lane<T> *)(src + row + gx);
            Lane<T> q;
#pragma unroll
            for (int e = 0; e < V; ++e) q.v[e] = T(0);
            if (src0) q = *(const Lane<T> *)(src0 + row + gx);
#pragma unroll
            for (int e = 0; e < V; ++e) d[e] = (double)p.v[e] - (double)q.v[e];
        } else {  // the lane that straddles nx and the ones behind it
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const int64_t at = row + min(gx + e, a.nx - 1);
                d[e] = (double)src[at] - (src0 ? (double)src0[at] : 0.0);
            }
        }
    }
    if (threadIdx.x < (REG_TY + 2) * 2) {
        const int r = (int)threadIdx.x / 2 - 1, side = threadIdx.x & 1;
        const int gy = min(max(y0 + r, 0), a.ny - 1), gx = min(max(side ? x0 + TX : x0 - 1, 0), a.nx - 1);
        const int64_t at = (plane + gy) * a.cx + gx;
        dst[(r + 1) * P + (side ? TX + 2 : 1)] = (double)src[at] - (src0 ? (double)src0[at] : 0.0);
    }
}

// s of the cell at LDS offset `at` of the plane Dc, Dn the plane above it (Dc itself on the last plane)
__device__ inline double cell_s(const double *Dc, const double *Dn, int at, int P, const RegArgs &a) {
    const double d0 = Dc[at];
    const double ex = Dc[at + 1] - d0, ey = Dc[at + P] - d0, ez = Dn[at] - d0;
    return a.wx * ex * ex + a.wy * ey * ey + a.wz * ez * ez;
}

template <typename T, bool TV, bool HASV>
__global__ __launch_bounds__(RG_BLOCK) void reg_apply(T *out, const T *x, const T *xp, const T *v, RegArgs a,
                                                      double *partial) {
    constexpr int V = 16 / sizeof(T), TX = REG_XL * V, P = TX + 4, PLANE = (REG_TY + 2) * P, KP = TX + 1;
    __shared__ double sD[2][PLANE];
    __shared__ double sV[HASV ? 2 : 1][HASV ? PLANE : 1];
    __shared__ double sK[TV ? (REG_TY + 1) * KP : 1];  // k of the cell (r, c) at (r + 1) * KP + c + 1, r and c from -1
    __shared__ double sRed[RG_BLOCK];
    const int tid = threadIdx.x, r = tid / REG_XL, l = tid % REG_XL;
    int b = blockIdx.x;
    const int x0 = (b % a.xtiles) * TX;
    b /= a.xtiles;
    const int y0 = (b % a.ytiles) * REG_TY, z0 = (b / a.ytiles) * REG_ZC;
    const int zend = z0 + REG_ZC < a.nz ? z0 + REG_ZC : a.nz;
    const int gy = y0 + r, gx0 = x0 + l * V, c0 = l * V;
    const int at0 = (r + 1) * P + c0 + 2;  // LDS offset of this thread's first cell
    const double eps2 = a.eps * a.eps;
    double fzprev[V], acc = 0.0;
#pragma unroll
    for (int e = 0; e < V; ++e) fzprev[e] = 0.0;

    const int zs = z0 > 0 ? z0 - 1 : 0;
    stage_plane<T>(sD[zs & 1], x, xp, a, zs, y0, x0);
    if (HASV) stage_plane<T>(sV[zs & 1], v, nullptr, a, zs, y0, x0);
    for (int z = zs; z < zend; ++z) {
        const bool hz = z < a.nz - 1, emit = z >= z0, flux = emit && out != nullptr;
        if (hz) {
            stage_plane<T>(sD[(z + 1) & 1], x, xp, a, z + 1, y0, x0);
            if (HASV) stage_plane<T>(sV[(z + 1) & 1], v, nullptr, a, z + 1, y0, x0);
        }
        __syncthreads();
        const double *Dc = sD[z & 1], *Dn = hz ? sD[(z + 1) & 1] : Dc;  // the last plane: an exact zero difference
        const double *Vc = HASV ? sV[z & 1] : Dc, *Vn = !HASV ? Dn : hz ? sV[(z + 1) & 1] : Vc;
        double fx[V], fy[V], fz[V];
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const int at = at0 + e;
            const double s = cell_s(Dc, Dn, at, P, a);
            double k = 1.0, term = 0.5 * s;
            if (TV) {
                const double q = s + eps2;
                k = rsqrt(q);
                term = s / (q * k + a.eps);  // sqrt(q) - eps without the cancellation
                if (flux) sK[(r + 1) * KP + c0 + e + 1] = k;
            }
            if (emit && gy < a.ny && gx0 + e < a.nx) acc += term;  // (not the copies outside the grid)
            const double v0 = Vc[at];
            fx[e] = a.wx * k * (Vc[at + 1] - v0);
            fy[e] = a.wy * k * (Vc[at + P] - v0);
            fz[e] = a.wz * k * (Vn[at] - v0);
        }
        if (TV && flux) {
            if (tid < TX) {  // the row below the tile
                sK[tid + 1] = rsqrt(cell_s(Dc, Dn, tid + 2, P, a) + eps2);
            } else if (tid >= 64 && tid < 64 + REG_TY) {  // the column left of it
                const int rr = tid - 64;
                sK[(rr + 1) * KP] = rsqrt(cell_s(Dc, Dn, (rr + 1) * P + 1, P, a) + eps2);
            }
        }
        __syncthreads();
        if (flux && gy < a.ny && gx0 < a.cx) {
            const int64_t o = ((int64_t)z * a.ny + gy) * a.cx + gx0;
            Lane<T> old, res;
            if (a.beta != 0.0) old = *(const Lane<T> *)(out + o);
            // the low x flux of the first cell comes from the neighbouring lane's (or tile's) last cell; at x = 0 and
            // y = 0 the low fluxes are exact zeros (the staged copies)
            double fl = a.wx * (TV ? sK[(r + 1) * KP + c0] : 1.0) * (Vc[at0] - Vc[at0 - 1]);
#pragma unroll
            for (int e = 0; e < V; ++e) {
                // the low y flux: the cell one row below
                const double fb = a.wy * (TV ? sK[r * KP + c0 + e + 1] : 1.0) * (Vc[at0 + e] - Vc[at0 + e - P]);
                double val = a.alpha * (((fl - fx[e]) + (fb - fy[e])) + (fzprev[e] - fz[e]));
                if (a.beta != 0.0) val += a.beta * (double)old.v[e];
                res.v[e] = gx0 + e < a.nx ? (T)val : T(0);
                fl = fx[e];
            }
            *(Lane<T> *)(out + o) = res;
        }
#pragma unroll
        for (int e = 0; e < V; ++e) fzprev[e] = fz[e];
        __syncthreads();  // the next step stages the plane z + 2 where the plane z lies
    }
    block_tree_sum_to_partial(acc, sRed, partial);
}

// partial[n] = sum of partial[0 .. n): strided per thread, then a fixed tree
__global__ __launch_bounds__(RG_BLOCK) void reg_final(double *partial, int64_t n) {
    __shared__ double sRed[RG_BLOCK];
    const int tid = threadIdx.x;
    double acc = 0.0;
    for (int64_t i = tid; i < n; i += RG_BLOCK) acc += partial[i];
    sRed[tid] = acc;
    __syncthreads();
    for (int s = RG_BLOCK / 2; s > 0; s >>= 1) {
        if (tid < s) sRed[tid] += sRed[tid + s];
        __syncthreads();
    }
    if (tid == 0) partial[n] = sRed[0];
}

struct RegGrid {
    int nz, ny, nx;
};

inline RegGrid reg_grid(const GridDesc &g) {
    return g.ndim == 2 ? RegGrid{1, g.nz, g.nx} : RegGrid{g.nz, g.ny, g.nx};
}

}  // namespace

template <typename T>
int64_t reg_blocks(const GridDesc &g) {
    constexpr int TX = REG_XL * (16 / (int)sizeof(T));
    const RegGrid rg = reg_grid(g);
    return (int64_t)((g.cx + TX - 1) / TX) * ((rg.ny + REG_TY - 1) / REG_TY) * ((rg.nz + REG_ZC - 1) / REG_ZC);
}

template <typename T>
hipError_t launch_regularizer(const GridDesc &g, int kind, T *out, const T *x, const T *x0, const T *v, double alpha,
                              double beta, const double w[3], double eps, double *partial, hipStream_t s) {
    constexpr int TX = REG_XL * (16 / (int)sizeof(T));
    const int64_t blocks = reg_blocks<T>(g);
    if ((kind != REG_TIKHONOV && kind != REG_TV) || !x || !w || !partial || blocks < 1 || blocks > 0x7fffffff ||
        (out && (out == x || out == x0 || out == v)))
        return hipErrorInvalidValue;
    const RegGrid rg = reg_grid(g);
    RegArgs a;
    a.nz = rg.nz, a.ny = rg.ny, a.nx = rg.nx, a.cx = g.cx;
    a.xtiles = (g.cx + TX - 1) / TX, a.ytiles = (rg.ny + REG_TY - 1) / REG_TY;
    a.wz = g.ndim == 2 ? 0.0 : w[0], a.wy = g.ndim == 2 ? w[0] : w[1], a.wx = w[2];
    a.eps = eps, a.alpha = alpha, a.beta = beta;
    const dim3 grid((unsigned)blocks), block(RG_BLOCK);
    if (kind == REG_TV) {
        if (v)
            hipLaunchKernelGGL((reg_apply<T, true, true>), grid, block, 0, s, out, x, x0, v, a, partial);
        else
            hipLaunchKernelGGL((reg_apply<T, true, false>), grid, block, 0, s, out, x, x0, v, a, partial);
    } else {
        if (v)
            hipLaunchKernelGGL((reg_apply<T, false, true>), grid, block, 0, s, out, x, x0, v, a, partial);
        else
            hipLaunchKernelGGL((reg_apply<T, false, false>), grid, block, 0, s, out, x, x0, v, a, partial);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_sum_partials(partial, blocks, s);
}

hipError_t launch_sum_partials(double *partial, int64_t n, hipStream_t s) {
    hipLaunchKernelGGL(reg_final, dim3(1), dim3(RG_BLOCK), 0, s, partial, n);
    return hipGetLastError();
}

template int64_t reg_blocks<float>(const GridDesc &);
template int64_t reg_blocks<double>(const GridDesc &);
template hipError_t launch_regularizer<float>(const GridDesc &, int, float *, const float *, const float *,
                                              const float *, double, double, const double *, double, double *,
                                              hipStream_t);
template hipError_t launch_regularizer<double>(const GridDesc &, int, double *, const double *, const double *,
                                               const double *, double, double, const double *, double, double *,
                                               hipStream_t);

}  // namespace fwi
