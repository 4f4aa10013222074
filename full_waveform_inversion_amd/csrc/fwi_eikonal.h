// First-arrival traveltimes (first-order Godunov eikonal solver) and their discrete adjoint on compact model-sized
// vectors, plus the two point primitives that move receiver values in and out of a vector (fwi_eikonal*,
// fwi_vec_scatter_points, fwi_vec_gather_points).  Internal launch interface between fwi_api_eikonal.hip and
// fwi_eikonal.hip.  The scheme is defined by the NumPy twin, full_waveform_inversion_amd/eikonal.py:
//
//   t_d = min(T[i - e_d], T[i + e_d]) per axis (outside the grid: +inf; tie: the lower-index neighbour is upwind),
//   sorted a <= b <= c, f = h / c_i, b' = b - a, c' = c - a,
//   G_i = a + f                                        if <= b,
//         a + (b' + sqrt(2 f^2 - b'^2)) / 2            else if <= c (2-D: always),
//         a + (S + sqrt(S^2 - 3 (Q - f^2))) / 3        else, S = b' + c', Q = b'^2 + c'^2;
//   T <- min(T, G(T)) from T_init (the listed nodes, +inf elsewhere) until nothing changes.
//   Adjoint at the fixed point: active axes D = {d : t_d < T_i}, den = sum_D (T_i - t_d),
//   dG_i/dt_d = (T_i - t_d) / den, dG_i/ds_i = h^2 / (c_i den), all zero where T_i < G_i (source-determined) or T_i = inf;
//   lambda = b + A^T lambda.
//
// Both iterations are block Jacobi with a ping-pong pair: a workgroup owns a tile, loads it with a frozen halo into LDS,
// runs K inner sweeps and writes its interior to the OTHER array, so the result of a launch depends on its input array
// only (no data crosses workgroups inside a launch; equal inputs give equal bits).  *flag is raised (atomic max) when
// any interior cell of the launch changed.
//
// No reference counterpart.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fwi_kernels.h"

namespace fwi {

// Tile edge of a workgroup (one thread per cell): 16 x 16 in 2-D, 8 x 8 x 8 in 3-D, and the default number of inner
// sweeps per launch (what crosses half a tile)
constexpr int EIK_TILE2 = 16, EIK_TILE3 = 8;
constexpr int EIK_K2 = 8, EIK_K3 = 4;
constexpr int EIK_KMAX = 64;
inline int eik_default_k(const GridDesc &g) { return g.ndim == 2 ? EIK_K2 : EIK_K3; }

// t := +inf on the grid's cells, 0 in the pad columns
template <typename T>
hipError_t launch_eikonal_fill(const GridDesc &g, T *t, hipStream_t s);
// t[idx[k]] = (1 / c[ref]) * dist[k] for k < n, in both arrays (compact indices, validated by the caller)
template <typename T>
hipError_t launch_eikonal_init(T *t0, T *t1, const T *c, const int64_t *idx, const T *dist, int64_t ref, int n,
                               hipStream_t s);
// out := K inner sweeps of min(T, G) on every tile of `in`; *flag = max(*flag, 1) if a cell changed
template <typename T>
hipError_t launch_eikonal_sweep(const GridDesc &g, const T *in, T *out, const T *c, double h, int K, int *flag,
                                hipStream_t s);
// out := K inner sweeps of lam <- b + A^T lam on every tile of `in` (A from `t` and `c`); flag as above
template <typename T>
hipError_t launch_eikonal_adjoint_sweep(const GridDesc &g, const T *t, const T *b, const T *in, T *out, const T *c,
                                        double h, int K, int *flag, hipStream_t s);
// out := beta out + g, g = (dG/ds) lam turned into the gradient with respect to velocity (-g_s / c^2) or to 1 / c^2
// (g_s c / 2); beta == 0: out is not read.  Then, by one thread in list order, the source term: the sum of
// dist[k] lam[idx[k]] over the listed nodes with T < G, converted likewise, is added to out[ref].  n == 0: no list.
template <typename T>
hipError_t launch_eikonal_gradient(const GridDesc &g, const T *t, const T *lam, const T *c, T *out, double h,
                                   double beta, int wrt_velocity, const int64_t *idx, const T *dist, int64_t ref, int n,
                                   hipStream_t s);
// x := beta x over the whole compact array (beta == 0: zeros, x is not read), then x[idx[k]] += v[k] (unique nodes)
template <typename T>
hipError_t launch_scatter_points(T *x, int64_t npts, double beta, const int64_t *idx, const T *v, int n, hipStream_t s);
// out[k] = x[idx[k]] as doubles
template <typename T>
hipError_t launch_gather_points(const T *x, const int64_t *idx, double *out, int n, hipStream_t s);

}  // namespace fwi
